#!/usr/bin/env python3
"""What routed bank calls (kws_bank_run_classifier_routed_device, kws_bank_live_route, kws_bank_scan_recordings_routed_device,
kws_bank_slide_recordings_routed_device; include/kws/kws.h) cost beside the two routes a multi-tenant caller had before, on one MI355X.

Four workloads (--workloads picks among them), every variant in the same process and library, all KWS_MODE_EXACT (bank calls always are):
  batch   --clips resident clips, the four shipped 49x40 models as one bank, one-hot round-robin routes (clip i -> member i mod 4):
            routed     one kws_bank_run_classifier_routed_device call
            unrouted   the unrouted bank call on the same batch (every member scores every clip: a superset of the routed call's work)
            own        the four members' own calls on four contiguous quarter batches (as many (clip, model) pairs as the routed call)
  live    a 16-member bank of the l476 model and fifteen more handles of the same file, --streams live streams with streams / 16 per
          member, one slice of 4000 samples (250 ms) per push, in steady state (every push returns one window per stream):
            routed     one push of the routed bank session
            own        sixteen pushes, one per member's own session of streams / 16 streams
  scan    the same 16-member bank, sixteen recordings of --seconds s each (225 s: one hour in all) at the shipped slicing of 4000 samples,
          recording k routed to member k:
            routed     one kws_bank_scan_recordings_routed_device call
            unrouted   the unrouted bank scan of the same audio (every member scores every window)
            own        sixteen kws_scan_recordings_device calls, one recording each
  slide   the same bank, recordings and routes, one one-shot window every 1600 samples (100 ms), without features:
            routed / unrouted / own   as for the scan, with kws_bank_slide_recordings_routed_device / kws_slide_recordings_device
Every variant: --warmup untimed steps, then --steps steps between two device events; the variants of one workload alternate, --repeats
times; every repeat is reported, with the median and the spread (max - min).  Before anything is timed the routed rows are compared with
the other variants' rows for the same (row, member) pairs: they must be the same bits.
The bar (batch, scan, slide): the routed call's median must not exceed the unrouted call's by more than the spread between the repeats of
the latter.  The comparison with the members' own calls and the live figures are recorded, not gated.  The process ends with status 1 when
the bar is missed.
One process, one workload after the other, each under its own time limit (--limit seconds: the process ends there, starting nothing more).
One JSON line per (workload, variant), appended to --out; --md FILE writes the tables from --out's lines (no GPU needed for that step).

usage: gpu_bank_route_rate.py [--workloads batch,live,scan,slide] [--clips 65536] [--streams 1024] [--seconds 225] [--steps 20] [--warmup 3] [--repeats 7] [--out FILE.jsonl]
       gpu_bank_route_rate.py --md profiles/bank_route_rate.md --out FILE.jsonl
"""
import argparse
import json
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFCC40 = ["cfg2_mfcc40_int8", "cfg2_mfcc40_f32", "cfg5_dscnn_mfcc40_int8", "cfg5_dscnn_mfcc40_f32"]
LIVE_MODEL, LIVE_MEMBERS, SLICE = "l476_no_yes", 16, 4000
SLIDE_HOP = 1600
BARRED = ("batch", "scan", "slide")


class StepLimit:
    """ends the process when the block takes longer than `seconds`: nothing more is started on the GPU after that"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def out_of_time(*_):
            print("%s: over its limit of %d s" % (self.what, self.seconds), file=sys.stderr, flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, out_of_time)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def timed(torch, fn, steps, warmup):
    """seconds per step between two device events on the stream the calls are enqueued on"""
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / steps


def measure(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fout = open(a.out, "a")

    def run(workload, variants, check, **facts):
        """variants: name -> callable; alternating, a.repeats times"""
        with StepLimit(workload, a.limit):
            for fn in variants.values():
                fn()
            assert check(), "%s: the routed rows differ from the other variants'" % workload
            times = {v: [] for v in variants}
            for _ in range(a.repeats):
                for v, fn in variants.items():
                    times[v].append(timed(torch, fn, a.steps, a.warmup))
        for v, ts in times.items():
            line = json.dumps(dict(workload=workload, variant=v, steps=a.steps, warmup=a.warmup, seconds_per_step=ts, median_ms=statistics.median(ts) * 1e3,
                                   spread_ms=(max(ts) - min(ts)) * 1e3, same_bits=True, **facts))
            print(line, flush=True)
            fout.write(line + "\n")
            fout.flush()
        return {v: statistics.median(ts) for v, ts in times.items()}, {v: max(ts) - min(ts) for v, ts in times.items()}

    def bits(t):
        return t.view(torch.int32)

    wanted = set(a.workloads.split(","))
    assert wanted and wanted <= {"batch", "live", "scan", "slide"}, a.workloads
    missed = []

    def bar(workload, med, spread):
        if med["routed"] > med["unrouted"] + spread["unrouted"]:
            missed.append("%s: routed %.3f ms > unrouted %.3f ms + its spread %.3f ms" % (workload, med["routed"] * 1e3, med["unrouted"] * 1e3, spread["unrouted"] * 1e3))

    if "batch" in wanted:
        # ---- batch: one-hot round-robin routes over resident clips
        models = [pkg.Model(os.path.join(ROOT, "models", m + ".kwsm")) for m in MFCC40]
        bank = pkg.Bank(models)
        K, B, clip = len(models), a.clips - a.clips % len(models), models[0].clip_samples
        pcm = torch.empty((B, clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(23, 0, B, clip, pcm.data_ptr())
        routes = (np.uint32(1) << (np.arange(B) % K).astype(np.uint32)).astype(np.uint32)

        def outs():
            return [torch.zeros((B, m.n_labels), dtype=torch.float32, device="cuda") for m in models]
        sr, su, so = outs(), outs(), outs()
        q = B // K

        def batch_routed():
            bank.run_classifier_routed_device(pcm.data_ptr(), B, routes, [t.data_ptr() for t in sr])

        def batch_unrouted():
            bank.run_classifier_batch_device(pcm.data_ptr(), B, [t.data_ptr() for t in su])

        def batch_own():
            for k, m in enumerate(models):
                m.run_classifier_batch_device(pcm[k * q:].data_ptr(), q, so[k][k * q:].data_ptr())

        def batch_check():
            torch.cuda.synchronize()
            ok = all(torch.equal(bits(sr[k])[k::K], bits(su[k])[k::K]) for k in range(K))
            # (the quarter batches hold other clips than the one-hot rows: compared with the unrouted bank's rows of the same clips)
            return ok and all(torch.equal(bits(so[k])[k * q:(k + 1) * q], bits(su[k])[k * q:(k + 1) * q]) for k in range(K))
        med, spread = run("batch", {"routed": batch_routed, "unrouted": batch_unrouted, "own": batch_own}, batch_check, clips=B, members=MFCC40)
        bar("batch", med, spread)
        torch.cuda.synchronize()
        bank.close()
        for m in models:
            m.close()
        del pcm, sr, su, so

    if wanted & {"live", "scan", "slide"}:
        models = [pkg.Model(os.path.join(ROOT, "models", LIVE_MODEL + ".kwsm")) for _ in range(LIVE_MEMBERS)]
        bank = pkg.Bank(models)
    if "live" in wanted:
        # ---- live: 16 handles of one model, streams / 16 streams per member, one slice per push
        K, S = len(models), a.streams - a.streams % len(models)
        per = S // K
        n_push = 16
        pcm = torch.empty((S * n_push * SLICE // 16000 + 1, 16000), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(29, 0, pcm.shape[0], 16000, pcm.data_ptr())
        lv = bank.live_streams(S, SLICE)
        lv.route(np.arange(S), (np.uint32(1) << (np.arange(S) // per).astype(np.uint32)).astype(np.uint32))     # streams [k per, (k + 1) per) -> member k
        own = [m.live_streams(per, SLICE) for m in models]
        sb = [torch.zeros((S, m.n_labels), dtype=torch.float32, device="cuda") for m in models]
        so = [torch.zeros((per, m.n_labels), dtype=torch.float32, device="cuda") for m in models]
        streams, lens = np.arange(S), np.full(S, SLICE)
        step, counts = {"routed": 0, "own": 0}, {}

        def offs(which):
            # every push hands each stream the next slice of its own audio; both variants walk the same audio, wrapping together
            i = step[which] % n_push
            step[which] += 1
            return (np.arange(S) * n_push + i) * SLICE

        def live_routed():
            counts["routed"] = int(lv.push_device(pcm.data_ptr(), streams, offs("routed"), lens, [t.data_ptr() for t in sb]).sum())

        def live_own():
            o = offs("own")
            counts["own"] = sum(int(own[k].push_device(pcm.data_ptr(), streams[:per], o[k * per:(k + 1) * per], lens[:per], so[k].data_ptr()).sum()) for k in range(K))

        def live_check():
            torch.cuda.synchronize()
            return step["routed"] == step["own"] and counts == {"routed": S, "own": S} and \
                all(torch.equal(bits(sb[k])[k * per:(k + 1) * per], bits(so[k])) for k in range(K))
        for _ in range(16000 // SLICE + 3):                                   # up to steady state: a window per stream and push
            live_routed()
            live_own()
        run("live", {"routed": live_routed, "own": live_own}, live_check, streams=S, members=[LIVE_MODEL] * K, slice_samples=SLICE)
        torch.cuda.synchronize()
        lv.close()
        for o in own:
            o.close()
    # ---- scan and slide: sixteen recordings, recording k routed to member k
    if wanted & {"scan", "slide"}:
        K = len(models)
        n_rec = a.seconds * 16000
        pcm = torch.empty((K * a.seconds, 16000), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(31, 0, pcm.shape[0], 16000, pcm.data_ptr())
        offs, lens = np.arange(K, dtype=np.uint64) * np.uint64(n_rec), np.full(K, n_rec, np.uint64)
        routes = (np.uint32(1) << np.arange(K).astype(np.uint32)).astype(np.uint32)
    for w in ("scan", "slide"):
        if w not in wanted:
            continue
        W = models[0].scan_window_count(n_rec, SLICE) if w == "scan" else models[0].slide_window_count(n_rec, SLIDE_HOP)
        sr, su = ([torch.zeros((K * W, m.n_labels), dtype=torch.float32, device="cuda") for m in models] for _ in range(2))
        so = [torch.zeros((W, m.n_labels), dtype=torch.float32, device="cuda") for m in models]

        def rec_routed(w=w, sr=sr):
            if w == "scan":
                bank.scan_recordings_device(pcm.data_ptr(), offs, lens, [t.data_ptr() for t in sr], None, slice_samples=SLICE, routes=routes)
            else:
                bank.slide_recordings_device(pcm.data_ptr(), offs, lens, SLIDE_HOP, [t.data_ptr() for t in sr], routes=routes)

        def rec_unrouted(w=w, su=su):
            if w == "scan":
                bank.scan_recordings_device(pcm.data_ptr(), offs, lens, [t.data_ptr() for t in su], None, slice_samples=SLICE)
            else:
                bank.slide_recordings_device(pcm.data_ptr(), offs, lens, SLIDE_HOP, [t.data_ptr() for t in su])

        def rec_own(w=w, so=so):
            for k, m in enumerate(models):
                if w == "scan":
                    m.scan_recordings_device(pcm.data_ptr(), offs[k:k + 1], lens[k:k + 1], so[k].data_ptr(), None, slice_samples=SLICE)
                else:
                    m.slide_recordings_device(pcm.data_ptr(), offs[k:k + 1], lens[k:k + 1], SLIDE_HOP, so[k].data_ptr())

        def rec_check(W=W, sr=sr, su=su, so=so):
            torch.cuda.synchronize()
            rows = lambda t, k: bits(t)[k * W:(k + 1) * W]
            return all(torch.equal(rows(sr[k], k), rows(su[k], k)) and torch.equal(rows(sr[k], k), bits(so[k])) and bool(so[k].any()) for k in range(K))
        med, spread = run(w, {"routed": rec_routed, "unrouted": rec_unrouted, "own": rec_own}, rec_check, recordings=K, seconds=a.seconds, windows=K * W,
                          members=[LIVE_MODEL] * K, **(dict(slice_samples=SLICE) if w == "scan" else dict(hop_samples=SLIDE_HOP)))
        bar(w, med, spread)
        torch.cuda.synchronize()
        del sr, su, so
    if wanted & {"live", "scan", "slide"}:
        bank.close()
        for m in models:
            m.close()
    fout.close()
    if missed:
        print("the bar is missed: " + "; ".join(missed), file=sys.stderr)
        sys.exit(1)


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    cells = {}
    for d in rows:
        cells.setdefault(d["workload"], {})[d["variant"]] = d
    first = rows[0]
    out = ["# Routed banks: each clip or stream scored only by the members it names", "",
           "One MI355X, KWS_MODE_EXACT kernels in every variant (bank calls always run them), every variant in one process and library.  Per variant: %d "
           "warm-up steps, then %d timed steps between two device events, the variants of a workload alternating, %d repeats; all repeats are listed, "
           "with their median and spread (max - min).  Before timing, the routed rows were compared with the other variants' rows of the same (row, "
           "member) pairs: same bits.  Times are per step of the whole call on the device (enqueue to last kernel), not kernel times.  Written by "
           "tools/gpu_bank_route_rate.py." % (first["warmup"], first["steps"], len(first["seconds_per_step"])), ""]
    what = {("batch", "routed"): "one routed bank call, one-hot round-robin routes", ("batch", "unrouted"): "the unrouted bank call, every member on every clip",
            ("batch", "own"): "the four members' own calls on four contiguous quarter batches", ("live", "routed"): "one push of the routed bank session",
            ("live", "own"): "sixteen pushes, one per member's own session",
            ("scan", "routed"): "one routed bank scan, recording k to member k", ("scan", "unrouted"): "the unrouted bank scan, every member on every window",
            ("scan", "own"): "sixteen own scans, one recording each",
            ("slide", "routed"): "one routed bank slide, recording k to member k", ("slide", "unrouted"): "the unrouted bank slide, every member on every window",
            ("slide", "own"): "sixteen own slides, one recording each"}
    for w, title in (("batch", "Batch: %d resident clips, the four 49x40 models as one bank"), ("live", "Live: %d streams, a 16-member bank of the l476 model, one 250 ms slice per push"),
                     ("scan", "Scan: %d windows of sixteen recordings (one hour of audio), a 16-member bank of the l476 model, slices of 4000 samples"),
                     ("slide", "Slide: %d windows of the same recordings, the same bank, one window every 1600 samples (100 ms)")):
        if w not in cells:
            out += ["## " + title.replace("%d ", ""), "", "not measured", ""]
            continue
        any_row = next(iter(cells[w].values()))
        out += ["## " + title % (any_row.get("clips") or any_row.get("streams") or any_row.get("windows")), "", "| variant | median ms | spread ms | every repeat, ms |", "|---|---|---|---|"]
        for v, d in cells[w].items():
            out.append("| %s | %.3f | %.3f | %s |" % (what[(w, v)], d["median_ms"], d["spread_ms"], " ".join("%.3f" % (t * 1e3) for t in d["seconds_per_step"])))
        out.append("")
        if w in BARRED and {"routed", "unrouted"} <= set(cells[w]):
            r, u = cells[w]["routed"], cells[w]["unrouted"]
            ok = r["median_ms"] <= u["median_ms"] + u["spread_ms"]
            out += ["The bar: the routed call's median (%.3f ms) must not exceed the unrouted call's (%.3f ms) by more than the spread between the latter's "
                    "repeats (%.3f ms): %s.  The comparison with the members' own calls and the live figures are recorded, not gated."
                    % (r["median_ms"], u["median_ms"], u["spread_ms"], "met" if ok else "MISSED"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="batch,live,scan,slide")
    ap.add_argument("--seconds", type=int, default=225, help="length of each of the sixteen recordings of the scan and slide workloads")
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds each workload may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "bank_route_rate.jsonl"))
    ap.add_argument("--md", default=None, help="write the tables from --out; runs nothing")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
