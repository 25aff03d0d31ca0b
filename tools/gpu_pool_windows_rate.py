#!/usr/bin/env python3
"""What the pool's window calls (kws_pool_scan_recordings_device, kws_pool_slide_recordings_device, kws_pool_slide_live_*,
kws_pool_cmvn_inference_device; include/kws/kws.h) cost beside the routed-bank calls a many-tenant caller had before, on one MI355X.

The method is tools/gpu_pool_rate.py's: the same 256 synthetic tenants of the 49 x 40 stock graph (--tenants), every variant in one process
and library, all KWS_MODE_EXACT; per variant --warmup untimed steps, then --steps steps between two device events, the variants of a
workload alternating, --repeats times; every repeat is reported, with the median and the spread (max - min).  Before anything is timed the
pool's rows are compared with the other variant's rows of the same (window, member) pairs: they must be the same bits.  The baseline of
every bar is existing code: routed-bank calls, 16 banks of 16 members, back to back on one stream.  Workloads (--workloads picks among them):
  scan      BAR A.  --seconds of audio (one hour) in 256 recordings, recording r -> tenant r, slices of 4000 samples:
              pool   one kws_pool_scan_recordings_device call
              banks  sixteen kws_bank_scan_recordings_routed_device calls of 16 recordings each, one-hot routes
  slide     BAR B.  the same audio, one window every 1600 samples (100 ms): kws_pool_slide_recordings_device against sixteen
            kws_bank_slide_recordings_routed_device calls
  live      BAR C.  --streams live one-shot streams of 256 tenants, one packet of 1600 samples per push at a hop of 1600, in steady state
            (a window per stream and push): one kws_pool_slide_live_push_device against sixteen routed kws_bank_slide_live_push_device calls
  scan16    recorded only: the first 16 recordings and tenants, one pool scan against ONE routed-bank scan on the same 16 handles
  cepstra   recorded only: --clips rows, row i -> tenant i mod 256: kws_pool_cmvn_inference_device on the first member's cepstra against
            kws_pool_run_classifier_device on the clips -- the difference is the front end's share
Each bar: the pool's median plus the spread between its repeats must stay below the sixteen routed-bank calls' median.  The process ends
with status 1 when a bar is missed.  One JSON line per (workload, variant), appended to --out; --md FILE writes the tables from --out's
lines (no GPU needed for that step).

usage: gpu_pool_windows_rate.py [--workloads scan,slide,live,scan16,cepstra] [--out FILE.jsonl]
       gpu_pool_windows_rate.py --md profiles/pool_windows_rate.md --out FILE.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_pool_rate import BANK, LABELS, SLICE, TENANTS, StepLimit, tenant_paths, timed  # noqa: E402

HOP = 1600                     # 100 ms
BARS = {"scan": "A", "slide": "B", "live": "C"}


def measure(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    wanted = a.workloads.split(",")
    assert wanted and set(wanted) <= {"scan", "slide", "live", "scan16", "cepstra"}, a.workloads
    pkg = load_package()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fout = open(a.out, "a")
    missed = []

    def emit(**d):
        line = json.dumps(d)
        print(line, flush=True)
        fout.write(line + "\n")
        fout.flush()

    def run(workload, variants, check, **facts):
        """variants: name -> callable; alternating, a.repeats times; returns the medians and spreads"""
        with StepLimit(workload, a.limit):
            for fn in variants.values():
                fn()
            assert check(), "%s: the pool's rows differ from the other variant's" % workload
            times = {v: [] for v in variants}
            for _ in range(a.repeats):
                for v, fn in variants.items():
                    times[v].append(timed(torch, fn, a.steps, a.warmup))
        for v, ts in times.items():
            emit(workload=workload, variant=v, steps=a.steps, warmup=a.warmup, seconds_per_step=ts, median_ms=statistics.median(ts) * 1e3,
                 spread_ms=(max(ts) - min(ts)) * 1e3, same_bits=True, **facts)
        med, spread = {v: statistics.median(ts) for v, ts in times.items()}, {v: max(ts) - min(ts) for v, ts in times.items()}
        if workload in BARS and med["pool"] + spread["pool"] >= med["banks"]:
            missed.append("bar %s: pool %.3f ms + its spread %.3f ms >= sixteen routed-bank calls %.3f ms"
                          % (BARS[workload], med["pool"] * 1e3, spread["pool"] * 1e3, med["banks"] * 1e3))

    def bits(t):
        return t.view(torch.int32)

    def zeros(rows, cols):
        return torch.zeros((rows, cols), dtype=torch.float32, device="cuda")

    models = [pkg.Model(p) for p in tenant_paths(a.tenants, TENANTS)]
    assert all(m.nn_kernel == "kws_nn_mfma_kernel" for m in models)
    clip, stride = models[0].clip_samples, max(LABELS)
    pool = pkg.Pool(models)
    banks = [pkg.Bank(models[b * BANK:(b + 1) * BANK]) for b in range(BANK)]
    onehot = (np.uint32(1) << np.arange(BANK, dtype=np.uint32)).astype(np.uint32)

    # ---- the recordings: --seconds of audio, one recording per tenant
    per = a.seconds * 16000 // TENANTS
    offs, lens = np.arange(TENANTS, dtype=np.uint64) * np.uint64(per), np.full(TENANTS, per, np.uint64)
    audio = None
    if set(wanted) & {"scan", "slide", "scan16"}:
        n_clips = (TENANTS * per + clip - 1) // clip
        audio = torch.empty((n_clips, clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(31, 0, n_clips, clip, audio.data_ptr())

    def recording_calls(workload, W, pool_call, bank_call, n_banks=BANK, **facts):
        """W windows per recording; pool_call(member, scores); bank_call(bank index, recordings slice, routes, [scores])"""
        n_rec = n_banks * BANK
        sp = zeros(n_rec * W, stride)
        sb = [[zeros(BANK * W, m.n_labels) for m in banks[b].members] for b in range(n_banks)]
        member = np.arange(n_rec, dtype=np.uint32)

        def f_pool():
            pool_call(member, sp)

        def f_banks():
            for b in range(n_banks):
                bank_call(b, slice(b * BANK, (b + 1) * BANK), onehot, [t.data_ptr() for t in sb[b]])

        def check():
            torch.cuda.synchronize()
            for k in range(n_rec):
                b, j = divmod(k, BANK)
                rows = bits(sp)[k * W:(k + 1) * W, :models[k].n_labels]
                if not torch.equal(rows, bits(sb[b][j])[j * W:(j + 1) * W]) or not bool(sb[b][j][j * W:(j + 1) * W].any()):
                    return False
            return True
        run(workload, {"pool": f_pool, "banks" if n_banks > 1 else "bank": f_banks}, check, recordings=n_rec, samples_per_recording=int(per),
            windows=n_rec * W, tenants=n_rec, **facts)

    def scan_pool(p):
        return lambda member, s: p.scan_recordings_device(audio.data_ptr(), offs[:member.size], lens[:member.size], member, s.data_ptr(), None, slice_samples=SLICE)

    def scan_bank(b, at, routes, ptrs):
        banks[b].scan_recordings_device(audio.data_ptr(), offs[at], lens[at], ptrs, None, slice_samples=SLICE, routes=routes)

    if "scan" in wanted:
        recording_calls("scan", models[0].scan_window_count(per, SLICE), scan_pool(pool), scan_bank, slice_samples=SLICE)
    if "slide" in wanted:
        recording_calls("slide", models[0].slide_window_count(per, HOP),
                        lambda member, s: pool.slide_recordings_device(audio.data_ptr(), offs, lens, member, HOP, s.data_ptr(), None),
                        lambda b, at, routes, ptrs: banks[b].slide_recordings_device(audio.data_ptr(), offs[at], lens[at], HOP, ptrs, None, routes=routes),
                        hop_samples=HOP)
    if "scan16" in wanted:
        pool16 = pkg.Pool(models[:BANK])
        recording_calls("scan16", models[0].scan_window_count(per, SLICE), scan_pool(pool16), scan_bank, n_banks=1, slice_samples=SLICE)
        torch.cuda.synchronize()
        pool16.close()
    del audio

    if "live" in wanted:
        S = a.streams - a.streams % TENANTS
        per_t, per_bank, n_push = S // TENANTS, S // BANK, 16
        pcm = torch.empty((S * n_push * HOP // clip + 1, clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(37, 0, pcm.shape[0], clip, pcm.data_ptr())
        sl = pool.slide_streams(S, HOP)
        sl.assign(np.arange(S), (np.arange(S) // per_t).astype(np.uint32))          # streams [k per_t, (k + 1) per_t) -> tenant k
        sessions = [bk.slide_streams(per_bank, HOP) for bk in banks]
        for ses in sessions:                                                       # stream j of a bank -> its member j / per_t
            ses.route(np.arange(per_bank), (np.uint32(1) << (np.arange(per_bank) // per_t).astype(np.uint32)).astype(np.uint32))
        sc = zeros(S, stride)
        sb = [[zeros(per_bank, m.n_labels) for m in bk.members] for bk in banks]
        streams, local = np.arange(S), np.arange(per_bank)
        state, bstate = {"step": 0, "count": 0}, {"step": 0, "count": 0}

        def packets(step):
            return (np.arange(S) * n_push + step % n_push) * HOP

        def push_pool():
            state["count"] = int(sl.push_device(pcm.data_ptr(), streams, packets(state["step"]), np.full(S, HOP), sc.data_ptr()).sum())
            state["step"] += 1

        def push_banks():
            o = packets(bstate["step"])
            bstate["count"] = sum(int(ses.push_device(pcm.data_ptr(), local, o[b * per_bank:(b + 1) * per_bank], np.full(per_bank, HOP),
                                                      [t.data_ptr() for t in sb[b]]).sum()) for b, ses in enumerate(sessions))
            bstate["step"] += 1

        def check():
            torch.cuda.synchronize()
            if state["step"] != bstate["step"] or state["count"] != S or bstate["count"] != S:
                return False
            for k, m in enumerate(models):
                b, j = divmod(k, BANK)
                if not torch.equal(bits(sc)[k * per_t:(k + 1) * per_t, :m.n_labels], bits(sb[b][j])[j * per_t:(j + 1) * per_t]):
                    return False
            return True
        for _ in range(clip // HOP + 3):                                           # up to steady state: a window per stream and push
            push_pool()
            push_banks()
        run("live", {"pool": push_pool, "banks": push_banks}, check, streams=S, tenants=TENANTS, hop_samples=HOP, path=sl.path)
        torch.cuda.synchronize()
        sl.close()
        for ses in sessions:
            ses.close()
        del pcm

    if "cepstra" in wanted:
        B = a.clips - a.clips % TENANTS
        pcm = torch.empty((B, clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(23, 0, B, clip, pcm.data_ptr())
        mfcc = torch.empty((B, models[0].n_features), dtype=torch.float32, device="cuda")
        models[0].mfcc_batch_device(pcm.data_ptr(), B, mfcc.data_ptr())
        member = (np.arange(B) % TENANTS).astype(np.uint32)
        s_cep, s_clip = zeros(B, stride), zeros(B, stride)

        def check():
            torch.cuda.synchronize()
            return torch.equal(bits(s_cep), bits(s_clip)) and bool(s_cep.any())
        run("cepstra", {"pool": lambda: pool.cmvn_inference_device(mfcc.data_ptr(), B, member, s_cep.data_ptr()),
                        "pool_clips": lambda: pool.run_classifier_device(pcm.data_ptr(), B, member, s_clip.data_ptr())}, check, rows=B, tenants=TENANTS)
        del pcm, mfcc

    torch.cuda.synchronize()
    for bk in banks:
        bk.close()
    pool.close()
    for m in models:
        m.close()
    fout.close()
    if missed:
        print("a bar is missed: " + "; ".join(missed), file=sys.stderr)
        sys.exit(1)


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    cells = {}
    for d in rows:                                               # (a later line of the same cell replaces an earlier one)
        cells.setdefault(d["workload"], {})[d["variant"]] = d
    first = rows[0]
    out = ["# Pools: recording scans, slides, live one-shot windows and the cepstra-in call", "",
           "One MI355X, KWS_MODE_EXACT kernels in every variant (pool and bank calls always run them), every variant in one process and library.  Tenants: "
           "256 synthetic int8 graphs of the stock two-block shape at 49 x 40 features, one seed each, 3 / 4 / 6 labels in turn.  Per variant: %d warm-up "
           "steps, then %d timed steps between two device events, the variants of a workload alternating, %d repeats; all repeats are listed, with their "
           "median and spread (max - min).  Before timing, the pool's rows were compared with the other variant's rows of the same (window, member) pairs: "
           "same bits.  Times are per step of the whole call or calls on the device (enqueue to last kernel), not kernel times.  The baseline of every bar "
           "is unchanged code: routed-bank calls, 16 banks of 16 members, back to back on one stream (profiles/pool_codeobj.md: the bank kernels are the "
           "parent's).  Written by tools/gpu_pool_windows_rate.py." % (first["warmup"], first["steps"], len(first["seconds_per_step"])), ""]
    what = {("scan", "pool"): "one pool scan", ("scan", "banks"): "sixteen routed-bank scans of 16 recordings each",
            ("slide", "pool"): "one pool slide", ("slide", "banks"): "sixteen routed-bank slides of 16 recordings each",
            ("live", "pool"): "one push of one pool session", ("live", "banks"): "sixteen routed-bank pushes, 16 banks of 16 members",
            ("scan16", "pool"): "one pool scan, 16 tenants", ("scan16", "bank"): "one routed-bank scan on the same 16 handles",
            ("cepstra", "pool"): "kws_pool_cmvn_inference_device on the cepstra", ("cepstra", "pool_clips"): "kws_pool_run_classifier_device on the clips"}

    def table(w):
        t = ["| variant | median ms | spread ms | every repeat, ms |", "|---|---|---|---|"]
        for v, d in cells[w].items():
            t.append("| %s | %.3f | %.3f | %s |" % (what[(w, v)], d["median_ms"], d["spread_ms"], " ".join("%.3f" % (x * 1e3) for x in d["seconds_per_step"])))
        return t + [""]

    def bar(w):
        p, b = cells[w]["pool"], cells[w]["banks"]
        met = p["median_ms"] + p["spread_ms"] < b["median_ms"]
        return ["The bar: the pool's median plus the spread between its repeats (%.3f + %.3f ms) must stay below the sixteen routed-bank calls' median "
                "(%.3f ms): %s (the sixteen calls take %.2f times the pool's median)." % (p["median_ms"], p["spread_ms"], b["median_ms"], "met" if met else "MISSED",
                                                                                       b["median_ms"] / p["median_ms"]), ""]
    for w, title in (("scan", "Bar A: recording scan"), ("slide", "Bar B: slide at a 100 ms hop")):
        if w in cells:
            d = cells[w]["pool"]
            out += ["## %s, %.2f hours of audio in %d recordings of %d samples, one per tenant (%d windows)"
                    % (title, d["recordings"] * d["samples_per_recording"] / 16000 / 3600, d["recordings"], d["samples_per_recording"], d["windows"]), ""] + table(w) + bar(w)
    if "live" in cells:
        d = cells["live"]["pool"]
        out += ["## Bar C: %d live one-shot streams of 256 tenants, one 100 ms packet per push at a 100 ms hop (path %d)" % (d["streams"], d["path"]), ""] + table("live") + bar("live")
    if "scan16" in cells:
        d = cells["scan16"]["pool"]
        out += ["## Recorded: the scan of 16 tenants (%d recordings of %d samples, %d windows) against one routed-bank scan" % (d["recordings"], d["samples_per_recording"], d["windows"]), ""]
        out += table("scan16")
    if "cepstra" in cells:
        p, c = cells["cepstra"]["pool"], cells["cepstra"]["pool_clips"]
        out += ["## Recorded: the cepstra-in call on %d rows of 256 tenants against the pool's batch call on the clips" % p["rows"], ""] + table("cepstra")
        out += ["The difference, %.3f ms of %.3f (%.0f %%), is what the batch call spends on the spectral front end; cmvnw, the upload of the items and the networks are the rest."
                % (c["median_ms"] - p["median_ms"], c["median_ms"], 100.0 * (c["median_ms"] - p["median_ms"]) / c["median_ms"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scan,slide,live,scan16,cepstra")
    ap.add_argument("--seconds", type=int, default=3600, help="audio of the scan and slide workloads, over 256 recordings")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds each workload may take")
    ap.add_argument("--tenants", default=os.path.join(ROOT, "build", "pool_tenants"), help="directory of the tenant files (written where missing)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pool_windows_rate.jsonl"))
    ap.add_argument("--md", default=None, help="write the tables from --out; runs nothing")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
