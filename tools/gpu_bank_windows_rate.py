#!/usr/bin/env python3
"""What the banks' window pipelines (kws_bank_scan_recordings_device, kws_bank_live_push_device, kws_bank_run_classifier_ragged_device;
include/kws/kws.h) save over one call per model, on one MI355X, for the four shipped 49x40 models as one bank.

Three workloads, each as the bank call beside the sum of the K members' own calls on the same inputs, in the same process and library:
  scan    one recording of --hours hours of synthetic speech-like audio in continuous mode, scores and raw scores.  Slices of --slice
          samples; by default 1 s where the stream API's rules accept that for the models' 1 s window, else the library's default of
          clip / 4 (the code a 1 s slice is refused with is recorded with the result);
  live    one push of one slice to each of --streams live streams, in steady state (every push returns one window per stream);
  ragged  --clips clips of seeded random lengths over the whole accepted range, scores only.
Every variant: --warmup untimed steps, then --steps steps between two device events; the variants of one workload alternate, --repeats
times; the median of the repeats is reported with their spread ((max - min) / median).  Before anything is timed the bank's rows are
compared with the members' own: they must be the same bits.  All KWS_MODE_EXACT (bank calls always are).
One process, one workload after the other, each under its own time limit (--limit seconds: the process ends there, starting nothing more).
One JSON line per (workload, variant), appended to --out; --md FILE writes the table from --out's lines (no GPU needed for that step).

usage: gpu_bank_windows_rate.py [--hours 1] [--streams 1024] [--clips 65536] [--steps 20] [--warmup 3] [--repeats 5] [--out FILE.jsonl]
       gpu_bank_windows_rate.py --md profiles/bank_windows_rate.md --out FILE.jsonl
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

MEMBERS = ["cfg2_mfcc40_int8", "cfg2_mfcc40_f32", "cfg5_dscnn_mfcc40_int8", "cfg5_dscnn_mfcc40_f32"]
SR = 16000


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


def same_bits(torch, a, b, rows):
    torch.cuda.synchronize()
    return all(torch.equal(x[:rows].view(torch.int32), y[:rows].view(torch.int32)) for x, y in zip(a, b))


def measure(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fout = open(a.out, "a")
    models = [pkg.Model(os.path.join(ROOT, "models", m + ".kwsm")) for m in MEMBERS]
    bank = pkg.Bank(models)
    clip = models[0].clip_samples
    try:
        models[0].scan_window_count(SR, SR)
        one_second = 0
    except pkg.KwsError as e:
        one_second = e.code
    sl = a.slice or (SR if one_second == 0 else clip // 4)

    def outs(rows):
        return [torch.zeros((rows, m.n_labels), dtype=torch.float32, device="cuda") for m in models]

    def ptrs(ts):
        return [t.data_ptr() for t in ts]

    def run(workload, rows, bank_fn, own_fn, check, **facts):
        with StepLimit(workload, a.limit):
            bank_fn()
            own_fn()
            assert check(), "%s: the bank's rows differ from the members' own" % workload
            times = {"bank": [], "own": []}
            for _ in range(a.repeats):
                times["bank"].append(timed(torch, bank_fn, a.steps, a.warmup))
                times["own"].append(timed(torch, own_fn, a.steps, a.warmup))
        for variant, ts in times.items():
            med = statistics.median(ts)
            line = json.dumps(dict(workload=workload, variant=variant, members=MEMBERS, rows=rows, steps=a.steps, warmup=a.warmup, seconds_per_step=ts,
                                   median_ms=med * 1e3, spread=(max(ts) - min(ts)) / med, same_bits=True, slice_samples=sl, one_second_slice_rc=one_second, **facts))
            print(line, flush=True)
            fout.write(line + "\n")
            fout.flush()

    # ---- scan: one recording
    n = a.hours * 3600 * SR
    n_clips = (n + clip - 1) // clip
    pcm = torch.empty((n_clips, clip), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(17, 0, n_clips, clip, pcm.data_ptr())
    W = models[0].scan_window_count(n, sl)
    sb, rb, so, ro = outs(W), outs(W), outs(W), outs(W)

    def scan_bank():
        bank.scan_recordings_device(pcm.data_ptr(), [0], [n], ptrs(sb), ptrs(rb), slice_samples=sl)

    def scan_own():
        for m, s, r in zip(models, so, ro):
            m.scan_recordings_device(pcm.data_ptr(), [0], [n], s.data_ptr(), r.data_ptr(), slice_samples=sl)
    run("scan", W, scan_bank, scan_own, lambda: same_bits(torch, sb + rb, so + ro, W), audio_hours=a.hours)
    del sb, rb, so, ro

    # ---- live: one slice to every stream, in steady state
    S = a.streams
    lv, own = bank.live_streams(S, sl), [m.live_streams(S, sl) for m in models]
    streams, offs, lens = np.arange(S), np.arange(S) * sl, np.full(S, sl)
    sb, so = outs(S), outs(S)
    counts = {}

    def live_bank():
        counts["bank"] = int(lv.push_device(pcm.data_ptr(), streams, offs, lens, ptrs(sb)).sum())

    def live_own():
        counts["own"] = sum(int(o.push_device(pcm.data_ptr(), streams, offs, lens, s.data_ptr()).sum()) for o, s in zip(own, so))
    for _ in range(clip // sl + 3):                                   # up to steady state: a window per stream and push
        live_bank()
        live_own()
    run("live", S, live_bank, live_own, lambda: same_bits(torch, sb, so, S) and counts == {"bank": S, "own": S * len(models)}, streams=S)
    lv.close()
    for o in own:
        o.close()
    del sb, so, pcm

    # ---- ragged: clips of their own lengths
    B = a.clips
    lo = next(k for k in range(1, clip) if models[0].window_frame_count(k) >= 1)
    pcm = torch.empty((B, clip), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(19, 0, B, clip, pcm.data_ptr())
    lens = np.random.default_rng(5).integers(lo, clip + 1, B)
    offs = np.arange(B) * clip
    sb, so = outs(B), outs(B)

    def ragged_bank():
        bank.run_classifier_ragged_device(pcm.data_ptr(), offs, lens, ptrs(sb))

    def ragged_own():
        for m, s in zip(models, so):
            m.run_classifier_ragged_device(pcm.data_ptr(), offs, lens, s.data_ptr())
    run("ragged", B, ragged_bank, ragged_own, lambda: same_bits(torch, sb, so, B), shortest=int(lo), longest=int(clip))
    torch.cuda.synchronize()
    bank.close()
    for m in models:
        m.close()
    fout.close()


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    cells = {}
    for d in rows:
        cells.setdefault(d["workload"], {})[d["variant"]] = d
    first = rows[0]
    out = ["# Banks over scans, live streams and ragged clips: one call for K models, against one call per model", "",
           "One MI355X, the four shipped 49x40 models (%s) as one bank, KWS_MODE_EXACT kernels on both sides (bank calls always run them).  `own` is "
           "the sum of the members' own calls on the same inputs, issued back to back in the same process and library: the route a caller had before, "
           "so it is the baseline.  Per variant: %d warm-up steps, then %d timed steps between two device events, the two variants alternating; median "
           "of %d repeats, spread = (max - min) / median.  Before timing, the bank's rows were compared with the members' own at the timed size: same "
           "bits.  Written by tools/gpu_bank_windows_rate.py." % (", ".join(first["members"]), first["warmup"], first["steps"], len(first["seconds_per_step"])), "",
           "| workload | rows per step | bank ms | own ms (sum of %d) | own / bank | largest spread |" % len(first["members"]), "|---|---|---|---|---|---|"]
    names = {"scan": lambda d: "scan, one recording of %g h of audio, 1 s windows in slices of %d samples, scores and raw scores" % (d["audio_hours"], d["slice_samples"]),
             "live": lambda d: "live push, one slice of %d samples to each of %d streams (steady state: one window per stream)" % (d["slice_samples"], d["streams"]),
             "ragged": lambda d: "ragged batch, clips of %d .. %d samples (seeded uniform), scores only" % (d["shortest"], d["longest"])}
    for w in ("scan", "live", "ragged"):
        if w not in cells:
            out.append("| %s | not measured | | | | |" % w)
            continue
        b, o = cells[w]["bank"], cells[w]["own"]
        out.append("| %s | %d | %.3f | %.3f | %.2f | %.1f %% |" % (names[w](b), b["rows"], b["median_ms"], o["median_ms"], o["median_ms"] / b["median_ms"],
                                                              100 * max(b["spread"], o["spread"])))
    if first.get("one_second_slice_rc"):
        out += ["", "A slice of one second is the models' whole window: kws_scan_window_count refuses it (code %d, the stream API's rule on frames per slice), "
                "so the continuous workloads run at the library's default slicing, four slices per window." % first["one_second_slice_rc"]]
    out += ["", "Times are per step of the whole call on the device (enqueue to last kernel), not kernel times; no kernel trace was taken."]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--slice", type=int, default=0, help="slice samples of the continuous workloads (default: clip / 4)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds each workload may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "bank_windows_rate.jsonl"))
    ap.add_argument("--md", default=None, help="write the table from --out; runs nothing")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
