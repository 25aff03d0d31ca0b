#!/usr/bin/env python3
"""Throughput of kws_live_push_device (live streams in continuous mode) on one MI355X.

Cases, per model and mode, all on 1 024 streams x 60 s of synthetic speech-like audio resident on the device (the pushes read it in place):
  (1) 250 ms packets to every stream (240 pushes; the last one finishes every stream) -- the stream API's own shape, so the lock-step
      kws_streams_step_device loop (S = 1 024, 240 steps) runs alongside as the comparison;
  (2) 20 ms packets to every stream (3 000 pushes);
  (3) seeded ragged packets of 10 - 500 ms, each push to a random half of the streams that still have audio;
  and kws_scan_recordings_device on the same audio in one call: the upper bound (no state, no push boundaries).
Each live run starts from kws_live_reset of every stream.  Rates come from a device synchronise around a warmed-up timed run.  Prints one
JSON line per case (also appended to --out FILE when given).

usage: gpu_live_rate.py [--models l476_no_yes,cfg2_mfcc40_f32] [--iters 2] [--out FILE.jsonl] [--no-streams] [--cases 1,2,3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def schedule_uniform(n_streams, n, pk):
    """pushes of pk samples to every stream, the last one finishing: [(streams, offsets, lengths, finish)]"""
    st = np.arange(n_streams, dtype=np.uint64)
    out = []
    for t in range(n // pk):
        out.append((st, st * np.uint64(n) + np.uint64(t * pk), np.full(n_streams, pk, np.uint64),
                    np.full(n_streams, int(t == n // pk - 1), np.int32)))
    return out


def schedule_ragged(n_streams, n, seed, lo=160, hi=8000):
    """seeded packets of lo..hi samples, each push to a random half of the streams with audio left; a stream's last packet finishes it"""
    rng = np.random.default_rng(seed)
    pos = np.zeros(n_streams, np.int64)
    out = []
    while (pos < n).any():
        live = np.nonzero(pos < n)[0]
        pick = live[rng.random(live.size) < 0.5]
        if pick.size == 0:
            continue
        ln = np.minimum(rng.integers(lo, hi + 1, pick.size), n - pos[pick])
        fin = (pos[pick] + ln == n).astype(np.int32)
        out.append((pick.astype(np.uint64), (pick * n + pos[pick]).astype(np.uint64), ln.astype(np.uint64), fin))
        pos[pick] += ln
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="l476_no_yes,cfg2_mfcc40_f32")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-streams", action="store_true")
    ap.add_argument("--cases", default="1,2,3")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    sr, slice_n = 16000, 4000
    n60, S = 60 * sr, 1024
    audio = torch.empty((S, n60), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(17, 0, S * 60, sr, audio.data_ptr())
    torch.cuda.synchronize()
    cases = [c for c in a.cases.split(",") if c]
    plans = {"1": ("live_250ms", schedule_uniform(S, n60, 4000)), "2": ("live_20ms", schedule_uniform(S, n60, 320)),
             "3": ("live_ragged_10_500ms", schedule_ragged(S, n60, 5))}
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / iters

    for name in a.models.split(","):
        gm = pkg.Model(os.path.join(ROOT, "models", name + ".kwsm"))
        C = gm.n_labels
        W = S * gm.scan_window_count(n60)
        for mode_name, mode in (("exact", pkg.MODE_EXACT), ("fast", pkg.MODE_FAST)):
            gm.set_mode(mode)
            s = torch.empty((W, C), dtype=torch.float32, device="cuda")
            offs = [i * n60 for i in range(S)]
            dt = timed(lambda: gm.scan_recordings_device(audio.data_ptr(), offs, [n60] * S, s.data_ptr()), a.iters)
            emit(dict(case="scan", model=name, mode=mode_name, streams=S, windows=W, seconds=dt, windows_per_s=W / dt))
            del s
            lv = gm.live_streams(S, slice_n)
            out = torch.empty((4 * S, C), dtype=torch.float32, device="cuda")
            for c in cases:
                label, plan = plans[c]
                got = [0]

                def run():
                    lv.reset()
                    total = 0
                    for st, off, ln, fin in plan:
                        total += int(lv.push_device(audio.data_ptr(), st, off, ln, out.data_ptr(), finish=fin).sum())
                    got[0] = total
                dt = timed(run, a.iters)
                assert got[0] == W, (label, got[0], W)
                emit(dict(case=label, model=name, mode=mode_name, streams=S, pushes=len(plan), windows=W, seconds=dt, windows_per_s=W / dt,
                          ms_per_push=1e3 * dt / len(plan)))
            lv.close()
            del out
            if not a.no_streams and "1" in cases:
                steps = n60 // slice_n
                sl = audio.view(S, steps, slice_n).transpose(0, 1).contiguous()       # [steps][S][slice]
                sb = pkg.StreamBatch(gm, S)
                ss = torch.empty((S, C), dtype=torch.float32, device="cuda")

                def run_streams():
                    sb.init()
                    for k in range(steps):
                        sb.step_device(sl[k].data_ptr(), slice_n, ss.data_ptr())
                dt = timed(run_streams, 1)
                Wl = S * (steps - 3)
                emit(dict(case="streams_lockstep_250ms", model=name, mode=mode_name, streams=S, pushes=steps, windows=Wl, seconds=dt,
                          windows_per_s=Wl / dt, ms_per_push=1e3 * dt / steps))
                sb.close()
                del sl
            torch.cuda.empty_cache()
        gm.close()
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
