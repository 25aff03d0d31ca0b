#!/usr/bin/env python3
"""Throughput of kws_scan_recordings_device (continuous mode over whole recordings) on one MI355X.

Cases, per model and mode:
  (a) 1 024 recordings x 60 s in one scan call;
  (b) one 1-hour recording in one scan call;
  the same 1 024 recordings stepped through kws_streams_step_device in lock step (S = 1 024, 240 steps) for comparison,
  and the one-shot batch path (kws_run_classifier_batch_device, 65 536 clips) for the clips/s the scan's windows/s is set against.
Rates come from a device synchronise around a warmed-up timed loop.  Prints one JSON line per case (also appended to --out FILE when given).

usage: gpu_scan_rate.py [--models l476_no_yes,cfg2_mfcc40_f32] [--iters 3] [--out FILE.jsonl] [--no-streams]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="l476_no_yes,cfg2_mfcc40_f32")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-streams", action="store_true")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    sr, slice_n = 16000, 4000
    n60, n_rec = 60 * sr, 1024
    # synthetic speech-like audio generated on the device: 1 024 x 60 s, and one hour
    audio = torch.empty((n_rec, n60), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(17, 0, n_rec * 60, sr, audio.data_ptr())
    hour = torch.empty(3600 * sr, dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(18, 0, 3600, sr, hour.data_ptr())
    clips = torch.empty((65536, sr), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(19, 0, 65536, sr, clips.data_ptr())
    torch.cuda.synchronize()
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
        for mode_name, mode in (("exact", pkg.MODE_EXACT), ("fast", pkg.MODE_FAST)):
            gm.set_mode(mode)
            # (a) 1 024 x 60 s
            offs = [i * n60 for i in range(n_rec)]
            lens = [n60] * n_rec
            W = sum(gm.scan_window_count(n) for n in lens)
            s = torch.empty((W, C), dtype=torch.float32, device="cuda")
            dt = timed(lambda: gm.scan_recordings_device(audio.data_ptr(), offs, lens, s.data_ptr()), a.iters)
            emit(dict(case="a_scan", model=name, mode=mode_name, recordings=n_rec, windows=W, seconds=dt, windows_per_s=W / dt,
                      audio_s_per_s=n_rec * 60 / dt))
            # (b) one hour
            Wh = gm.scan_window_count(hour.numel())
            sh = torch.empty((Wh, C), dtype=torch.float32, device="cuda")
            dt = timed(lambda: gm.scan_recordings_device(hour.data_ptr(), [0], [hour.numel()], sh.data_ptr()), a.iters)
            emit(dict(case="b_scan_1h", model=name, mode=mode_name, recordings=1, windows=Wh, seconds=dt, windows_per_s=Wh / dt,
                      audio_s_per_s=3600 / dt))
            # the one-shot batch path on the same model
            sc = torch.empty((65536, C), dtype=torch.float32, device="cuda")
            dt = timed(lambda: gm.run_classifier_batch_device(clips.data_ptr(), 65536, sc.data_ptr()), a.iters)
            emit(dict(case="batch_clips", model=name, mode=mode_name, clips=65536, seconds=dt, clips_per_s=65536 / dt))
            # (a) through the stream API in lock step
            if not a.no_streams:
                steps = n60 // slice_n
                sl = audio.view(n_rec, steps, slice_n).transpose(0, 1).contiguous()       # [steps][S][slice]
                sb = pkg.StreamBatch(gm, n_rec)
                ss = torch.empty((n_rec, C), dtype=torch.float32, device="cuda")

                def run_streams():
                    sb.init()
                    for k in range(steps):
                        sb.step_device(sl[k].data_ptr(), slice_n, ss.data_ptr())
                dt = timed(run_streams, 1)
                emit(dict(case="a_streams_lockstep", model=name, mode=mode_name, recordings=n_rec, windows=W, seconds=dt,
                          windows_per_s=W / dt, audio_s_per_s=n_rec * 60 / dt))
                sb.close()
                del sl
                torch.cuda.empty_cache()
        gm.close()
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
