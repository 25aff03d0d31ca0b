#!/usr/bin/env python3
"""Throughput of kws_slide_recordings_device (one-shot windows of whole recordings at a hop) on one MI355X.

Workload: --recordings recordings (default 1 024) x 60 s of synthetic speech-like audio, per model, mode (exact, fast) and hop
(stride, 5 stride, 4000, 8000, clip): windows/s of the SHARED path, the DIRECT path and AUTO, and of the route a user has without the call
-- the windows gathered on the device into [B][clip] pieces (a strided copy) and kws_run_classifier_batch_device on each piece; existing
API only.  Every figure is a host clock around a warmed-up call that ends in a device synchronise; the variants of one (model, mode, hop)
alternate, --repeats times each (default 3), and the spread of the repeats is kept ((max - min) / median).
Prints one JSON line per (model, mode, hop, variant) (also appended to --out FILE) and, with --md FILE, writes the table.

usage: gpu_slide_rate.py [--models l476_no_yes,cfg2_mfcc40_f32] [--recordings 1024] [--repeats 3] [--out FILE.jsonl] [--md FILE.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 32768            # windows per piece of the baseline: 1 GiB of gathered clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="l476_no_yes,cfg2_mfcc40_f32")
    ap.add_argument("--recordings", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="exact,fast")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--md", default=None, help="write the table to this file")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    sr, n_rec = 16000, a.recordings
    n60 = 60 * sr
    audio = torch.empty((n_rec, n60), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(17, 0, n_rec * 60, sr, audio.data_ptr())
    torch.cuda.synchronize()
    offs = [i * n60 for i in range(n_rec)]
    lens = [n60] * n_rec
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")
    rows = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")
        rows.append(d)

    def once(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for name in a.models.split(","):
        gm = pkg.Model(os.path.join(ROOT, "models", name + ".kwsm"))
        C, clip, stride = gm.n_labels, gm.clip_samples, gm.frame_stride_samples
        gathered = torch.empty((PIECE, clip), dtype=torch.int16, device="cuda")
        for mode_name in a.modes.split(","):
            gm.set_mode(pkg.MODE_FAST if mode_name == "fast" else pkg.MODE_EXACT)
            for hop in (stride, 5 * stride, 4000, 8000, clip):
                plan = gm.slide_plan(lens, hop)
                W = plan["n_windows"]
                s = torch.empty((W, C), dtype=torch.float32, device="cuda")
                view = audio.unfold(1, clip, hop)                 # [recordings][windows per recording][clip], a view
                per = view.shape[1]

                def baseline():
                    # pieces of whole recordings' windows: a strided device copy, then the batch call
                    step = max(1, PIECE // per)
                    for r0 in range(0, n_rec, step):
                        v = view[r0:r0 + step]
                        n = v.shape[0] * per
                        g = gathered[:n].view(v.shape[0], per, clip)
                        g.copy_(v)
                        gm.run_classifier_batch_device(gathered.data_ptr(), n, s[r0 * per:].data_ptr())

                variants = {
                    "shared": lambda: gm.slide_recordings_device(audio.data_ptr(), offs, lens, hop, s.data_ptr(), flags=pkg.SLIDE_SHARED),
                    "direct": lambda: gm.slide_recordings_device(audio.data_ptr(), offs, lens, hop, s.data_ptr(), flags=pkg.SLIDE_DIRECT),
                    "auto": lambda: gm.slide_recordings_device(audio.data_ptr(), offs, lens, hop, s.data_ptr(), flags=pkg.SLIDE_AUTO),
                    "baseline": baseline,
                }
                times = {k: [] for k in variants}
                for fn in variants.values():                      # warm-up: code objects, scratch growth
                    once(fn)
                for _ in range(a.repeats):
                    for k, fn in variants.items():
                        times[k].append(once(fn))
                for k, ts in times.items():
                    med = statistics.median(ts)
                    emit(dict(model=name, mode=mode_name, hop=hop, variant=k, windows=W, seconds=ts, windows_per_s=W / med,
                              spread=(max(ts) - min(ts)) / med, auto_path="shared" if plan["path"] == pkg.SLIDE_SHARED else "direct",
                              rows_shared=plan["rows_shared"], rows_first=plan["rows_first"], rows_direct=plan["rows_direct"], phases=plan["phases"]))
                del s
        del gathered
        gm.close()
        torch.cuda.empty_cache()
    if fout:
        fout.close()
    if a.md:
        write_md(a.md, rows, n_rec, a.repeats)


def write_md(path, rows, n_rec, repeats):
    key = lambda d: (d["model"], d["mode"], d["hop"])
    cells = {}
    for d in rows:
        cells.setdefault(key(d), {})[d["variant"]] = d
    out = ["# kws_slide_recordings_device: windows/s on one MI355X", "",
           "%d recordings x 60 s, scores only; median of %d alternating repeats after a warm-up call each, host clock around a device "
           "synchronise; spread = (max - min) / median of the repeats.  Baseline: the windows gathered on the device into [B][clip] pieces "
           "and kws_run_classifier_batch_device (existing API only).  Written by tools/gpu_slide_rate.py." % (n_rec, repeats), "",
           "| model | mode | hop | windows | rows shared + first / direct | shared | direct | auto (path) | baseline | shared / baseline | largest spread |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for k in sorted(cells):
        c = cells[k]
        any_ = next(iter(c.values()))
        r = lambda v: "%.3g M/s" % (c[v]["windows_per_s"] / 1e6)
        out.append("| %s | %s | %d | %d | %.3f | %s | %s | %s (%s) | %s | %.2f | %.1f %% |" % (
            k[0], k[1], k[2], any_["windows"], (any_["rows_shared"] + any_["rows_first"]) / max(any_["rows_direct"], 1), r("shared"), r("direct"),
            r("auto"), any_["auto_path"], r("baseline"), c["shared"]["windows_per_s"] / c["baseline"]["windows_per_s"],
            100 * max(v["spread"] for v in c.values())))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
