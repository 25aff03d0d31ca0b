#!/usr/bin/env python3
"""Throughput of kws_slide_live_push_device (live streams of one-shot windows) on one MI355X.

Workload: --streams streams (default 1 024) x --seconds s (default 60) of synthetic speech-like audio, pushed in lock step in packets of
--packets ms (default 20 and 250), per model, mode (exact, fast) and hop (stride, 5 stride, 4000, clip): windows/s of a SHARED session
(where the hop is served), a DIRECT session and an AUTO session, against
  slide     one kws_slide_recordings_device call over the same audio -- the ceiling: nothing is cut into pushes;
  baseline  the route a user has without the feature: per push, the windows it completes gathered on the device into [B][clip] clips (a
            strided copy out of the audio the user keeps) and kws_run_classifier_batch_device on them; existing API only.
Every figure is a host clock around a warmed-up run (a fresh session, every push of the audio) that ends in a device synchronise; the
variants of one (model, mode, hop, packet) alternate, --repeats times each (default 3), and the spread of the repeats is kept
((max - min) / median).  Prints one JSON line per (model, mode, hop, packet, variant) (also appended to --out FILE) and, with --md FILE,
writes the table.

usage: gpu_slide_live_rate.py [--models l476_no_yes,cfg2_mfcc40_f32] [--streams 1024] [--seconds 60] [--packets 20,250] [--repeats 3]
                              [--modes exact,fast] [--hops s,5s,4000,c] [--out FILE.jsonl] [--md FILE.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="l476_no_yes,cfg2_mfcc40_f32")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--packets", default="20,250", help="packet lengths in ms")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="exact,fast")
    ap.add_argument("--hops", default="s,5s,4000,c", help="s = the frame stride, c = the clip")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--md", default=None, help="write the table to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    sr, S = 16000, a.streams
    n_all = a.seconds * sr
    audio = torch.empty((S, n_all), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(17, 0, S * a.seconds, sr, audio.data_ptr())
    torch.cuda.synchronize()
    base = np.arange(S, dtype=np.uint64) * np.uint64(n_all)
    streams = np.arange(S, dtype=np.uint64)
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
        C, clip, stride, nf = gm.n_labels, gm.clip_samples, gm.frame_stride_samples, gm.n_frames
        for mode_name in a.modes.split(","):
            gm.set_mode(pkg.MODE_FAST if mode_name == "fast" else pkg.MODE_EXACT)
            for hop_name in a.hops.split(","):
                hop = {"s": stride, "5s": 5 * stride, "c": clip}.get(hop_name) or int(hop_name)
                per = gm.slide_window_count(n_all, hop)             # windows per stream
                W = per * S
                served = hop % stride == 0 and hop // stride <= nf - 1
                view = audio.unfold(1, clip, hop)                   # [streams][windows per stream][clip], a view
                s_all = torch.empty((W, C), dtype=torch.float32, device="cuda")
                for ms in (int(x) for x in a.packets.split(",")):
                    packet = sr * ms // 1000
                    most = (packet + hop - 1) // hop + 1            # windows one push can complete per stream
                    s_push = torch.empty((S * most, C), dtype=torch.float32, device="cuda")
                    gathered = torch.empty((S * most, clip), dtype=torch.int16, device="cuda")
                    lens = np.full(S, packet, np.uint64)

                    def live(flags):
                        def run():
                            sess = gm.slide_streams(S, hop, flags)
                            for pos in range(0, n_all - packet + 1, packet):
                                sess.push_device(audio.data_ptr(), streams, base + np.uint64(pos), lens, s_push.data_ptr())
                            torch.cuda.synchronize()
                            sess.close()
                        return run

                    def baseline():
                        w0 = 0
                        for pos in range(0, n_all - packet + 1, packet):
                            n1 = pos + packet
                            w1 = 0 if n1 < clip else (n1 - clip) // hop + 1
                            if w1 > w0:
                                n = S * (w1 - w0)
                                gathered[:n].view(S, w1 - w0, clip).copy_(view[:, w0:w1])
                                gm.run_classifier_batch_device(gathered.data_ptr(), n, s_push.data_ptr())
                            w0 = w1

                    variants = {"direct": live(pkg.SLIDE_DIRECT), "auto": live(pkg.SLIDE_AUTO), "baseline": baseline,
                                "slide": lambda: gm.slide_recordings_device(audio.data_ptr(), base, np.full(S, n_all, np.uint64), hop, s_all.data_ptr())}
                    if served:
                        variants["shared"] = live(pkg.SLIDE_SHARED)
                    sess = gm.slide_streams(S, hop, pkg.SLIDE_AUTO)
                    auto_path = "shared" if sess.path == pkg.SLIDE_SHARED else "direct"
                    sess.close()
                    times = {k: [] for k in variants}
                    for fn in variants.values():                    # warm-up: code objects, scratch growth
                        once(fn)
                    for _ in range(a.repeats):
                        for k, fn in variants.items():
                            times[k].append(once(fn))
                    n_push = (n_all - packet) // packet + 1
                    w_pushed = gm.slide_window_count(n_push * packet, hop) * S
                    for k, ts in times.items():
                        med = statistics.median(ts)
                        w = W if k == "slide" else w_pushed
                        emit(dict(model=name, mode=mode_name, hop=hop, packet_ms=ms, variant=k, streams=S, seconds=a.seconds, windows=w, pushes=n_push,
                                  times=ts, windows_per_s=w / med, ms_per_push=None if k == "slide" else 1e3 * med / n_push,
                                  spread=(max(ts) - min(ts)) / med, auto_path=auto_path))
                    del s_push, gathered
                del s_all
        gm.close()
        torch.cuda.empty_cache()
    if fout:
        fout.close()
    if a.md:
        write_md(a.md, rows, a)


def write_md(path, rows, a):
    cells = {}
    for d in rows:
        cells.setdefault((d["model"], d["mode"], d["hop"], d["packet_ms"]), {})[d["variant"]] = d
    out = ["# kws_slide_live_push_device: windows/s on one MI355X", "",
           "%d streams x %d s pushed in lock step, scores only; median of %d alternating repeats after a warm-up run each, host clock around "
           "a whole run (a fresh session, every push) that ends in a device synchronise; spread = (max - min) / median of the repeats.  slide: "
           "one kws_slide_recordings_device call over the same audio (the ceiling).  baseline: per push, the completed windows gathered on the "
           "device into [B][clip] clips and kws_run_classifier_batch_device (existing API only).  Written by tools/gpu_slide_live_rate.py."
           % (a.streams, a.seconds, a.repeats), "",
           "| model | mode | hop | packet | windows | shared | direct | auto (path) | baseline | slide | best live / baseline | ms per push (auto) | largest spread |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for k in sorted(cells):
        c = cells[k]
        any_ = c["auto"]
        r = lambda v: "%.3g M/s" % (c[v]["windows_per_s"] / 1e6) if v in c else "not served"      # noqa: E731
        best = max(c[v]["windows_per_s"] for v in ("shared", "direct", "auto") if v in c)
        out.append("| %s | %s | %d | %d ms | %d | %s | %s | %s (%s) | %s | %s | %.2f | %.3f | %.1f %% |" % (
            k[0], k[1], k[2], k[3], any_["windows"], r("shared"), r("direct"), r("auto"), any_["auto_path"], r("baseline"), r("slide"),
            best / c["baseline"]["windows_per_s"], any_["ms_per_push"], 100 * max(v["spread"] for v in c.values())))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
