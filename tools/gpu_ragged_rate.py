#!/usr/bin/env python3
"""What clips of their own lengths cost (kws_run_classifier_ragged_device, include/kws/kws.h), on one MI355X, scores only.

Timed, at --clips resident clips (default 65 536) of synthetic speech-like audio, for l476_no_yes and cfg2_mfcc40_f32:
  (a) uniform   every clip kws_clip_samples long on a 16-byte boundary: the ragged call against kws_run_classifier_batch_device in
                KWS_MODE_EXACT on the same buffer.  The batch call's launches are untouched by the ragged work, so it is the baseline.
                Requirement: ragged <= 1.10 x batch (what differs per clip is one descriptor read and a pad map taken from a table; per call
                the upload of 16 bytes per clip and the host loop over the lengths).
  (b) mixed     the same number of clips with lengths uniform over the valid range (seeded), each on a 16-byte boundary of the same
                buffer (one every kws_clip_samples: the longest overlap their neighbour): ms per call, clips/s and frames/s.  No bar: it records what per-clip frame counts cost.
Every variant: --warmup untimed steps, then --steps timed steps between device synchronisations (host clock); the variants alternate,
--repeats times; median and spread ((max - min) / median) of the repeats.  Before anything is timed the ragged call's scores on (a) are
compared with the batch call's: they must be the same bits.  One JSON line per (model, variant), also appended to --out.

Launch counts come from a run of its own under the profiler (tracing slows the host; nothing timed above is traced):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/gpu_ragged_rate.py --leg mixed:l476_no_yes --calls 4
runs only that leg, --calls calls and nothing else.  Legs: mixed:<model>, uniform:<model>, batch:<model>.

--md FILE writes the tables from --out's lines and the kernel_stats.csv files named with --stats LEG=FILE (no GPU needed for this step).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = ["l476_no_yes", "cfg2_mfcc40_f32"]
REQUIREMENT = 1.10


class Workload:
    def __init__(self, pkg, torch, name, clips):
        import numpy as np
        self.pkg, self.torch, self.name, self.B = pkg, torch, name, clips
        self.m = m = pkg.Model(os.path.join(ROOT, "models", name + ".kwsm"))
        clip = m.clip_samples
        self.pcm = torch.empty((clips + 1, clip), dtype=torch.int16, device="cuda")      # (+ 1: the longest clips reach into the next slot)
        pkg.synth_clips_device(17, 0, clips + 1, clip, self.pcm.data_ptr())
        self.s_batch = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.s_ragged = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.offsets = np.arange(clips, dtype=np.uint64) * clip          # clip is a multiple of 8 samples: every clip on a 16-byte boundary
        self.len_uniform = np.full(clips, clip, np.uint64)
        lo = next(n for n in range(clip) if m.window_frame_count(n) >= 1)
        hi = clip
        while m.window_frame_count(hi + 1) == m.n_frames:
            hi += 1
        # lengths uniform over the valid range (the shipped impulse: 640 .. 16 319); clips may overlap, and the longest do
        self.len_mixed = np.random.default_rng(65536).integers(lo, hi + 1, clips).astype(np.uint64)
        stride = self.m.L.kws_frame_stride_samples(m.h)
        flen = lo - stride
        self.frames_uniform = clips * m.n_frames
        self.frames_mixed = int(((self.len_mixed.astype(np.int64) - flen) // stride).sum())
        assert all(m.window_frame_count(int(n)) == (int(n) - flen) // stride for n in self.len_mixed[:64])
        torch.cuda.synchronize()

    def batch(self):
        self.m.run_classifier_batch_device(self.pcm.data_ptr(), self.B, self.s_batch.data_ptr())

    def uniform(self):
        self.m.run_classifier_ragged_device(self.pcm.data_ptr(), self.offsets, self.len_uniform, self.s_ragged.data_ptr())

    def mixed(self):
        self.m.run_classifier_ragged_device(self.pcm.data_ptr(), self.offsets, self.len_mixed, self.s_ragged.data_ptr())

    def same_bits(self):
        self.torch.cuda.synchronize()
        return self.torch.equal(self.s_batch.view(self.torch.int32), self.s_ragged.view(self.torch.int32))

    def close(self):
        self.m.close()


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def measure(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")

    for name in MODELS:
        w = Workload(pkg, torch, name, a.clips)
        w.batch()
        w.uniform()
        assert w.same_bits(), "%s: the ragged call's scores on full-length clips differ from the batch call's" % name
        times = {"batch": [], "uniform": [], "mixed": []}
        for _ in range(a.repeats):
            for variant in times:
                times[variant].append(timed(torch, getattr(w, variant), a.steps, a.warmup))
        for variant, ts in times.items():
            med = statistics.median(ts)
            frames = w.frames_mixed if variant == "mixed" else w.frames_uniform
            emit(dict(model=name, variant=variant, clips=w.B, frames=frames, steps=a.steps, warmup=a.warmup, seconds_per_step=ts, median_ms=med * 1e3,
                      spread=(max(ts) - min(ts)) / med, clips_per_s=w.B / med, frames_per_s=frames / med, same_bits=True))
        w.close()
        del w
        torch.cuda.empty_cache()
    if fout:
        fout.close()


def leg(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    kind, name = a.leg.split(":")
    w = Workload(pkg, torch, name, a.clips)
    for _ in range(a.calls):
        getattr(w, kind)()
    torch.cuda.synchronize()
    w.close()


def read_stats(path):
    """[(kernel, calls, total us)] of a rocprofv3 kernel_stats.csv, the library's kernels only"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "kws_" not in name or "kws_synth_kernel" in name:          # (the leg's audio: set-up, not a call)
                continue
            rows.append((name, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3))
    return sorted(rows, key=lambda x: -x[2])


def short(name):
    name = name.replace("void ", "")
    return name[:name.index("(")] if "(" in name else name


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    cells = {}
    for d in rows:
        cells.setdefault(d["model"], {})[d["variant"]] = d
    out = ["# Clips of their own lengths: kws_run_classifier_ragged_device against the fixed-length batch call", "",
           "One MI355X, scores only, the exact kernels on both sides (the ragged call always runs them; the batch call in KWS_MODE_EXACT, whose launches "
           "this work does not touch: it is the baseline).  Per variant: warm-up steps, then timed steps between device synchronisations (host clock), "
           "the variants alternating; median of the repeats, spread = (max - min) / median.  Before timing, the ragged call's scores on full-length "
           "clips were compared with the batch call's: same bits.  Written by tools/gpu_ragged_rate.py.", "",
           "## (a) Full-length uniform batch: every clip kws_clip_samples long, on a 16-byte boundary", "",
           "| model | clips | batch ms | ragged ms | ragged / batch | requirement | met | largest spread |", "|---|---|---|---|---|---|---|---|"]
    missed = []
    for model, c in sorted(cells.items()):
        b, u = c["batch"], c["uniform"]
        ratio = u["median_ms"] / b["median_ms"]
        if ratio > REQUIREMENT:
            missed.append((model, ratio))
        out.append("| %s | %d | %.3f | %.3f | %.3f | <= %.2f | %s | %.1f %% |" % (model, b["clips"], b["median_ms"], u["median_ms"], ratio, REQUIREMENT,
                                                                                "yes" if ratio <= REQUIREMENT else "NO", 100 * max(b["spread"], u["spread"])))
    out += ["", ("Requirement NOT met for: " + ", ".join("%s (%.3f)" % x for x in missed) + ".") if missed else
            "The requirement (ragged <= %.2f x batch) is met for both models." % REQUIREMENT]
    out += ["", "## (b) Mixed batch: lengths uniform over the valid range (seeded), every clip on a 16-byte boundary", "",
            "| model | clips | frames | ms per call | clips/s | frames/s | (a) ragged frames/s | (a) batch frames/s | spread |", "|---|---|---|---|---|---|---|---|---|"]
    for model, c in sorted(cells.items()):
        x = c["mixed"]
        out.append("| %s | %d | %d | %.3f | %.3g | %.3g | %.3g | %.3g | %.1f %% |" % (model, x["clips"], x["frames"], x["median_ms"], x["clips_per_s"], x["frames_per_s"],
                                                                                    c["uniform"]["frames_per_s"], c["batch"]["frames_per_s"], 100 * x["spread"]))
    out += ["", "No bar on (b): it records what per-clip frame counts cost.  A wave owns a clip whatever its length, so a short clip leaves its wave's "
            "per-clip work (the lane constants, the DCT and cmvnw set-up, the network) spread over fewer frames.",
            "", "Steps per timing: %d timed after %d warm-up, %d repeats." % (rows[0]["steps"], rows[0]["warmup"], len(rows[0]["seconds_per_step"]))]
    if a.stats:
        out += ["", "The traced legs below create their models too: the few launches that do not scale with the calls (the spectral kernel without "
                "cmvnw, from kws_create's gain calibration of a float32 graph) belong to that, not to a call."]
    for spec in a.stats or []:
        legname, path = spec.split("=", 1)
        st = read_stats(path)
        out += ["", "## (c) Launches: `%s`, %d calls under `rocprofv3 --kernel-trace --stats` (a run of its own)" % (legname, a.calls), "",
                "| kernel | launches | per call | total us | us per call |", "|---|---|---|---|---|"]
        for name, calls, us in st:
            out.append("| `%s` | %d | %.4g | %.1f | %.1f |" % (short(name)[:90], calls, calls / a.calls, us, us / a.calls))
        out.append("| all | %d | %.4g | %.1f | %.1f |" % (sum(x[1] for x in st), sum(x[1] for x in st) / a.calls, sum(x[2] for x in st),
                                                      sum(x[2] for x in st) / a.calls))
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (with --md: read them from it)")
    ap.add_argument("--leg", default=None, help="run only this leg, --calls times (for a profiler run): mixed|uniform|batch:<model>")
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--md", default=None, help="write the tables from --out and --stats; runs nothing")
    ap.add_argument("--stats", action="append", help="LEG=kernel_stats.csv of a profiler run of that leg")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    elif a.leg:
        leg(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
