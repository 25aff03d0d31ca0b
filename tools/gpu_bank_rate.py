#!/usr/bin/env python3
"""What a bank (kws_bank_*: K models behind one DSP block, include/kws/kws.h) saves over one call per model, on one MI355X.

Timed, at --clips resident clips (default 65 536) of synthetic speech-like audio, scores only:
  * the four shipped 49x40 models: one kws_bank_run_classifier_batch_device call against the four members' own
    kws_run_classifier_batch_device calls in KWS_MODE_EXACT (the path a caller had before banks; their sum is the baseline);
  * the same for the l476 pair (int8 + float32 twin);
  * both banks over --minutes minutes of audio (default 10) at hop 1600: kws_bank_slide_recordings_device against the members' own
    kws_slide_recordings_device calls.
Every variant: --warmup untimed steps, then --steps timed steps between device synchronisations (bench.py's pattern, host clock); the
variants of one workload alternate, --repeats times, and the spread of the repeats is kept ((max - min) / median).  Before anything is
timed the bank's scores are compared with the members' own at the timed size: they must be the same bits.
One JSON line per (workload, variant), also appended to --out.

Launch counts come from runs of their own under the profiler (tracing slows the host; nothing timed above is traced):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/gpu_bank_rate.py --leg bank:mfcc40 --calls 4
runs only that leg, --calls calls and nothing else.  Legs: bank:<b>, own:<b>, slidebank:<b>, slideown:<b>; b = mfcc40 or l476.

--md FILE writes the table from --out's lines and the kernel_stats.csv files named with --stats LEG=FILE (no GPU needed for this step).

usage: gpu_bank_rate.py [--clips 65536] [--minutes 10] [--steps 40] [--warmup 3] [--repeats 3] [--out FILE.jsonl]
       gpu_bank_rate.py --leg bank:mfcc40 [--calls 4]
       gpu_bank_rate.py --md profiles/bank_rate.md --out FILE.jsonl [--stats bank:mfcc40=FILE.csv ...] [--calls 4]
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

BANKS = {
    "mfcc40": ["cfg2_mfcc40_int8", "cfg2_mfcc40_f32", "cfg5_dscnn_mfcc40_int8", "cfg5_dscnn_mfcc40_f32"],
    "l476": ["l476_no_yes", "l476_no_yes_f32"],
}
HOP = 1600
SR = 16000


class Workload:
    """one bank, its members, the resident audio and the output buffers; bank() / own() run one step of each route"""

    def __init__(self, pkg, torch, name, clips, minutes):
        self.pkg, self.torch, self.name = pkg, torch, name
        self.models = [pkg.Model(os.path.join(ROOT, "models", m + ".kwsm")) for m in BANKS[name]]
        self.bank = pkg.Bank(self.models)
        self.B = clips
        clip = self.models[0].clip_samples
        self.pcm = torch.empty((max(clips, minutes * 60), clip), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(17, 0, self.pcm.shape[0], clip, self.pcm.data_ptr())
        self.rec_len = minutes * 60 * SR
        self.W = self.models[0].slide_window_count(self.rec_len, HOP)
        rows = max(clips, self.W)
        self.s_bank = [torch.zeros((rows, m.n_labels), dtype=torch.float32, device="cuda") for m in self.models]
        self.s_own = [torch.zeros((rows, m.n_labels), dtype=torch.float32, device="cuda") for m in self.models]
        torch.cuda.synchronize()

    def run_bank(self):
        self.bank.run_classifier_batch_device(self.pcm.data_ptr(), self.B, [t.data_ptr() for t in self.s_bank])

    def run_own(self):
        for m, t in zip(self.models, self.s_own):
            m.run_classifier_batch_device(self.pcm.data_ptr(), self.B, t.data_ptr())

    def slide_bank(self):
        self.bank.slide_recordings_device(self.pcm.data_ptr(), [0], [self.rec_len], HOP, [t.data_ptr() for t in self.s_bank])

    def slide_own(self):
        for m, t in zip(self.models, self.s_own):
            m.slide_recordings_device(self.pcm.data_ptr(), [0], [self.rec_len], HOP, t.data_ptr())

    def same_bits(self, rows):
        self.torch.cuda.synchronize()
        return all(self.torch.equal(a[:rows].view(self.torch.int32), b[:rows].view(self.torch.int32)) for a, b in zip(self.s_bank, self.s_own))

    def close(self):
        self.bank.close()
        for m in self.models:
            m.close()


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

    for name in BANKS:
        w = Workload(pkg, torch, name, a.clips, a.minutes)
        for kind, bank_fn, own_fn, rows in (("batch", w.run_bank, w.run_own, w.B), ("slide", w.slide_bank, w.slide_own, w.W)):
            bank_fn()
            own_fn()
            assert w.same_bits(rows), "%s %s: the bank's scores differ from the members' own" % (name, kind)
            times = {"bank": [], "own": []}
            for _ in range(a.repeats):
                times["bank"].append(timed(torch, bank_fn, a.steps, a.warmup))
                times["own"].append(timed(torch, own_fn, a.steps, a.warmup))
            for variant, ts in times.items():
                med = statistics.median(ts)
                emit(dict(bank=name, members=BANKS[name], workload=kind, variant=variant, rows=rows, steps=a.steps, warmup=a.warmup,
                          seconds_per_step=ts, median_ms=med * 1e3, spread=(max(ts) - min(ts)) / med, same_bits=True,
                          audio_minutes=a.minutes if kind == "slide" else None, hop=HOP if kind == "slide" else None))
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
    w = Workload(pkg, torch, name, a.clips, a.minutes)
    fn = {"bank": w.run_bank, "own": w.run_own, "slidebank": w.slide_bank, "slideown": w.slide_own}[kind]
    for _ in range(a.calls):
        fn()
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
        cells.setdefault((d["bank"], d["workload"]), {})[d["variant"]] = d
    out = ["# Banks: one call for K models behind one DSP block, against one call per model", "",
           "One MI355X, scores only, KWS_MODE_EXACT kernels on both sides (bank calls always run them).  `own` is the sum of the members' own calls, "
           "issued back to back in the same process and library: the route a caller had before banks, so it is the baseline.  Per variant: "
           "warm-up steps, then timed steps between device synchronisations (host clock), the two variants alternating; median of the repeats, "
           "spread = (max - min) / median.  Before timing, the bank's scores were compared with the members' own at the timed size: same bits.  "
           "Written by tools/gpu_bank_rate.py.", "",
           "| bank | members | workload | rows | bank ms | own ms (sum) | own / bank | largest spread |", "|---|---|---|---|---|---|---|---|"]
    below = []
    for (bank, kind), c in sorted(cells.items()):
        b, o = c["bank"], c["own"]
        what = "%d clips" % b["rows"] if kind == "batch" else "slide, %d min of audio at hop %d" % (b["audio_minutes"], b["hop"])
        ratio = o["median_ms"] / b["median_ms"]
        if ratio < 1:
            below.append((bank, kind, ratio))
        out.append("| %s | %d | %s | %d | %.3f | %.3f | %.2f | %.1f %% |" % (bank, len(b["members"]), what, b["rows"], b["median_ms"], o["median_ms"], ratio,
                                                                         100 * max(b["spread"], o["spread"])))
    out += ["", "Steps per timing: %d timed after %d warm-up, %d repeats." % (rows[0]["steps"], rows[0]["warmup"], len(rows[0]["seconds_per_step"]))]
    if below:
        out += ["", "Ratios below 1: " + ", ".join("%s %s (%.2f)" % x for x in below) + " -- see the traces below."]
    if a.stats:
        out += ["", "The traced legs below create their models too: the few launches that do not scale with the calls (the spectral kernel without "
                "cmvnw, from kws_create's gain calibration of a float32 graph) belong to that, not to a call."]
    for spec in a.stats or []:
        legname, path = spec.split("=", 1)
        st = read_stats(path)
        out += ["", "## Launches: `%s`, %d calls under `rocprofv3 --kernel-trace --stats` (a run of its own)" % (legname, a.calls), "",
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
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (with --md: read them from it)")
    ap.add_argument("--leg", default=None, help="run only this leg, --calls times (for a profiler run): bank|own|slidebank|slideown:mfcc40|l476")
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--md", default=None, help="write the table from --out and --stats; runs nothing")
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
