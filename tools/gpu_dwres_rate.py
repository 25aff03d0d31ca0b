#!/usr/bin/env python3
"""What depthwise steps on the step trunks cost, on one MI355X, KWS_MODE_EXACT: the network launch alone at --clips resident clips
(default 65 536).

Two graphs of tests/dwres_testlib.py DW_SPECS, each as the int8 graph and as its float32 twin (tools/dequantize_model.py), each beside its
FULL-CONVOLUTION twin (dwres_testlib.conv_twin_spec: every DEPTHWISE_CONV_2D replaced by a CONV_2D of the same filter size, stride and padding over all
input channels -- graphs the library served before this work):
  mnv2_ir      a 2-D inverted residual, 8 -> 24 -> depthwise 3 x 3 -> 8 channels with an identity skip; its twin runs on the same step trunk
  ds2d_plain   a 2-D depthwise-separable graph without an ADD; its twin is a CONV_2D + MAX_POOL_2D chain of the 2-D family (kws_nn2d_*_trunk_kernel)
Each graph's multiply-accumulate count per clip is printed next to its time.

Timed with device events on resident int8 tensors / feature matrices of standardised random values, both handles warmed up first and alternating inside
each of --repeats rounds, at least --steps launches and --window-ms of device time per figure.  Per figure: median of the rounds and spread = (max - min) / median; per pair the ratio of the
medians.  Every (graph, precision) pair is a child process of its own under `timeout`; the first one that fails ends the run.  Nothing is built here: the
library must have been built (__graft_entry__.build(), at most 16 jobs).  No rate is promised: there is no parent implementation to compare with.  One
JSON line per handle, also appended to --out.  --md FILE writes the table from --out's lines (no GPU needed).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRAPHS = ("mnv2_ir", "ds2d_plain")
STEP_TIMEOUT_S = 240


def graph_blob(name, full_conv, is_float):
    import dequantize_model
    import dwres_testlib as T
    import synth_model
    blob = synth_model.synth_model_blob(**T.conv_twin_spec(name)) if full_conv else T.dw_blob(name)
    return dequantize_model.dequantize(blob) if is_float else blob


def macs_per_clip(blob):
    """multiply-accumulates of one clip: every CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED output x its filter's operands per output (padding taps
    included)"""
    import eon_import
    tens, nodes, _, _, _ = eon_import.parse_blob(blob)
    n = 0
    for nd in nodes:
        if nd["op"] in (1, 4, 6):
            w, y = tens[nd["in"][1]]["dims"], tens[nd["out"][0]]["dims"]
            out = 1
            for d in y:
                out *= d
            n += out * (w[-1] if nd["op"] == 4 else w[1] * w[2] if nd["op"] == 6 else w[1] * w[2] * w[3])
    return n


class Handle:
    def __init__(self, pkg, torch, name, full_conv, is_float, clips):
        self.torch, self.name, self.full_conv, self.is_float, self.B = torch, name, full_conv, is_float, clips
        blob = graph_blob(name, full_conv, is_float)
        self.macs = macs_per_clip(blob)
        self.m = m = pkg.Model(blob=blob)
        g = torch.Generator(device="cuda").manual_seed(17)
        self.f = torch.randn((clips, m.n_features), generator=g, dtype=torch.float32, device="cuda")
        self.q = torch.clamp(torch.round(self.f * 16.0), -128, 127).to(torch.int8)
        self.s = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")

    def net(self):
        if self.is_float:
            self.m.nn_f32_batch_device(self.f.data_ptr(), self.B, self.s.data_ptr(), None)
        else:
            self.m.nn_batch_device(self.q.data_ptr(), self.B, self.s.data_ptr())


def timed(torch, fn, steps):
    """device-event milliseconds per step"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def worker(a):
    """one (graph, precision) pair: the depthwise graph and its full-convolution twin"""
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from __graft_entry__ import load_package
    pkg = load_package()
    is_float = a.precision == "f32"
    hs = [Handle(pkg, torch, a.worker, full_conv, is_float, a.clips) for full_conv in (False, True)]
    for h in hs:
        for _ in range(a.warmup):
            h.net()
    torch.cuda.synchronize()
    # launches per figure: at least --steps, and enough for --window-ms of device time (a window of a few milliseconds measures the clock and the scheduler)
    steps = [max(a.steps, int(a.window_ms / timed(torch, h.net, a.steps)) + 1) for h in hs]
    t = [[], []]
    for _ in range(a.repeats):
        for k, h in enumerate(hs):
            t[k].append(timed(torch, h.net, steps[k]))
    med = [statistics.median(v) for v in t]
    lines = []
    for k, h in enumerate(hs):
        lines.append(json.dumps(dict(graph=a.worker, form="full_conv" if h.full_conv else "depthwise", precision=a.precision, kernel=h.m.nn_kernel,
                                     depthwise_steps=h.m.depthwise_step_count, macs_per_clip=h.macs, clips=a.clips, steps=steps[k], warmup=a.warmup, net_ms=t[k],
                                     net_median_ms=med[k], net_spread=(max(t[k]) - min(t[k])) / med[k], ratio_to_full_conv=med[0] / med[1])))
        h.m.close()
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def measure(a):
    for name in GRAPHS:
        for precision in ("int8", "f32"):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--worker", name, "--precision", precision,
                   "--clips", str(a.clips), "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--window-ms", str(a.window_ms)] + (["--out", a.out] if a.out else [])
            rc = subprocess.call(cmd)
            if rc != 0:
                sys.exit("%s %s ended with status %d: nothing more is started" % (name, precision, rc))


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    r0 = rows[0]
    out = ["# depthwise steps on the step trunks: time per %d resident clips" % r0["clips"], "",
           "One MI355X, KWS_MODE_EXACT, %d resident clips.  Device-event time of the network launch alone; both handles of a pair warmed up (%d launches), then "
           "at least %d timed launches and 0.3 s of device time per figure (the steps column), the two handles alternating inside each of %d rounds of one "
           "process; median of the rounds, spread = (max - min) / median.  `depthwise` is the graph of tests/dwres_testlib.py (the code under test); `full_conv` is the same graph with every depthwise step "
           "replaced by a CONV_2D of the same filter size over all input channels, which the library served before this work.  ratio = depthwise median / "
           "full_conv median of the same pair.  No rate was promised for this work and there is no parent implementation to compare with; nothing else was "
           "measured.  Written by tools/gpu_dwres_rate.py." % (r0["clips"], r0["warmup"], min(d["steps"] for d in rows), len(r0["net_ms"])), "",
           "| graph | form | precision | kernel | MAC / clip | steps | net ms | net spread | M clips / s | ratio |", "|---|---|---|---|---|---|---|---|---|---|"]
    for d in rows:
        out.append("| %s | %s | %s | `%s` | %d | %d | %.3f | %.1f %% | %.2f | %s |" % (
            d["graph"], d["form"], d["precision"], d["kernel"], d["macs_per_clip"], d["steps"], d["net_median_ms"], 100 * d["net_spread"],
            d["clips"] / d["net_median_ms"] / 1e3, "%.2f" % d["ratio_to_full_conv"] if d["form"] == "depthwise" else ""))
    if a.note:
        out += ["", open(a.note).read().rstrip()]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0, help="device time a figure spans at least (the launches per figure follow from it)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (with --md: read them from it)")
    ap.add_argument("--md", default=None, help="write the table from --out; runs nothing")
    ap.add_argument("--note", default=None, help="with --md: a text file appended under the table")
    ap.add_argument("--worker", default=None, help="(internal) measure this graph's pair in this process")
    ap.add_argument("--precision", default="int8", choices=("int8", "f32"))
    a = ap.parse_args()
    if a.md:
        write_md(a)
    elif a.worker:
        worker(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
