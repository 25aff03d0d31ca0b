#!/usr/bin/env python3
"""What residual graphs cost, on one MI355X, KWS_MODE_EXACT: the network launch alone at --clips resident clips (default 65 536).

Three graphs, each as the int8 graph and as its float32 twin (tools/dequantize_model.py):
  tc_res8        three stride-2 projection blocks, 16 -> 24 -> 32 -> 48 channels, 9-tap filters (tests/residual_testlib.py RES_SPECS): 13 steps --
                 kws_nnres_trunk_kernel + kws_dense_i8_kernel / kws_nnres_f32_trunk_kernel + kws_dense_f32_kernel, the code under test
  res2d_proj_s2  a 2-D projection block on 49 x 13 x 1, the same kernels
  tc_chain       the YARDSTICK: tc_res8 with its ADDs and shortcuts removed -- a strided chain of the 1-D family (kws_nn_sd_kernel /
                 kws_nn_f32_sd_kernel, served before this work); the same main-path convolutions, no 1 x 1 shortcuts, no ADDs.  A twin the library
                 refuses (its filters exceed the 1-D float kernel's LDS budget) is reported as refused, with the message.
Each graph's multiply-accumulate count per clip is printed next to its time.

Timed with device events on resident int8 tensors / feature matrices of standardised random values, every handle warmed up first, the handles of a
precision alternating inside each of --repeats rounds in this one command, --steps launches per figure.  Per figure: median of the rounds and spread =
(max - min) / median.  No rate is promised: there is no parent implementation to compare with.  One JSON line per handle, also appended to --out.
--md FILE writes the table from --out's lines (no GPU needed).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRAPHS = ("tc_res8", "res2d_proj_s2", "tc_chain")
TC_CHAIN = dict(seed=903, blocks=((16, 3, 1), (24, 9, 1), (24, 9, 1), (32, 9, 1), (32, 9, 1), (48, 9, 1), (48, 9, 1)), conv_stride={1: 2, 3: 2, 5: 2},
                logit_std=1.5)


def graph_blob(name, is_float):
    import dequantize_model
    import residual_testlib as T
    import synth_model
    if name == "tc_chain":
        blob = synth_model.synth_model_blob(**TC_CHAIN)
        return dequantize_model.dequantize(blob) if is_float else blob
    return T.res_twin(name) if is_float else T.res_blob(name)


def macs_per_clip(blob):
    """multiply-accumulates of one clip: every CONV_2D / FULLY_CONNECTED output x its filter's operands (padding taps included)"""
    import eon_import
    tens, nodes, _, _, _ = eon_import.parse_blob(blob)
    n = 0
    for nd in nodes:
        if nd["op"] in (1, 4):
            w, y = tens[nd["in"][1]]["dims"], tens[nd["out"][0]]["dims"]
            out = 1
            for d in y:
                out *= d
            n += out * (w[-1] if nd["op"] == 4 else w[1] * w[2] * w[3])
    return n


class Handle:
    def __init__(self, pkg, torch, name, is_float, clips):
        self.torch, self.name, self.is_float, self.B = torch, name, is_float, clips
        blob = graph_blob(name, is_float)
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

    def close(self):
        self.m.close()


def timed(torch, fn, steps):
    """device-event milliseconds per step"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


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
    for is_float in (False, True):
        hs = {}
        for name in GRAPHS:
            try:
                hs[name] = Handle(pkg, torch, name, is_float, a.clips)
            except pkg.KwsError as e:
                emit(dict(graph=name, precision="f32" if is_float else "int8", refused=str(e), clips=a.clips, steps=a.steps, warmup=a.warmup))
        for h in hs.values():
            for _ in range(a.warmup):
                h.net()
        torch.cuda.synchronize()
        t = {name: [] for name in hs}
        for _ in range(a.repeats):
            for name, h in hs.items():
                t[name].append(timed(torch, h.net, a.steps))
        for name, h in hs.items():
            med = statistics.median(t[name])
            emit(dict(graph=name, precision="f32" if is_float else "int8", kernel=h.m.nn_kernel, macs_per_clip=h.macs, clips=a.clips, steps=a.steps,
                      warmup=a.warmup, net_ms=t[name], net_median_ms=med, net_spread=(max(t[name]) - min(t[name])) / med))
            h.close()
        del hs
        torch.cuda.empty_cache()
    if fout:
        fout.close()


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    r0 = [d for d in rows if "net_ms" in d][0]
    out = ["# residual graphs: time per %d resident clips" % r0["clips"], "",
           "One MI355X, KWS_MODE_EXACT, %d resident clips.  Device-event time of the network launch alone; every handle warmed up (%d launches), then %d "
           "timed launches per figure, the handles of a precision alternating inside each of %d rounds of one command; median of the rounds, spread = "
           "(max - min) / median.  `tc_res8` and `res2d_proj_s2` are residual graphs (the code under test); `tc_chain` is `tc_res8` without its ADDs and "
           "shortcuts, a strided chain of the 1-D family served before this work: a yardstick of the main path's cost on the older kernels, not a baseline of "
           "the same arithmetic.  No rate was promised for this work and there is no parent implementation to compare with; nothing else was measured.  "
           "Written by tools/gpu_residual_rate.py." % (r0["clips"], r0["warmup"], r0["steps"], len(r0["net_ms"])), "",
           "| graph | precision | kernel | MAC / clip | net ms | net spread | G MAC / s |", "|---|---|---|---|---|---|---|"]
    for d in rows:
        if "refused" in d:
            out.append("| %s | %s | refused: %s | | | | |" % (d["graph"], d["precision"], d["refused"]))
            continue
        out.append("| %s | %s | `%s` | %d | %.3f | %.1f %% | %.0f |" % (
            d["graph"], d["precision"], d["kernel"], d["macs_per_clip"], d["net_median_ms"], 100 * d["net_spread"],
            d["macs_per_clip"] * d["clips"] / d["net_median_ms"] / 1e6))
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
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (with --md: read them from it)")
    ap.add_argument("--md", default=None, help="write the table from --out; runs nothing")
    ap.add_argument("--note", default=None, help="with --md: a text file appended under the table")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
