#!/usr/bin/env python3
"""What the 2-D convolutional classifier costs, on one MI355X, KWS_MODE_EXACT, --clips resident clips (default 65 536) of synthetic
speech-like audio.

Two graphs, each as the int8 graph and as its float32 twin (tools/dequantize_model.py):
  ei_2d    the stock 2-D graph on 49 x 13 features (tests/conv2d_testlib.py CONV2D_SPECS): 8 ch 3 x 3, pool 2 x 2, 16 ch 3 x 3, pool 2 x 2, Dense(4) --
           kws_nn2d_trunk_kernel + kws_dense_i8_kernel / kws_nn2d_f32_trunk_kernel + kws_dense_f32_kernel, the code under test
  l476     the shipped 1-D impulse (models/l476_no_yes.kwsm and its float twin), the YARDSTICK beside it: another graph on the same features, served before
           this work -- not a baseline of the same arithmetic.  Each graph's multiply-accumulate count per clip is printed next to its time.

Timed with device events, every handle warmed up first, the handles alternating inside each of --repeats rounds in this one command:
  net    the network launch alone (kws_nn_batch_device / kws_nn_f32_batch_device on the resident int8 tensors / feature matrices), --steps launches
  call   the whole batch call from PCM (kws_run_classifier_batch_device), --steps calls
Per figure: median of the rounds and spread = (max - min) / median.  No rate is promised: there is no parent implementation to compare with.  One JSON line
per handle, also appended to --out.  --md FILE writes the table from --out's lines (no GPU needed).
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

GRAPHS = ("ei_2d", "l476")


def graph_blob(name, is_float):
    import conv2d_testlib as T
    import dequantize_model
    if name == "ei_2d":
        return T.conv2d_twin(name) if is_float else T.conv2d_blob(name)
    blob = open(os.path.join(ROOT, "models", "l476_no_yes.kwsm"), "rb").read()
    return dequantize_model.dequantize(blob) if is_float else blob


def macs_per_clip(blob):
    """multiply-accumulates of one clip: every CONV_2D / DEPTHWISE_CONV_2D / FULLY_CONNECTED output x its filter's operands (padding taps included)"""
    import eon_import
    tens, nodes, _, _, _ = eon_import.parse_blob(blob)
    n = 0
    for nd in nodes:
        if nd["op"] in (1, 4, 6):
            w, y = tens[nd["in"][1]]["dims"], tens[nd["out"][0]]["dims"]
            out = 1
            for d in y:
                out *= d
            per = w[-1] if nd["op"] == 4 else w[1] * w[2] * (1 if nd["op"] == 6 else w[3])
            n += out * per
    return n


class Handle:
    def __init__(self, pkg, torch, name, is_float, clips):
        self.torch, self.name, self.is_float, self.B = torch, name, is_float, clips
        blob = graph_blob(name, is_float)
        self.macs = macs_per_clip(blob)
        self.m = m = pkg.Model(blob=blob)
        self.pcm = torch.empty((clips, m.clip_samples), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(17, 0, clips, m.clip_samples, self.pcm.data_ptr())
        self.s = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.s_net = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.f = torch.empty((clips, m.n_features), dtype=torch.float32, device="cuda")
        self.q = torch.empty((clips, m.n_features), dtype=torch.int8, device="cuda")
        m.run_classifier_batch_device(self.pcm.data_ptr(), clips, self.s.data_ptr(), self.f.data_ptr(), None if is_float else self.q.data_ptr())
        self.net()
        torch.cuda.synchronize()
        # the network launch alone reproduces the call's scores (same bits: same kernels on the same inputs)
        assert torch.equal(self.s.view(torch.int32), self.s_net.view(torch.int32)), name

    def net(self):
        if self.is_float:
            self.m.nn_f32_batch_device(self.f.data_ptr(), self.B, self.s_net.data_ptr(), None)
        else:
            self.m.nn_batch_device(self.q.data_ptr(), self.B, self.s_net.data_ptr())

    def call(self):
        self.m.run_classifier_batch_device(self.pcm.data_ptr(), self.B, self.s.data_ptr())

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
    for is_float in (False, True):
        hs = {name: Handle(pkg, torch, name, is_float, a.clips) for name in GRAPHS}
        for h in hs.values():
            for _ in range(a.warmup):
                h.net()
                h.call()
        torch.cuda.synchronize()
        t = {name: {"net": [], "call": []} for name in hs}
        for _ in range(a.repeats):
            for name, h in hs.items():
                t[name]["net"].append(timed(torch, h.net, a.steps))
                t[name]["call"].append(timed(torch, h.call, a.steps))
        for name, h in hs.items():
            d = dict(graph=name, precision="f32" if is_float else "int8", kernel=h.m.nn_kernel, macs_per_clip=h.macs, clips=a.clips, steps=a.steps,
                     warmup=a.warmup)
            for k in ("net", "call"):
                med = statistics.median(t[name][k])
                d[k + "_ms"] = t[name][k]
                d[k + "_median_ms"] = med
                d[k + "_spread"] = (max(t[name][k]) - min(t[name][k])) / med
            line = json.dumps(d)
            print(line, flush=True)
            if fout:
                fout.write(line + "\n")
            h.close()
        del hs
        torch.cuda.empty_cache()
    if fout:
        fout.close()


def write_md(a):
    rows = [json.loads(ln) for ln in open(a.out) if ln.strip()]
    r0 = rows[0]
    out = ["# 2-D convolutional classifier: time per %d resident clips" % r0["clips"], "",
           "One MI355X, KWS_MODE_EXACT, %d resident clips.  Device-event time of the network launch alone (`net`) and of the whole batch call from PCM "
           "(`call`); every handle warmed up (%d launches and calls), then %d timed steps per figure, the handles of a precision alternating inside each of "
           "%d rounds of one command; median of the rounds, spread = (max - min) / median.  `ei_2d` is the stock 2-D graph on 49 x 13 features (the code "
           "under test); `l476` is the shipped 1-D impulse on the same features, a yardstick of another graph's cost, not a baseline of the same arithmetic.  "
           "No rate was promised for this work and there is no parent implementation to compare with.  Written by tools/gpu_conv2d_rate.py."
           % (r0["clips"], r0["warmup"], r0["steps"], len(r0["net_ms"])), "",
           "| graph | precision | kernel | MAC / clip | net ms | net spread | G MAC / s (net) | call ms | call spread |", "|---|---|---|---|---|---|---|---|---|"]
    for d in rows:
        out.append("| %s | %s | `%s` | %d | %.3f | %.1f %% | %.0f | %.3f | %.1f %% |" % (
            d["graph"], d["precision"], d["kernel"], d["macs_per_clip"], d["net_median_ms"], 100 * d["net_spread"],
            d["macs_per_clip"] * d["clips"] / d["net_median_ms"] / 1e6, d["call_median_ms"], 100 * d["call_spread"]))
    if a.note:
        out += ["", open(a.note).read().rstrip()]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
