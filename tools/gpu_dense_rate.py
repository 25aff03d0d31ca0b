#!/usr/bin/env python3
"""Time of the dense-stack kernels at 65 536 resident clips, written to profiles/dense_rate.md: for d0_h20_h10, c2_h64, d0_m40_h128
(tests/dense_testlib.py) and their float twins the network-only launch (int8: kws_nn_batch_device without taps; float32: kws_nn_f32_batch_device)
and the whole exact batch call (kws_run_classifier_batch_device, scores only).  Next to each network time: the time the launch's unavoidable
bytes (input tensor + scores, + the trunk's hand-off written and read once where there is one) take at 8 000 GB/s, and -- same run, same box --
the shipped network's launch (kws_nn_mfma_kernel on l476_no_yes, kws_nn_f32_kernel on its twin), which is the parent's kernel and not under test.
Device events around ITERS launches per sample (tens of milliseconds each); three rounds that alternate over all models; median and spread (max - min) / median.

usage: gpu_dense_rate.py [out.md]         (needs the GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B, ROUNDS = 65536, 3
ITERS = {"nn": 200, "call": 20}          # launches per sample: every sample covers tens of milliseconds (0.07 - 2.7 ms / 2 - 6 ms each)
HBM_GBS = 8000.0


def main():
    import torch
    from __graft_entry__ import load_package
    import dense_testlib as D
    pkg = load_package()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dense_rate.md")
    models = []
    for name in ("d0_h20_h10", "c2_h64", "d0_m40_h128"):
        models.append((name, pkg.Model(blob=D.dense_blob(name)), D.dense_blob(name)))
        models.append((name + " f32", pkg.Model(blob=D.dense_twin(name)), D.dense_blob(name)))
    models.append(("l476_no_yes (shipped)", pkg.Model(os.path.join(ROOT, "models", "l476_no_yes.kwsm")), None))
    models.append(("l476_no_yes_f32 (shipped)", pkg.Model(os.path.join(ROOT, "models", "l476_no_yes_f32.kwsm")), None))
    pcm = torch.randint(-20000, 20000, (B, 16000), dtype=torch.int16, device="cuda")
    bufs = {}
    for name, m, _ in models:
        x = (torch.randn((B, m.n_features), dtype=torch.float32, device="cuda") if m.is_float
             else torch.randint(-128, 128, (B, m.n_features), dtype=torch.int8, device="cuda"))
        bufs[name] = (x, torch.empty((B, m.n_labels), dtype=torch.float32, device="cuda"))

    def nn(name, m):
        x, s = bufs[name]
        if m.is_float:
            m.nn_f32_batch_device(x.data_ptr(), B, s.data_ptr())
        else:
            m.nn_batch_device(x.data_ptr(), B, s.data_ptr())

    def call(name, m):
        m.run_classifier_batch_device(pcm.data_ptr(), B, bufs[name][1].data_ptr())

    def sample(fn, name, m):
        n = ITERS["nn" if fn is nn else "call"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn(name, m)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for name, m, _ in models:                                # warm-up: code objects, scratch growth
        for _ in range(2):
            nn(name, m)
            call(name, m)
    torch.cuda.synchronize()
    t_nn = {name: [] for name, _, _ in models}
    t_call = {name: [] for name, _, _ in models}
    for _ in range(ROUNDS):
        for name, m, _ in models:
            t_nn[name].append(sample(nn, name, m))
        for name, m, _ in models:
            t_call[name].append(sample(call, name, m))

    def stat(v):
        med = float(np.median(v))
        return med, (max(v) - min(v)) / med

    lines = ["# dense stacks at %d resident clips (tools/gpu_dense_rate.py)" % B, "",
             "Median of %d alternating rounds of %d network launches / %d batch calls each (device events); spread = (max - min) / median.  Floor: the bytes the network launch"
             % (ROUNDS, ITERS["nn"], ITERS["call"]),
             "must move (input tensor + scores, + the trunk's hand-off written and read once) / %d GB/s." % int(HBM_GBS), "",
             "| model | kernel | network only ms | spread | floor ms | x floor | batch call ms | spread |", "|---|---|---|---|---|---|---|---|"]
    for name, m, blob in models:
        elem = 4 if m.is_float else 1
        nbytes = B * (m.n_features * elem + m.n_labels * 4)
        if blob is not None:
            tens, nodes, hidden, last, _, _ = D.graph_layout(blob)
            first_fc = [nd for nd in nodes if nd["op"] == 4][0]
            k0 = tens[first_fc["in"][1]]["dims"][1]
            if any(nd["op"] in (1, 6) for nd in nodes):
                nbytes += 2 * B * k0 * elem
        floor = nbytes / (HBM_GBS * 1e9) * 1e3
        a, sa = stat(t_nn[name])
        c, sc = stat(t_call[name])
        lines.append("| %s | %s | %.4f | %.1f %% | %.4f | %.1f | %.3f | %.1f %% |" % (name, m.nn_kernel, a, 100 * sa, floor, a / floor, c, 100 * sc))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "w") as f:
        f.write(text)
    for _, m, _ in models:
        m.close()


if __name__ == "__main__":
    main()
