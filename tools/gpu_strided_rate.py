#!/usr/bin/env python3
"""What a strided first block costs, on one MI355X, KWS_MODE_EXACT, --clips resident clips (default 65 536) of synthetic speech-like audio.

Four graphs, each as the int8 graph and as its float32 twin (tools/dequantize_model.py):
  g13_s2   49 x 13 features, blocks (30 ch, 7 taps, pool 7) (10 ch, 7 taps, pool 3), the first block at stride 2 (49 -> 25 rows)
  g13_s1   the same blocks at stride 1: its twin, served before this work -- the BASELINE, not the code under test
  g40_s2   49 x 40 features (the cfg2 DSP block), the same blocks, first block at stride 2
  g40_s1   its stride-1 twin
(the shipped graphs' SAME pools of 7 do not divide 25 rows without padding, which no kernel here serves: both forms pool VALID, 7 then 3.)
A stride-1 form runs kws_nn_kernel / kws_nn_f32_kernel, its stride-2 form kws_nn_sd_kernel / kws_nn_f32_sd_kernel (labels: the SD instantiations of the same
templates).

Timed with device events, every handle warmed up first, the handles alternating inside each of --repeats rounds in this one command:
  net    the network launch alone (kws_nn_batch_device / kws_nn_f32_batch_device on the resident int8 tensors / feature matrices), --steps launches
  call   the whole batch call from PCM (kws_run_classifier_batch_device), --steps calls
Per figure: median of the rounds and spread = (max - min) / median.  The condition: a stride-2 graph computes half the outputs of its first block and
everything behind it on half the rows, so its network launch must not take longer than its stride-1 twin's; the only allowance is the larger of the two
spreads measured here.  One JSON line per handle, also appended to --out.  --md FILE writes the tables from --out's lines (no GPU needed); --bench
"LABEL=json line" adds bench.py result lines (this commit's and the parent's, same call) to show that the headline did not move.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BLOCKS = ((30, 7, -7), (10, 7, -3))
GRAPHS = {
    "g13_s2": dict(seed=801, blocks=BLOCKS, conv_stride={0: 2}, logit_std=1.5),
    "g13_s1": dict(seed=801, blocks=BLOCKS, logit_std=1.5),
    "g40_s2": dict(seed=802, num_filters=40, ncep=40, low=300, high=0, blocks=BLOCKS, conv_stride={0: 2}, logit_std=1.5),
    "g40_s1": dict(seed=802, num_filters=40, ncep=40, low=300, high=0, blocks=BLOCKS, logit_std=1.5),
}
PAIRS = (("g13_s2", "g13_s1"), ("g40_s2", "g40_s1"))


class Handle:
    def __init__(self, pkg, torch, name, is_float, clips):
        import dequantize_model
        import synth_model
        self.pkg, self.torch, self.name, self.is_float, self.B = pkg, torch, name, is_float, clips
        blob = synth_model.synth_model_blob(**GRAPHS[name])
        self.m = m = pkg.Model(blob=dequantize_model.dequantize(blob) if is_float else blob)
        self.pcm = torch.empty((clips, m.clip_samples), dtype=torch.int16, device="cuda")
        pkg.synth_clips_device(17, 0, clips, m.clip_samples, self.pcm.data_ptr())
        self.s = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.s_net = torch.zeros((clips, m.n_labels), dtype=torch.float32, device="cuda")
        self.f = torch.empty((clips, m.n_features), dtype=torch.float32, device="cuda")
        self.q = torch.empty((clips, m.n_features), dtype=torch.int8, device="cuda")
        m.run_classifier_batch_device(self.pcm.data_ptr(), clips, self.s.data_ptr(), self.f.data_ptr(), None if is_float else self.q.data_ptr())
        self.net()
        torch.cuda.synchronize()
        # the network launch alone reproduces the call's scores (same bits: same kernel on the same inputs)
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
            d = dict(graph=name, precision="f32" if is_float else "int8", kernel=h.m.nn_kernel, clips=a.clips, steps=a.steps, warmup=a.warmup)
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
    cell = {(d["graph"], d["precision"]): d for d in rows}
    r0 = rows[0]
    out = ["# Strided first blocks: the network launch of a stride-2 graph against its stride-1 twin", "",
           "One MI355X, KWS_MODE_EXACT, %d resident clips.  Device-event time of the network launch alone (`net`) and of the whole batch call from PCM "
           "(`call`); every handle warmed up (%d launches and calls), then %d timed steps per figure, the four handles of a precision alternating inside each of "
           "%d rounds of one command; median of the rounds, spread = (max - min) / median.  The stride-1 twin (the same blocks at stride 1, served before "
           "this work) is the baseline, not the code under test.  Graphs: 49 x 13 and 49 x 40 features, blocks (30 ch, 7 taps, VALID pool 7) (10 ch, 7 taps, "
           "VALID pool 3), first block at stride 2 or 1.  Written by tools/gpu_strided_rate.py." % (r0["clips"], r0["warmup"], r0["steps"], len(r0["net_ms"])), "",
           "| graph | precision | kernel | net ms | net spread | call ms | call spread |", "|---|---|---|---|---|---|---|"]
    for d in rows:
        out.append("| %s | %s | `%s` | %.3f | %.1f %% | %.3f | %.1f %% |" % (d["graph"], d["precision"], d["kernel"], d["net_median_ms"], 100 * d["net_spread"],
                                                                            d["call_median_ms"], 100 * d["call_spread"]))
    out += ["", "## The condition: net(stride 2) <= net(stride 1) x (1 + the larger of the two spreads)", "",
            "| pair | precision | stride-2 net ms | stride-1 net ms | ratio | allowance | holds |", "|---|---|---|---|---|---|---|"]
    lost = []
    for s2, s1 in PAIRS:
        for prec in ("int8", "f32"):
            x, y = cell[(s2, prec)], cell[(s1, prec)]
            ratio, allow = x["net_median_ms"] / y["net_median_ms"], max(x["net_spread"], y["net_spread"])
            ok = ratio <= 1.0 + allow
            if not ok:
                lost.append((s2, prec, ratio))
            out.append("| %s / %s | %s | %.3f | %.3f | %.3f | %.1f %% | %s |" % (s2, s1, prec, x["net_median_ms"], y["net_median_ms"], ratio, 100 * allow,
                                                                                 "yes" if ok else "NO"))
    out += ["", "The condition holds for every pair." if not lost else
            "The condition does NOT hold for: " + ", ".join("%s %s (%.3f)" % v for v in lost) + " -- see the note below."]
    if a.note:
        out += ["", open(a.note).read().rstrip()]
    if a.bench:
        out += ["", "## bench.py (the headline workload), same call at this commit and at its parent", "", "| tree | result line |", "|---|---|"]
        for spec in a.bench:
            label, line = spec.split("=", 1)
            out.append("| %s | `%s` |" % (label, line.strip()))
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    open(a.md, "w").write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (with --md: read them from it)")
    ap.add_argument("--md", default=None, help="write the tables from --out; runs nothing")
    ap.add_argument("--note", default=None, help="with --md: a text file appended under the condition table (which path loses the time, and why)")
    ap.add_argument("--bench", action="append", help="with --md: LABEL=bench.py's JSON result line (or the fields of it to show)")
    a = ap.parse_args()
    if a.md:
        write_md(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
