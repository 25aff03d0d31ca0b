#!/usr/bin/env python3
"""Development aid: what the MFE block costs at the general DSP shapes A - D of tests/mfe_general_shapes.py, 8 192 clips resident in HBM.
Writes profiles/mfe_general_rate.md (and a copy to every path on the command line).

Per shape, timed between HIP events on the default stream (10 calls per sample after 3 warm-up calls; every figure the median of three
samples, the variants of a comparison taken in alternation -- a, b, a, b, a, b -- so that a clock or thermal drift hits both; the spread is
max - min of the three):
  spectral   kws_mfe_batch_device: the tuned kernel over chunks of frames (shape A) or the cooperative kernel
  block      kws_extract_mfe_batch_device: the spectral launch(es) + the normalisation kernel; `norm` = block - spectral
  call       kws_run_classifier_batch_device, int8 graph: block (+ the int8 tensor in the same pass) + the network
against two reference points of the same run: the general MFCC path at the same spectral shape (kws_mfcc_batch_device and the whole call of
an MFCC-block model with the same framing, fft and filters, 13 cepstra), and the tuned 49 x 32 MFE model per frame.
Comparisons (development library, switches read per call): shape A's tuned-chunk route against the cooperative route
(KWS_DEV_GENERIC_NO_TUNED_SPECTRAL), and the LDS form of the normalisation against its global-memory form (KWS_DEV_MFE_NORM_GLOBAL) on every
shape both can run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
import mfe_general_shapes as G  # noqa: E402
from make_golden import MFE_MODEL_KW  # noqa: E402

B, CALLS, WARM = 8192, 10, 3
pkg = load_package(dev=True)
out_lines = []


def say(s=""):
    print(s, flush=True)
    out_lines.append(s)


def sample(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(CALLS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / CALLS


def alternate(fns):
    """{name: (median ms, spread ms)} of three samples per variant, taken in alternation"""
    got = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            got[k].append(sample(fn))
    return {k: (sorted(v)[1], max(v) - min(v)) for k, v in got.items()}


def with_env(name, fn):
    def run():
        os.environ[name] = "1"
        try:
            fn()
        finally:
            del os.environ[name]
    return run


say("# MFE block at general shapes: %d clips resident, %s" % (B, torch.cuda.get_device_name(0)))
say()
say("ms per call: median of three alternating samples of %d calls (spread = max - min).  `norm` = block - spectral." % CALLS)
say()
say("| shape | frames x filters | spectral kernel | spectral | block | norm | call (int8) | ns / frame (call) | MFCC spectral, same shape | MFCC call |")
say("|---|---|---|---|---|---|---|---|---|---|")
compare = []
for tag in ("A", "B", "C", "D"):
    kw = G.SHAPES[tag]
    n = kw.get("raw_samples", 16000)
    pcm = torch.empty((B, n), dtype=torch.int16, device="cuda:0")
    pkg.synth_clips_device(0, 0, B, n, pcm.data_ptr())
    gm = pkg.Model(blob=G.blob(tag))
    gc = pkg.Model(blob=G.blob(dict(kw, dsp_block="mfcc", ncep=13)))
    rows, cols = G.ROWS_COLS[tag]
    mel = torch.empty((B, rows * cols), dtype=torch.float32, device="cuda:0")
    ft = torch.empty((B, rows * cols), dtype=torch.float32, device="cuda:0")
    sc = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
    cep = torch.empty((B, gc.n_features), dtype=torch.float32, device="cuda:0")
    spectral = lambda: gm.mfe_batch_device(pcm.data_ptr(), B, mel.data_ptr())
    block = lambda: gm.extract_mfe_batch_device(pcm.data_ptr(), B, ft.data_ptr())
    call = lambda: gm.run_classifier_batch_device(pcm.data_ptr(), B, sc.data_ptr(), ft.data_ptr())
    r = alternate({"spectral": spectral, "block": block, "call": call,
                   "mfcc_spectral": lambda: gc.mfcc_batch_device(pcm.data_ptr(), B, cep.data_ptr()),
                   "mfcc_call": lambda: gc.run_classifier_batch_device(pcm.data_ptr(), B, sc.data_ptr())})
    f = lambda k: "%.3f (%.3f)" % r[k]
    say("| %s | %d x %d | %s | %s | %s | %.3f | %s | %.2f | %s | %s |" % (tag, rows, cols, gm.mfcc_kernel, f("spectral"), f("block"), r["block"][0] - r["spectral"][0],
                                                                     f("call"), r["call"][0] * 1e6 / (B * rows), f("mfcc_spectral"), f("mfcc_call")))
    c = alternate({"lds": block, "global": with_env("KWS_DEV_MFE_NORM_GLOBAL", block)})
    compare.append("| %s | normalisation: LDS form vs global-memory form (block) | %.3f (%.3f) | %.3f (%.3f) |" % ((tag,) + c["lds"] + c["global"]))
    if gm.mfcc_kernel.startswith("kws_mfcc8"):
        c = alternate({"chunks": spectral, "coop": with_env("KWS_DEV_GENERIC_NO_TUNED_SPECTRAL", spectral)})
        compare.append("| %s | spectral: tuned kernel over chunks vs cooperative kernel | %.3f (%.3f) | %.3f (%.3f) |" % ((tag,) + c["chunks"] + c["coop"]))
    gm.close(); gc.close()
    del pcm, mel, ft, cep
say()
say("| shape | comparison | first, ms (spread) | second, ms (spread) |")
say("|---|---|---|---|")
for ln in compare:
    say(ln)
pcm = torch.empty((B, 16000), dtype=torch.int16, device="cuda:0")
pkg.synth_clips_device(0, 0, B, 16000, pcm.data_ptr())
gm = pkg.Model(blob=G.blob(MFE_MODEL_KW))
ft = torch.empty((B, gm.n_features), dtype=torch.float32, device="cuda:0")
sc = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda:0")
r = alternate({"block": lambda: gm.extract_mfe_batch_device(pcm.data_ptr(), B, ft.data_ptr()),
               "call": lambda: gm.run_classifier_batch_device(pcm.data_ptr(), B, sc.data_ptr(), ft.data_ptr())})
say()
say("Tuned MFE model (49 x 32, %s): block %.3f (%.3f) ms, call %.3f (%.3f) ms = %.2f ns / frame." % ((gm.mfcc_kernel,) + r["block"] + r["call"] + (r["call"][0] * 1e6 / (B * 49),)))
gm.close()
for path in [os.path.join(ROOT, "profiles", "mfe_general_rate.md")] + sys.argv[1:]:           # further copies: paths on the command line
    with open(path, "w") as fh:
        fh.write("\n".join(out_lines) + "\n")
