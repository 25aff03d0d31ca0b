"""Which kernels and list operations every batch and stream entry point enqueues, per model and mode, pinned without a GPU: the
library's host code on the stub runtime of tests/sanitize (hip_stub.cpp records every launch's device name, every memset and copy when KWS_STUB_RECORD
names a file; kernels do not run), driven by host_driver.cpp --routes -- each call once with B = 5.  The seven shipped models, one MFE-block model
(tests/test_gpu_mfe_model.py's), and -- on a second build with -DKWS_DEV_SWITCHES -- KWS_DEV_FAST_ENTRY=2 / 3 for the two routes no shipped model takes
(from-cepstra entry of an un-fused graph, exact kernels throughout).  ROUTES below was written from the trace of the commit that added this test and
checked against DESIGN section 4.6; kernel arguments (which list, which plan) are not visible here: the GPU tests see them."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

from kws_testlib import MODELS, ROOT, synth_model_blob

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) and shutil.which("gcc")), reason="needs ROCm's clang++ and gcc")

FORCED = ("cfg2_mfcc40_int8.kwsm", "l476_no_yes_f32.kwsm")


def build(out, extra=None):
    exe = os.path.join(out, "kws_host_san")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize"), "OUT=" + out, exe] + (["EXTRA=" + extra] if extra else []))
    return exe


def record(exe, models, rec_file, **switches):
    env = dict(os.environ, KWS_STUB_RECORD=rec_file, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **switches)
    p = subprocess.run([exe, "--routes"] + models, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.count(" rc 0") == len(models), p.stdout
    return open(rec_file).read()


def mfe_model(directory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import MFE_MODEL_KW
    path = os.path.join(directory, "mfe_block.kwsm")
    with open(path, "wb") as f:
        f.write(synth_model_blob(**MFE_MODEL_KW))
    return path


def full_trace(san_dir, san_dev_dir, tmp):
    """every recorded line of the whole route set: product build over the shipped models and the MFE-block model, then the forced entry tiers"""
    os.makedirs(tmp, exist_ok=True)
    exe, exe_dev = build(san_dir), build(san_dev_dir, "-DKWS_DEV_SWITCHES")
    rec = os.path.join(tmp, "routes.rec")
    text = record(exe, sorted(glob.glob(os.path.join(MODELS, "*.kwsm"))) + [mfe_model(tmp)], rec)
    for entry in ("2", "3"):
        forced = record(exe_dev, [os.path.join(MODELS, m) for m in FORCED], rec, KWS_DEV_FAST_ENTRY=entry)
        text += re.sub(r"^ROUTE ", "ROUTE entry%s:" % entry, forced, flags=re.M)
    return text


def short_name(demangled):
    """`void kws_fast_kernel<5, 1, false>(int, float*)` -> `kws_fast_kernel<5, 1, false>`"""
    s = demangled[5:] if demangled.startswith("void ") else demangled
    depth = 0
    for i, c in enumerate(s):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return s[:i]
    return s


def routes_of(trace):
    """{tag: [operation, ...]}: kernel launches by demangled name, enqueued memsets and copies by kind and byte count, the call's return code last"""
    routes, cur = {}, None
    for ln in trace.splitlines():
        w = ln.split()
        if w[0] == "ROUTE":
            cur = routes.setdefault(" ".join(w[1:]), [])
        elif cur is None:
            continue
        elif w[0] == "launch":
            cur.append(short_name(ln.split(" | ", 1)[1]))
        elif w[0] in ("memset_async", "memcpy_async"):                # (the blocking ones are set-up: the lists' first allocation)
            cur.append("%s %s" % (w[0], w[1].split("=")[1]))
        elif w[0] == "rc":
            cur.append(ln)
            cur = None
    return routes


# One block per distinct sequence: the operations, then (indented) every "<model> <mode> <call>" that enqueues exactly them.  "entry2:" / "entry3:": the
# development build with KWS_DEV_FAST_ENTRY=2 / 3.  Template arguments of kws_fast_kernel: <NZ, DG, PROF, FROM_CEP, NET, QCP, MFE>.
ROUTES_TABLE = """
kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm exact classify_features
    cfg2_mfcc40_f32.kwsm exact classify_scores
    cfg5_dscnn_mfcc40_f32.kwsm exact classify_features
    cfg5_dscnn_mfcc40_f32.kwsm exact classify_scores
kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; rc 0
    cfg2_mfcc40_f32.kwsm exact extract_mfcc
    cfg2_mfcc40_int8.kwsm exact extract_mfcc
    cfg5_dscnn_mfcc40_f32.kwsm exact extract_mfcc
    cfg5_dscnn_mfcc40_int8.kwsm exact extract_mfcc
    entry2:cfg2_mfcc40_int8.kwsm exact extract_mfcc
    entry3:cfg2_mfcc40_int8.kwsm exact extract_mfcc
kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm exact cmvn_inference_features
    cfg2_mfcc40_f32.kwsm exact cmvn_inference_scores
    cfg5_dscnn_mfcc40_f32.kwsm exact cmvn_inference_features
    cfg5_dscnn_mfcc40_f32.kwsm exact cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; rc 0
    cfg2_mfcc40_f32.kwsm exact streams_step_1
    cfg2_mfcc40_f32.kwsm exact streams_step_2
    cfg2_mfcc40_f32.kwsm exact streams_step_3
    cfg2_mfcc40_f32.kwsm fast streams_step_1
    cfg2_mfcc40_f32.kwsm fast streams_step_2
    cfg2_mfcc40_f32.kwsm fast streams_step_3
    cfg2_mfcc40_int8.kwsm exact streams_step_1
    cfg2_mfcc40_int8.kwsm exact streams_step_2
    cfg2_mfcc40_int8.kwsm exact streams_step_3
    cfg2_mfcc40_int8.kwsm fast streams_step_1
    cfg2_mfcc40_int8.kwsm fast streams_step_2
    cfg2_mfcc40_int8.kwsm fast streams_step_3
    cfg5_dscnn_mfcc40_f32.kwsm exact streams_step_1
    cfg5_dscnn_mfcc40_f32.kwsm exact streams_step_2
    cfg5_dscnn_mfcc40_f32.kwsm exact streams_step_3
    cfg5_dscnn_mfcc40_f32.kwsm fast streams_step_1
    cfg5_dscnn_mfcc40_f32.kwsm fast streams_step_2
    cfg5_dscnn_mfcc40_f32.kwsm fast streams_step_3
    cfg5_dscnn_mfcc40_int8.kwsm exact streams_step_1
    cfg5_dscnn_mfcc40_int8.kwsm exact streams_step_2
    cfg5_dscnn_mfcc40_int8.kwsm exact streams_step_3
    cfg5_dscnn_mfcc40_int8.kwsm fast streams_step_1
    cfg5_dscnn_mfcc40_int8.kwsm fast streams_step_2
    cfg5_dscnn_mfcc40_int8.kwsm fast streams_step_3
    entry2:cfg2_mfcc40_int8.kwsm exact streams_step_1
    entry2:cfg2_mfcc40_int8.kwsm exact streams_step_2
    entry2:cfg2_mfcc40_int8.kwsm exact streams_step_3
    entry2:cfg2_mfcc40_int8.kwsm fast streams_step_1
    entry2:cfg2_mfcc40_int8.kwsm fast streams_step_2
    entry2:cfg2_mfcc40_int8.kwsm fast streams_step_3
    entry3:cfg2_mfcc40_int8.kwsm exact streams_step_1
    entry3:cfg2_mfcc40_int8.kwsm exact streams_step_2
    entry3:cfg2_mfcc40_int8.kwsm exact streams_step_3
    entry3:cfg2_mfcc40_int8.kwsm fast streams_step_1
    entry3:cfg2_mfcc40_int8.kwsm fast streams_step_2
    entry3:cfg2_mfcc40_int8.kwsm fast streams_step_3
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<512, false, false> ; kws_maf_kernel ; rc 0
    cfg2_mfcc40_f32.kwsm exact streams_step_4
    cfg2_mfcc40_f32.kwsm exact streams_step_5
    cfg5_dscnn_mfcc40_f32.kwsm exact streams_step_4
    cfg5_dscnn_mfcc40_f32.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<4, 5, false, false, false, 0, false> ; memset_async 4 ; kws_fast_kernel_w3<4, 5, false, false, true, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm fast classify_features
memset_async 4 ; kws_fast_kernel_w3<4, 5, false, false, true, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm fast classify_scores
memset_async 4 ; kws_fast_kernel<4, 5, false, false, false, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_cmvn_nn_kernel<false> ; rc 0
    cfg2_mfcc40_f32.kwsm fast extract_mfcc
    cfg2_mfcc40_int8.kwsm fast extract_mfcc
    cfg5_dscnn_mfcc40_int8.kwsm fast extract_mfcc
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm fast cmvn_inference_features
    cfg5_dscnn_mfcc40_f32.kwsm fast cmvn_inference_features
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<512, false, false> ; rc 0
    cfg2_mfcc40_f32.kwsm fast cmvn_inference_scores
    cfg5_dscnn_mfcc40_f32.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<512, false, false> ; kws_maf_kernel ; rc 0
    cfg2_mfcc40_f32.kwsm fast streams_step_4
    cfg2_mfcc40_f32.kwsm fast streams_step_5
    cfg5_dscnn_mfcc40_f32.kwsm fast streams_step_4
    cfg5_dscnn_mfcc40_f32.kwsm fast streams_step_5
kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; kws_nn_mfma_kernel<64> ; rc 0
    cfg2_mfcc40_int8.kwsm exact classify_features
    cfg2_mfcc40_int8.kwsm exact classify_scores
    entry2:cfg2_mfcc40_int8.kwsm exact classify_features
    entry2:cfg2_mfcc40_int8.kwsm exact classify_scores
    entry3:cfg2_mfcc40_int8.kwsm exact classify_features
    entry3:cfg2_mfcc40_int8.kwsm exact classify_scores
kws_cmvn_nn_kernel<false> ; kws_nn_mfma_kernel<64> ; rc 0
    cfg2_mfcc40_int8.kwsm exact cmvn_inference_features
    cfg2_mfcc40_int8.kwsm exact cmvn_inference_scores
    entry2:cfg2_mfcc40_int8.kwsm exact cmvn_inference_features
    entry2:cfg2_mfcc40_int8.kwsm exact cmvn_inference_scores
    entry3:cfg2_mfcc40_int8.kwsm exact cmvn_inference_features
    entry3:cfg2_mfcc40_int8.kwsm exact cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; kws_cmvn_nn_kernel<false> ; kws_nn_mfma_kernel<64> ; kws_maf_kernel ; rc 0
    cfg2_mfcc40_int8.kwsm exact streams_step_4
    cfg2_mfcc40_int8.kwsm exact streams_step_5
    entry2:cfg2_mfcc40_int8.kwsm exact streams_step_4
    entry2:cfg2_mfcc40_int8.kwsm exact streams_step_5
    entry3:cfg2_mfcc40_int8.kwsm exact streams_step_4
    entry3:cfg2_mfcc40_int8.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<4, 5, false, false, false, 64, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<64> ; kws_cmvn_nn_kernel<false> ; kws_nn_mfma_kernel<64> ; rc 0
    cfg2_mfcc40_int8.kwsm fast classify_features
    cfg2_mfcc40_int8.kwsm fast classify_scores
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<64> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_mfma_kernel<64> ; rc 0
    cfg2_mfcc40_int8.kwsm fast cmvn_inference_features
    cfg2_mfcc40_int8.kwsm fast cmvn_inference_scores
    entry2:cfg2_mfcc40_int8.kwsm fast cmvn_inference_features
    entry2:cfg2_mfcc40_int8.kwsm fast cmvn_inference_scores
    entry3:cfg2_mfcc40_int8.kwsm fast cmvn_inference_features
    entry3:cfg2_mfcc40_int8.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<64> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_mfma_kernel<64> ; kws_maf_kernel ; rc 0
    cfg2_mfcc40_int8.kwsm fast streams_step_4
    cfg2_mfcc40_int8.kwsm fast streams_step_5
    entry2:cfg2_mfcc40_int8.kwsm fast streams_step_4
    entry2:cfg2_mfcc40_int8.kwsm fast streams_step_5
    entry3:cfg2_mfcc40_int8.kwsm fast streams_step_4
    entry3:cfg2_mfcc40_int8.kwsm fast streams_step_5
memset_async 4 ; memset_async 4 ; kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_nn_f32_kernel<512, false, false> ; memcpy_async 4 ; rc 0
    cfg5_dscnn_mfcc40_f32.kwsm fast classify_features
    cfg5_dscnn_mfcc40_f32.kwsm fast classify_scores
memset_async 4 ; memset_async 4 ; kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; rc 0
    cfg5_dscnn_mfcc40_f32.kwsm fast extract_mfcc
    entry3:cfg2_mfcc40_int8.kwsm fast extract_mfcc
kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; kws_nn_kernel<16, false, false> ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm exact classify_features
    cfg5_dscnn_mfcc40_int8.kwsm exact classify_scores
kws_cmvn_nn_kernel<false> ; kws_nn_kernel<16, false, false> ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm exact cmvn_inference_features
    cfg5_dscnn_mfcc40_int8.kwsm exact cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; kws_cmvn_nn_kernel<false> ; kws_nn_kernel<16, false, false> ; kws_maf_kernel ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm exact streams_step_4
    cfg5_dscnn_mfcc40_int8.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<4, 5, false, false, false, 0, false> ; kws_nn_kernel<16, false, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_kernel<16, false, false> ; kws_cmvn_nn_kernel<false> ; kws_nn_kernel<16, false, false> ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm fast classify_features
    cfg5_dscnn_mfcc40_int8.kwsm fast classify_scores
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_kernel<16, false, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_kernel<16, false, false> ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm fast cmvn_inference_features
    cfg5_dscnn_mfcc40_int8.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 8, 40, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_kernel<16, false, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_kernel<16, false, false> ; kws_maf_kernel ; rc 0
    cfg5_dscnn_mfcc40_int8.kwsm fast streams_step_4
    cfg5_dscnn_mfcc40_int8.kwsm fast streams_step_5
kws_mfcc8_kernel<true, 12, 32, false, false, 2> ; kws_nn_mfma_kernel<16> ; rc 0
    l432_trick_or_treat.kwsm exact classify_features
    l432_trick_or_treat.kwsm exact classify_scores
kws_mfcc8_kernel<true, 12, 32, false, false, 2> ; rc 0
    l432_trick_or_treat.kwsm exact extract_mfcc
kws_cmvn_nn_kernel<true> ; rc 0
    l432_trick_or_treat.kwsm exact cmvn_inference_features
    l432_trick_or_treat.kwsm exact cmvn_inference_scores
    l476_no_yes.kwsm exact cmvn_inference_features
    l476_no_yes.kwsm exact cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 12, 32, false, false, 0> ; rc 0
    l432_trick_or_treat.kwsm exact streams_step_1
    l432_trick_or_treat.kwsm exact streams_step_2
    l432_trick_or_treat.kwsm exact streams_step_3
    l432_trick_or_treat.kwsm fast streams_step_1
    l432_trick_or_treat.kwsm fast streams_step_2
    l432_trick_or_treat.kwsm fast streams_step_3
kws_mfcc_kernel<9, false, false, 12, 32, false, false, 0> ; kws_cmvn_nn_kernel<true> ; kws_maf_kernel ; rc 0
    l432_trick_or_treat.kwsm exact streams_step_4
    l432_trick_or_treat.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<8, 4, false, false, false, 16, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 12, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<16> ; kws_cmvn_nn_kernel<true> ; rc 0
    l432_trick_or_treat.kwsm fast classify_features
    l432_trick_or_treat.kwsm fast classify_scores
memset_async 4 ; kws_fast_kernel<8, 4, false, false, false, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 12, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_cmvn_nn_kernel<false> ; rc 0
    l432_trick_or_treat.kwsm fast extract_mfcc
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<16> ; kws_cmvn_nn_kernel<true> ; memcpy_async 4 ; rc 0
    l432_trick_or_treat.kwsm fast cmvn_inference_features
    l432_trick_or_treat.kwsm fast cmvn_inference_scores
    l476_no_yes.kwsm fast cmvn_inference_features
    l476_no_yes.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 12, 32, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<16> ; kws_cmvn_nn_kernel<true> ; memcpy_async 4 ; kws_maf_kernel ; rc 0
    l432_trick_or_treat.kwsm fast streams_step_4
    l432_trick_or_treat.kwsm fast streams_step_5
kws_mfcc8_kernel<true, 4, 32, false, false, 2> ; kws_nn_mfma_kernel<16> ; rc 0
    l476_no_yes.kwsm exact classify_features
    l476_no_yes.kwsm exact classify_scores
kws_mfcc8_kernel<true, 4, 32, false, false, 2> ; rc 0
    l476_no_yes.kwsm exact extract_mfcc
    l476_no_yes_f32.kwsm exact extract_mfcc
    entry2:l476_no_yes_f32.kwsm exact extract_mfcc
    entry3:l476_no_yes_f32.kwsm exact extract_mfcc
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; rc 0
    l476_no_yes.kwsm exact streams_step_1
    l476_no_yes.kwsm exact streams_step_2
    l476_no_yes.kwsm exact streams_step_3
    l476_no_yes.kwsm fast streams_step_1
    l476_no_yes.kwsm fast streams_step_2
    l476_no_yes.kwsm fast streams_step_3
    l476_no_yes_f32.kwsm exact streams_step_1
    l476_no_yes_f32.kwsm exact streams_step_2
    l476_no_yes_f32.kwsm exact streams_step_3
    l476_no_yes_f32.kwsm fast streams_step_1
    l476_no_yes_f32.kwsm fast streams_step_2
    l476_no_yes_f32.kwsm fast streams_step_3
    mfe_block.kwsm exact streams_step_1
    mfe_block.kwsm exact streams_step_2
    mfe_block.kwsm exact streams_step_3
    mfe_block.kwsm fast streams_step_1
    mfe_block.kwsm fast streams_step_2
    mfe_block.kwsm fast streams_step_3
    entry2:l476_no_yes_f32.kwsm exact streams_step_1
    entry2:l476_no_yes_f32.kwsm exact streams_step_2
    entry2:l476_no_yes_f32.kwsm exact streams_step_3
    entry2:l476_no_yes_f32.kwsm fast streams_step_1
    entry2:l476_no_yes_f32.kwsm fast streams_step_2
    entry2:l476_no_yes_f32.kwsm fast streams_step_3
    entry3:l476_no_yes_f32.kwsm exact streams_step_1
    entry3:l476_no_yes_f32.kwsm exact streams_step_2
    entry3:l476_no_yes_f32.kwsm exact streams_step_3
    entry3:l476_no_yes_f32.kwsm fast streams_step_1
    entry3:l476_no_yes_f32.kwsm fast streams_step_2
    entry3:l476_no_yes_f32.kwsm fast streams_step_3
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; kws_cmvn_nn_kernel<true> ; kws_maf_kernel ; rc 0
    l476_no_yes.kwsm exact streams_step_4
    l476_no_yes.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<4, 4, false, false, false, 16, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<16> ; kws_cmvn_nn_kernel<true> ; rc 0
    l476_no_yes.kwsm fast classify_features
    l476_no_yes.kwsm fast classify_scores
memset_async 4 ; kws_fast_kernel<4, 4, false, false, false, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_cmvn_nn_kernel<false> ; rc 0
    l476_no_yes.kwsm fast extract_mfcc
    l476_no_yes_f32.kwsm fast extract_mfcc
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<16> ; kws_cmvn_nn_kernel<true> ; memcpy_async 4 ; kws_maf_kernel ; rc 0
    l476_no_yes.kwsm fast streams_step_4
    l476_no_yes.kwsm fast streams_step_5
kws_mfcc8_kernel<true, 4, 32, false, false, 2> ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm exact classify_features
    l476_no_yes_f32.kwsm exact classify_scores
    entry2:l476_no_yes_f32.kwsm exact classify_features
    entry2:l476_no_yes_f32.kwsm exact classify_scores
    entry3:l476_no_yes_f32.kwsm exact classify_features
    entry3:l476_no_yes_f32.kwsm exact classify_scores
kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm exact cmvn_inference_features
    l476_no_yes_f32.kwsm exact cmvn_inference_scores
    entry2:l476_no_yes_f32.kwsm exact cmvn_inference_features
    entry2:l476_no_yes_f32.kwsm exact cmvn_inference_scores
    entry3:l476_no_yes_f32.kwsm exact cmvn_inference_features
    entry3:l476_no_yes_f32.kwsm exact cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<1024, false, false> ; kws_maf_kernel ; rc 0
    l476_no_yes_f32.kwsm exact streams_step_4
    l476_no_yes_f32.kwsm exact streams_step_5
    entry2:l476_no_yes_f32.kwsm exact streams_step_4
    entry2:l476_no_yes_f32.kwsm exact streams_step_5
    entry3:l476_no_yes_f32.kwsm exact streams_step_4
    entry3:l476_no_yes_f32.kwsm exact streams_step_5
memset_async 4 ; kws_fast_kernel<4, 4, false, false, false, 0, false> ; memset_async 4 ; kws_fast_kernel_w3<4, 4, false, false, true, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm fast classify_features
memset_async 4 ; kws_fast_kernel_w3<4, 4, false, false, true, 0, false> ; memset_async 4 ; kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm fast classify_scores
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm fast cmvn_inference_features
    entry2:l476_no_yes_f32.kwsm fast cmvn_inference_features
    entry3:l476_no_yes_f32.kwsm fast cmvn_inference_features
memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<1024, false, false> ; rc 0
    l476_no_yes_f32.kwsm fast cmvn_inference_scores
    entry2:l476_no_yes_f32.kwsm fast cmvn_inference_scores
    entry3:l476_no_yes_f32.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_f32_kernel<1024, false, false> ; kws_maf_kernel ; rc 0
    l476_no_yes_f32.kwsm fast streams_step_4
    l476_no_yes_f32.kwsm fast streams_step_5
    entry2:l476_no_yes_f32.kwsm fast streams_step_4
    entry2:l476_no_yes_f32.kwsm fast streams_step_5
    entry3:l476_no_yes_f32.kwsm fast streams_step_4
    entry3:l476_no_yes_f32.kwsm fast streams_step_5
kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_mfe_norm_kernel ; kws_quantize_kernel ; kws_nn_kernel<16, false, false> ; rc 0
    mfe_block.kwsm exact classify_features
    mfe_block.kwsm exact classify_scores
kws_mfcc8_kernel<false, 4, 32, false, false, 2> ; kws_mfe_norm_kernel ; kws_quantize_kernel ; rc 0
    mfe_block.kwsm exact extract_mfcc
kws_unring_kernel ; kws_mfe_norm_kernel ; kws_quantize_kernel ; kws_nn_kernel<16, false, false> ; rc 0
    mfe_block.kwsm exact cmvn_inference_features
    mfe_block.kwsm exact cmvn_inference_scores
    mfe_block.kwsm fast cmvn_inference_features
    mfe_block.kwsm fast cmvn_inference_scores
kws_mfcc_kernel<9, false, false, 4, 32, false, false, 0> ; kws_unring_kernel ; kws_mfe_norm_kernel ; kws_quantize_kernel ; kws_nn_kernel<16, false, false> ; kws_maf_kernel ; rc 0
    mfe_block.kwsm exact streams_step_4
    mfe_block.kwsm exact streams_step_5
    mfe_block.kwsm fast streams_step_4
    mfe_block.kwsm fast streams_step_5
memset_async 4 ; kws_fast_kernel<4, 4, false, false, false, 0, true> ; kws_mfe_norm_kernel ; kws_quantize_kernel ; kws_nn_kernel<16, false, false> ; rc 0
    mfe_block.kwsm fast classify_features
    mfe_block.kwsm fast classify_scores
memset_async 4 ; kws_fast_kernel<4, 4, false, false, false, 0, true> ; kws_mfe_norm_kernel ; kws_quantize_kernel ; rc 0
    mfe_block.kwsm fast extract_mfcc
memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_nn_mfma_kernel<64> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; kws_nn_mfma_kernel<64> ; rc 0
    entry2:cfg2_mfcc40_int8.kwsm fast classify_features
    entry2:cfg2_mfcc40_int8.kwsm fast classify_scores
memset_async 4 ; kws_mfcc8_kernel<false, 8, 40, false, false, 2> ; memset_async 4 ; memset_async 4 ; kws_fast_kernel<4, 4, false, true, false, 0, false> ; kws_cmvn_nn_kernel<false> ; memcpy_async 4 ; rc 0
    entry2:cfg2_mfcc40_int8.kwsm fast extract_mfcc
memset_async 4 ; memset_async 4 ; kws_mfcc8_kernel<true, 4, 32, false, false, 2> ; kws_fast_kernel<4, 4, false, true, true, 0, false> ; kws_nn_f32_kernel<1024, false, false> ; memcpy_async 4 ; rc 0
    entry2:l476_no_yes_f32.kwsm fast classify_features
    entry2:l476_no_yes_f32.kwsm fast classify_scores
    entry3:l476_no_yes_f32.kwsm fast classify_features
    entry3:l476_no_yes_f32.kwsm fast classify_scores
memset_async 4 ; memset_async 4 ; kws_mfcc8_kernel<true, 4, 32, false, false, 2> ; rc 0
    entry2:l476_no_yes_f32.kwsm fast extract_mfcc
    entry3:l476_no_yes_f32.kwsm fast extract_mfcc
memset_async 4 ; memset_async 4 ; kws_mfcc8_kernel<true, 8, 40, false, true, 2> ; kws_nn_mfma_kernel<64> ; rc 0
    entry3:cfg2_mfcc40_int8.kwsm fast classify_features
    entry3:cfg2_mfcc40_int8.kwsm fast classify_scores
"""


def parse_table(text):
    routes, ops = {}, None
    for ln in text.splitlines():
        if ln.startswith("    "):
            routes[ln.strip()] = ops
        elif ln.strip():
            ops = ln.split(" ; ")
    return routes


ROUTES = parse_table(ROUTES_TABLE)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kws_routes")
    return routes_of(full_trace(str(tmp / "san"), str(tmp / "san_dev"), str(tmp)))


def test_every_entry_point_enqueues_the_pinned_operations(routes):
    assert sorted(routes) == sorted(ROUTES)
    wrong = {tag: (ops, ROUTES[tag]) for tag, ops in routes.items() if ops != ROUTES[tag]}
    assert not wrong, "\n".join("%s:\n  got      %s\n  expected %s" % (tag, got, want) for tag, (got, want) in sorted(wrong.items()))
