"""No GPU: csrc/kws_fast_scale.h -- the fast kernel leaves its power rows unscaled; the plan uploads the mel tap weights multiplied by the power
spectrum's scale instead (a fast plan itself needs a device: its tables are uploaded as they are built, so the shared helper is run through a
stand-alone driver, tests/fast_pscale/fast_pscale_driver.cpp).  The move changes no bit only if the scale is a power of two and every scaled weight is
the unscaled one times it EXACTLY -- none of them subnormal.  The weights are the reference's filterbanks (the oracle's, pinned to the reference by
tests/test_oracle_golden.py) of the shipped configurations, and the smallest weights a filterbank can hold."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from kws_testlib import L476_CONFIG, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("g++")
    if not cxx:
        pytest.skip("needs a C++ compiler")
    exe = str(tmp_path_factory.mktemp("fast_pscale") / "fast_pscale_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "fast_pscale", "fast_pscale_driver.cpp")])
    return exe


def scale(driver, tmp_path, w, fft_length=256):
    src, dst = str(tmp_path / "w.bin"), str(tmp_path / "ws.bin")
    np.ascontiguousarray(w, np.float32).tofile(src)
    head = subprocess.run([driver, str(fft_length), src, dst], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    info = dict(pscale=float.fromhex(head[1]), bits=int(head[3], 16), n=int(head[5]), subnormal=int(head[7]))
    return info, np.fromfile(dst, np.float32)


def test_the_scale_is_a_power_of_two(driver, tmp_path):
    info, _ = scale(driver, tmp_path, np.ones(4, np.float32))
    # 1 / 256 x 2^-30 (int16 samples, squared) x 1/4 (the split leaves twice the reference's bins)
    assert info["pscale"] == 2.0 ** -40
    assert info["bits"] & 0x007FFFFF == 0 and 0 < (info["bits"] >> 23) < 255      # no mantissa bit, a normal exponent, positive


@pytest.mark.parametrize("kw", [dict(), dict(high_frequency=0), dict(num_filters=40, high_frequency=0), dict(quantize_filterbank=1),
                                dict(num_filters=40, high_frequency=0, quantize_filterbank=1)],
                         ids=["l476", "l432", "40", "l476_qfb", "40_qfb"])
def test_every_uploaded_tap_weight_is_the_unscaled_one_times_the_scale_exactly(driver, tmp_path, kw):
    fb = Oracle().filterbanks(L476_CONFIG().copy(**kw)).ravel()
    assert (fb != 0).sum() > 30                                                     # (narrow triangles: most slopes hold one or two bins)
    info, out = scale(driver, tmp_path, fb)
    assert info["n"] == fb.size and info["subnormal"] == 0
    exact = fb.astype(np.float64) * info["pscale"]                                  # exact in double: 24 bits x a power of two
    assert (out.astype(np.float64) == exact).all()
    assert (np.signbit(out) == np.signbit(fb)).all() and ((out == 0) == (fb == 0)).all()
    assert (np.abs(out[out != 0]) >= TINY).all()                                    # none subnormal
    # and back: nothing was rounded on the way
    assert ((out.astype(np.float64) / info["pscale"]).astype(np.float32).view(np.uint32) == fb.view(np.uint32)).all()


def test_the_smallest_weights_stay_normal_and_a_subnormal_result_is_reported(driver, tmp_path):
    # a triangular filter's smallest non-zero weight is 1 / (bins of its slope) >= 1 / 128; a quantised one 1 / 256 -- 1e-7 leaves five decades of margin
    w = np.array([1.0, 1.0 / 128, 1.0 / 256, 1e-7, 0.0, -0.0], np.float32)
    info, out = scale(driver, tmp_path, w)
    assert info["subnormal"] == 0 and (np.abs(out[:4]) >= TINY).all() and (out[:4].astype(np.float64) == w[:4].astype(np.float64) * 2.0 ** -40).all()
    assert out[4] == 0 and out[5] == 0 and not np.signbit(out[4]) and np.signbit(out[5])
    # what the plan refuses: a weight whose product with the scale falls below the normal range
    info, out = scale(driver, tmp_path, np.array([1.0, 1e-27, -1e-30], np.float32))
    assert info["subnormal"] == 2
