"""kws_live_* without a GPU: the symbols are exported and bound, and the host side of the calls -- window counts per push, argument checks,
the stream API's slicing rules, the bookkeeping of pushes that do work -- runs under ASan + UBSan against the stub HIP runtime of
tests/sanitize (kernels do not run there)."""
import ctypes
import glob
import os
import subprocess

import pytest

from kws_testlib import MODELS, ROOT

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
# the flags of tests/sanitize/Makefile's host-only build of the library
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
SHIPPED = ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm", "cfg2_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
SYMBOLS = {"kws_live_create", "kws_live_destroy", "kws_live_reset", "kws_live_window_count", "kws_live_push_device"}


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_live_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert callable(pkg.Model.live_streams)
    for m in ("push_device", "window_count", "reset", "close"):
        assert callable(getattr(pkg.LiveStreams, m)), m


@pytest.fixture(scope="module")
def live_exe(host_exe):
    """tests/live/live_host_driver.cpp linked with the host objects host_exe built, plus the scan and live units compiled the same way"""
    base = os.path.dirname(host_exe)
    out = os.path.join(base, "live")                # a directory of its own: the other stub tests link every object file of base
    os.makedirs(out, exist_ok=True)
    objs = []
    for unit, ext in (("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip")):
        o = os.path.join(out, "live_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host sides refer to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u", objs[1], objs[3]]).decode().split()
    known = open(os.path.join(base, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "live_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "live_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "live_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "live", "live_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    lib_objs = [p for p in sorted(glob.glob(os.path.join(base, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith("scan_")]
    exe = os.path.join(out, "kws_live_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(base, "fatbin_syms.o"), os.path.join(base, "hip_stub.o"), drv,
                                                                         "-ldl", "-lpthread"])
    return exe


def _run(exe, models):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in models], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    per = {}
    cur = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "model":
            cur = per.setdefault(os.path.basename(f[1]), {"rc": int(f[3]), "slicing": {}, "refuse": {}, "big": {}})
        elif f[0] == "slicing":
            cur["slicing"][int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "refuse":
            cur["refuse"][f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "big":
            cur["big"][int(f[1])] = (int(f[2]), int(f[3]))
        else:
            cur[f[0]] = tuple(int(x) for x in f[1:])
    return per


def test_live_host_logic_under_sanitizers(live_exe):
    per = _run(live_exe, SHIPPED)
    assert sorted(per) == sorted(SHIPPED)
    for name, r in per.items():
        assert r["rc"] == 0, name
        # a slicing is refused exactly when, and with the code with which, the scan (and so the stream API) refuses it
        for sl, (live_rc, scan_rc) in r["slicing"].items():
            assert live_rc == scan_rc, (name, sl, live_rc, scan_rc)
        assert r["slicing"][4000] == (0, 0)
        assert r["slicing"][4001][0] == -5 and r["slicing"][100][0] == -5 and r["slicing"][0][0] == -5
        assert r["create0"] == (-20,)
        # random chunkings: every push's counts are kws_live_window_count's, and per finished stream they sum to the scan's count
        pushes, mismatches, diff_streams, first_bad = r["chunked"]
        assert pushes == 360 and mismatches == 0 and diff_streams == 0 and first_bad == 0, (name, r["chunked"])
        for case in ("duplicate", "range", "nullstreams", "nulllengths", "nullcounts", "nullscores", "nullpcm", "nulloffsets", "nullsession",
                     "resetrange", "resetnull", "countrange", "countnull"):
            assert r["refuse"][case] == (-20, 1), (name, case, r["refuse"][case])
        assert r["refuse"]["zerolen"] == (0, 1) and r["refuse"]["empty"] == (0, 1)
        assert r["big"][0][0] == 0 and r["big"][0][1] > 5000, (name, r["big"])
        assert r["big"].get(1, (0, 0))[0] == 0, (name, r["big"])
