"""kws_scan_* without a GPU: the symbols are exported and bound, and the host side of the calls -- window counts, argument checks, the
stream API's slicing rules, the bookkeeping of a call that does work -- runs under ASan + UBSan against the stub HIP runtime of
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


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_scan_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert {"kws_scan_window_count", "kws_scan_recordings_device"} <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "kws_scan_window_count") and hasattr(lib, "kws_scan_recordings_device")
    assert callable(pkg.Model.scan_recordings_device) and callable(pkg.Model.scan_window_count)


@pytest.fixture(scope="module")
def scan_exe(host_exe):
    """tests/scan/scan_host_driver.cpp linked with the host objects host_exe built, plus the two scan units compiled the same way"""
    out = os.path.dirname(host_exe)
    objs = []
    for unit, ext in (("kws_scan", "cpp"), ("kws_scan_kernels", "hip")):
        o = os.path.join(out, "scan_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel unit's host side refers to its device code object: one dummy word (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u", objs[1]]).decode().split()
    known = open(os.path.join(out, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "scan_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "scan_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "scan_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "scan", "scan_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    lib_objs = [p for p in sorted(glob.glob(os.path.join(out, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith("scan_")]
    exe = os.path.join(out, "kws_scan_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(out, "fatbin_syms.o"), os.path.join(out, "hip_stub.o"), drv,
                                                                         "-ldl", "-lpthread"])
    return exe


def _run(exe, models):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in models], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    per = {}
    cur = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "model":
            cur = per.setdefault(os.path.basename(f[1]), {"rc": int(f[3]), "count": {}, "slicing": {}, "full": {}})
        elif f[0] == "count":
            cur["count"][int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "slicing":
            cur["slicing"][int(f[1])] = tuple(int(x) for x in f[2:])
        elif f[0] == "full":
            cur["full"][int(f[1])] = int(f[2])
        else:
            cur[f[0]] = tuple(int(x) for x in f[1:])
    return per


def test_scan_host_logic_under_sanitizers(scan_exe):
    per = _run(scan_exe, SHIPPED)
    assert sorted(per) == sorted(SHIPPED)
    for name, r in per.items():
        assert r["rc"] == 0, name
        # the stream rule with 4000-sample slices: nothing below 16 000 samples, then one window per slice from the fourth on
        for n, (w, rc) in r["count"].items():
            assert rc == 0 and w == (0 if n < 16000 else n // 4000 - 3), (name, n, w)
        # a slicing is refused exactly when, and with the code with which, the stream API refuses it
        for sl, (scan_rc, stream_rc, count_rc) in r["slicing"].items():
            assert scan_rc == stream_rc == count_rc, (name, sl, scan_rc, stream_rc, count_rc)
        assert r["slicing"][4000] == (0, 0, 0)
        assert r["slicing"][4001][0] == -5 and r["slicing"][100][0] == -5 and r["slicing"][0][0] == -5
        assert r["null"] == (-20,) and r["nullpcm"] == (-20,)
        assert r["empty"] == (0, 1) and r["short"] == (0, 1)
        assert r["full"][0] == 0 and r["full"].get(1, 0) == 0, name
