"""kws_slide_live_* without a GPU: the symbols are exported and bound, and the host side of the calls -- the path each flag gives at each
hop, window counts per push, argument checks, position arithmetic past 2^32 samples, the bookkeeping of pushes that do work on both
paths -- runs under ASan + UBSan against the stub HIP runtime of tests/sanitize (kernels do not run there)."""
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
SYMBOLS = {"kws_slide_live_create", "kws_slide_live_destroy", "kws_slide_live_path", "kws_slide_live_reset", "kws_slide_live_window_count",
           "kws_slide_live_push_device"}
AUTO, DIRECT, SHARED = 0, 1, 2


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_slide_live_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert callable(pkg.Model.slide_streams)
    for m in ("push_device", "window_count", "reset", "close"):
        assert callable(getattr(pkg.SlideStreams, m)), m
    assert isinstance(pkg.SlideStreams.path, property)


@pytest.fixture(scope="module")
def slide_live_exe(host_exe):
    """tests/slide_live/slide_live_host_driver.cpp linked with the host objects host_exe built, plus the slide and slide-live units (and the
    scan's kernel unit, whose count launch they share) compiled the same way"""
    base = os.path.dirname(host_exe)
    out = os.path.join(base, "slide_live")          # a directory of its own: the other stub tests link every object file of base
    os.makedirs(out, exist_ok=True)
    objs, kernel_objs = [], []
    for unit, ext in (("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_scan_kernels", "hip"), ("kws_slide_live", "cpp"),
                      ("kws_slide_live_kernels", "hip")):
        o = os.path.join(out, "sl_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
        if ext == "hip":
            kernel_objs.append(o)
    # the kernel units' host sides refer to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + kernel_objs).decode().split()
    known = open(os.path.join(base, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "sl_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "sl_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "slide_live_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv,
                                                                     os.path.join(ROOT, "tests", "slide_live", "slide_live_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_")                 # objects other host tests add to the same directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(base, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_slide_live_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(base, "fatbin_syms.o"), os.path.join(base, "hip_stub.o"), drv,
                                                                         "-ldl", "-lpthread"])
    return exe


def _run(exe, models):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in models], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    per = {}
    cur = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "model":
            cur = per.setdefault(os.path.basename(f[1]), {"rc": int(f[3]), "path": {}, "chunked": {}, "refuse": {}, "big": {}})
        elif f[0] == "geom":
            cur["geom"] = tuple(int(x) for x in f[1:])
        elif f[0] == "path":
            cur["path"][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
        elif f[0] == "chunked":
            cur["chunked"][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
        elif f[0] == "refuse":
            cur["refuse"][f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "big":
            cur["big"][int(f[1])] = tuple(int(x) for x in f[2:])
        else:
            raise AssertionError(line)
    return per


def test_slide_live_host_logic_under_sanitizers(slide_live_exe):
    per = _run(slide_live_exe, SHIPPED)
    assert sorted(per) == sorted(SHIPPED)
    for name, r in per.items():
        assert r["rc"] == 0, name
        stride, clip, nf = r["geom"]
        pre = 1                                                    # the shipped models' block is MFCC: frame 0 is per window
        hops = [stride, 2 * stride, 4000, 48 * stride, 49 * stride, 1000, 7, clip, clip + 13]
        for hop in hops:
            # the retained-row path serves the slide's phases == 1, touching case; AUTO takes it where it computes fewer rows per window
            served = hop % stride == 0 and hop // stride <= nf - pre
            auto = SHARED if served and hop // stride + pre < nf else DIRECT
            assert r["path"][(hop, AUTO)] == (0, auto), (name, hop, r["path"][(hop, AUTO)])
            assert r["path"][(hop, DIRECT)] == (0, DIRECT), (name, hop)
            assert r["path"][(hop, SHARED)] == ((0, SHARED) if served else (-20, 0)), (name, hop, r["path"][(hop, SHARED)])
            # random chunkings: every push's counts are kws_slide_live_window_count's, and per stream they sum to the slide's count
            for flags in (AUTO, DIRECT) + ((SHARED,) if served else ()):
                pushes, mismatches, diff_streams, first_bad = r["chunked"][(hop, flags)]
                assert pushes == 40 and mismatches == 0 and diff_streams == 0 and first_bad == 0, (name, hop, flags, r["chunked"][(hop, flags)])
            assert (hop, SHARED) in r["chunked"] or not served
        for case in ("create_s0", "create_sbig", "create_hop0", "create_hopbig", "create_flags", "create_flagsneg", "create_shared7", "create_shared49",
                     "create_nullout", "create_nullhandle", "duplicate", "range", "nullstreams", "nulllengths", "nullcounts", "nullscores", "nullpcm",
                     "nulloffsets", "nullsession", "toomany", "resetrange", "resetnull", "countrange", "countnull", "countmany"):
            assert r["refuse"][case] == (-20, 1), (name, case, r["refuse"][case])
        assert "create_left_a_session" not in r["refuse"]
        assert r["refuse"]["zerolen"] == (0, 1) and r["refuse"]["empty"] == (0, 1)
        # one stream past 2^32 samples, on the retained-row path (hop = stride) and at hop 4000 (the shipped strides: the direct path)
        for hop in (stride, 4000):
            path = SHARED if hop % stride == 0 and hop // stride + pre < nf else DIRECT
            rc, got_path, samples, windows, want = r["big"][hop]
            assert rc == 0 and got_path == path and samples > 2 ** 32 and windows == want == (samples - clip) // hop + 1, (name, hop, r["big"][hop])
