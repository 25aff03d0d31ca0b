"""kws_slide_* without a GPU: the symbols are exported and bound, and the host side of the calls -- window counts, the plan's row
arithmetic against a brute-force count of the frame positions the windows need, argument checks, the bookkeeping of calls that do
work on every path -- runs under ASan + UBSan against the stub HIP runtime of tests/sanitize (kernels do not run there)."""
import ctypes
import glob
import math
import os
import subprocess

import pytest

from kws_testlib import MODELS, ROOT, synth_model_blob
from slide_testlib import MFE_KW, brute_force_rows

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
# the flags of tests/sanitize/Makefile's host-only build of the library
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
SHIPPED = ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm", "cfg2_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
SLIDE_SYMBOLS = {"kws_frame_stride_samples", "kws_slide_window_count", "kws_slide_plan", "kws_slide_recordings_device"}
AUTO, DIRECT, SHARED = 0, 1, 2


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_slide_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert SLIDE_SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SLIDE_SYMBOLS)
    assert callable(pkg.Model.slide_recordings_device) and callable(pkg.Model.slide_window_count) and callable(pkg.Model.slide_plan)
    assert isinstance(pkg.Model.frame_stride_samples, property)
    assert (pkg.SLIDE_AUTO, pkg.SLIDE_DIRECT, pkg.SLIDE_SHARED) == (AUTO, DIRECT, SHARED)
    assert ctypes.sizeof(pkg.SlidePlanInfo) == 4 * ctypes.sizeof(ctypes.c_size_t) + 8


@pytest.fixture(scope="module")
def slide_exe(host_exe):
    """tests/slide/slide_host_driver.cpp linked with the host objects host_exe built, plus the slide units (and the scan's kernel unit, whose
    count launch the slide calls share) compiled the same way"""
    out = os.path.dirname(host_exe)
    objs = []
    for unit, ext in (("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_scan_kernels", "hip")):
        o = os.path.join(out, "slide_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + objs[1:]).decode().split()
    known = open(os.path.join(out, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "slide_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "slide_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "slide_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "slide", "slide_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_")                 # objects other host tests add to the same directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(out, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_slide_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(out, "fatbin_syms.o"), os.path.join(out, "hip_stub.o"), drv,
                                                                         "-ldl", "-lpthread"])
    return exe


def _run(exe, paths):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    per = {}
    cur = None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "model":
            cur = per.setdefault(os.path.basename(f[1]), {"rc": int(f[3]), "count": {}, "plan": {}, "full": {}})
        elif f[0] == "count":
            cur["count"][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
        elif f[0] == "plan":
            cur["plan"][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
        elif f[0] == "full":
            cur["full"][(int(f[1]), int(f[2]), int(f[3]))] = int(f[4])
        else:
            cur[f[0]] = tuple(int(x) for x in f[1:])
    return per


def test_slide_host_logic_under_sanitizers(slide_exe, tmp_path):
    mfe = str(tmp_path / "mfe.kwsm")
    open(mfe, "wb").write(synth_model_blob(**MFE_KW))
    per = _run(slide_exe, [os.path.join(MODELS, m) for m in SHIPPED] + [mfe])
    assert sorted(per) == sorted(SHIPPED + ["mfe.kwsm"])
    for name, r in per.items():
        assert r["rc"] == 0, name
        clip, nf, stride = r["geom"]
        pre = 0 if name == "mfe.kwsm" else 1
        assert (clip, nf, stride) == (16000, 49, 320), name
        hops = sorted({hop for _, hop in r["count"]})
        assert hops == sorted({stride, 2 * stride, 4000, 1000, 7, 1, clip, clip + 13})
        lens = sorted({n for n, _ in r["count"]})
        for (n, hop), (w, rc) in r["count"].items():
            assert rc == 0 and w == (0 if n < clip else (n - clip) // hop + 1), (name, n, hop, w)
        for (hop, flags), (rc, n_win, shared, first, direct, phases, path) in r["plan"].items():
            assert rc == 0, (name, hop, flags)
            W = [r["count"][(n, hop)][0] for n in lens]
            assert n_win == sum(W) and direct == n_win * nf and first == (n_win if pre else 0), (name, hop, flags)
            assert phases == stride // math.gcd(hop, stride), (name, hop)
            # every frame position the windows need, counted once per recording: exactly what the shared path computes
            assert shared == sum(brute_force_rows(w, hop, stride, nf, pre) for w in W), (name, hop, shared)
            want = SHARED if shared + first < direct else DIRECT
            assert path == (want if flags == AUTO else flags), (name, hop, flags, path)
        assert {hop: r["plan"][(hop, AUTO)][5] for hop in (stride, 2 * stride, 4000, 1000, 7, 1)} == {320: 1, 640: 1, 4000: 2, 1000: 8, 7: 320, 1: 320}
        assert r["plan"][(stride, AUTO)][6] == SHARED and r["plan"][(clip, AUTO)][6] == DIRECT and r["plan"][(clip + 13, AUTO)][6] == DIRECT
        # at hop = stride a window costs one new shared row (+ its frame 0) once the first window's rows exist
        rc, n_win, shared, first, direct, _, _ = r["plan"][(stride, AUTO)]
        n_rec = sum(1 for n in lens if n >= clip)
        assert shared == n_win - n_rec + n_rec * (nf - pre)
        assert r["hop0"] == (-20, -20, -20) and r["nullscores"] == (-20,) and r["badflags"] == (-20, -20, -20) and r["nullpcm"] == (-20,)
        assert r["hugelen"] == (-20, -20, -20) and r["hugehop"] == (-20,) and r["hugecount"] == (-20,)
        assert r["empty"] == (0, 1) and r["short"] == (0, 1)
        # the calls that do work: every path at every hop in exact mode (and in fast mode where the model has one)
        assert {k[1:] for k in r["full"] if k[0] == 0} == {(f, hop) for f in (AUTO, DIRECT, SHARED) for hop in hops if hop >= 100 or f == SHARED}, name
        assert all(rc == 0 for rc in r["full"].values()), (name, r["full"])
