"""MFE-block models at general DSP shapes without a GPU: which plans kws_create admits and refuses, what kws_mfcc_kernel_name reports, and which
kernels each batch call launches -- the tuned spectral kernel over chunks of frames or the cooperative kernel, the LDS or the global-memory
form of the normalisation -- read from the launch log of the stub HIP runtime (tests/ragged/ragged_hip_stub.cpp; kernels do not run there),
under ASan + UBSan.  The driver (tests/mfe_general/mfe_general_host_driver.cpp) links the host objects host_exe built."""
import glob
import os
import subprocess

import pytest

import mfe_general_shapes as G
from kws_testlib import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
UNSUPPORTED_MODEL, BAD_ARGUMENT = -18, -20
TAGS = sorted(G.SHAPES)
COLS = ("mfcc8", "mfcc", "coop", "scratch", "norm_tuned", "norm_lds", "centre", "scale", "quantise", "unring", "all")


def _tuned_kw():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import MFE_MODEL_KW
    return MFE_MODEL_KW


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_mfe_general_stub"))
    stub = os.path.join(out, "hip_stub_rec.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN +
                          ["-c", "-o", stub, os.path.join(ROOT, "tests", "ragged", "ragged_hip_stub.cpp")])
    drv = os.path.join(out, "driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "mfe_general", "mfe_general_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_")        # objects other host tests add to that directory
    objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_mfe_general_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + objs + [stub, drv, "-ldl", "-lpthread"])
    paths = [G.write_model(t, out) for t in TAGS] + [G.write_model("A", out, f32=True)]
    for name, kw in (("tuned", _tuned_kw()), ("radix7", G.RADIX7_KW), ("f24", G.FEW_FILTERS_KW)):
        p = os.path.join(out, name + ".kwsm")
        open(p, "wb").write(G.blob(kw))
        paths.append(p)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "done"
    names = TAGS + ["A_f32", "tuned", "radix7", "f24"]
    load = {names[int(ln.split()[1])]: (int(ln.split()[2]), ln.split(None, 3)[3]) for ln in lines if ln.startswith("load ")}
    route = {}
    for ln in lines:
        if ln.startswith("route "):
            w = ln.split()
            route[(names[int(w[1])], w[2])] = (int(w[3]), dict(zip(COLS, map(int, w[4:]))))
    fast = {names[int(ln.split()[1])]: (int(ln.split()[2]), ln.split(None, 3)[3] if len(ln.split(None, 3)) > 3 else "") for ln in lines if ln.startswith("fast ")}
    return load, route, fast


def test_plans_admitted_refused_and_named(run):
    load, _, fast = run
    for t in TAGS:
        assert load[t] == (0, G.SPECTRAL[t]), (t, load[t])
    assert load["A_f32"] == (0, G.SPECTRAL["A"])
    assert load["tuned"] == (0, "kws_mfcc8_kernel")                               # the tuned MFE model keeps its kernels
    assert load["radix7"][0] == UNSUPPORTED_MODEL and "radix" in load["radix7"][1]
    assert load["f24"][0] == UNSUPPORTED_MODEL and "32 filters" in load["f24"][1]       # a general MFE plan below 32 filters stays refused
    for t in TAGS + ["A_f32"]:                                                    # no fast mode for a general plan, with a reason
        assert fast[t][0] == UNSUPPORTED_MODEL and fast[t][1], (t, fast[t])
    assert fast["tuned"][0] == 0


@pytest.mark.parametrize("tag", TAGS + ["A_f32"])
def test_batch_calls_pick_the_route_of_the_shape(run, tag):
    _, route, _ = run
    shape = tag.split("_")[0]
    chunked, lds = G.SPECTRAL[shape].startswith("kws_mfcc8"), G.NORM_LDS[shape]
    n_chunks = 2 if shape == "A" else 1

    def spectral(r, aligned=True):
        if chunked and aligned:
            return r["mfcc8"] == n_chunks and r["coop"] == 0 and r["scratch"] == 0 and r["mfcc"] == 0
        return r["coop"] == 1 and r["mfcc8"] == 0 and r["scratch"] == 0 and r["mfcc"] == 0

    def norm(r):
        return r["norm_tuned"] == 0 and r["quantise"] == 0 and (r["norm_lds"], r["centre"], r["scale"]) == ((1, 0, 0) if lds else (0, 1, 1))
    for call in ("classify", "extract_mfe"):
        rc, r = route[(tag, call)]
        assert rc == 0 and spectral(r) and norm(r), (tag, call, r)
    rc, r = route[(tag, "classify_unaligned")]                                   # a general plan has no alignment rule: the cooperative kernel
    assert rc == 0 and spectral(r, aligned=False) and norm(r), (tag, r)
    rc, r = route[(tag, "mfe")]
    assert rc == 0 and spectral(r) and r["norm_lds"] + r["centre"] + r["scale"] + r["norm_tuned"] == 0, (tag, r)
    rc, r = route[(tag, "cmvn_inference")]                                       # the normalisation of a COPY, then the network
    assert rc == 0 and r["unring"] == 1 and norm(r) and r["mfcc8"] + r["coop"] == 0, (tag, r)
    # the whole block: spectral launch(es), the normalisation (the int8 tensor in the same pass), the network
    rc, r = route[(tag, "classify")]
    assert r["all"] == n_chunks * chunked + (not chunked) + (1 if lds else 2) + 1, (tag, r)


def test_tuned_mfe_model_keeps_its_launches(run):
    _, route, _ = run
    rc, r = route[("tuned", "classify")]
    assert rc == 0 and r["mfcc8"] == 1 and r["norm_tuned"] == 1 and r["quantise"] == 1 and r["norm_lds"] + r["centre"] + r["scale"] + r["coop"] == 0, r
    assert route[("tuned", "classify_unaligned")][0] == BAD_ARGUMENT
    rc, r = route[("tuned", "extract_mfe")]
    assert rc == 0 and r["mfcc8"] == 1 and r["norm_tuned"] == 1 and r["all"] == 2, r
