"""The shapes of tests/general_dsp_shapes.py without a GPU: which plans kws_create admits and refuses (with the refusal's text), what
kws_mfcc_kernel_name reports, and which kernels each batch call launches -- the cooperative kernel (and which of its two builds, with or
without pair loads), the scratch kernel or the tuned spectral kernel over chunks; the LDS or the global-memory form of cmvnw -- read from the
launch log of the stub HIP runtime (tests/ragged/ragged_hip_stub.cpp; kernels do not run there), under ASan + UBSan.  The driver
(tests/general_dsp/general_dsp_host_driver.cpp) links the host objects host_exe built."""
import glob
import os
import subprocess

import pytest

import general_dsp_shapes as G
from kws_testlib import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
UNSUPPORTED_MODEL = -18
COLS = ("mfcc8", "coop", "coop_w2", "coop_w4", "coop_pairs", "scratch", "cmvn_nn", "cmvn_lds", "cmvn_global", "all")
REFUSED = sorted(G.REFUSED)


HOST_FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off", "-DKWS_BUILDING_LIBRARY",
              "-Wno-unused-value"]             # tests/sanitize/Makefile's, for the one unit this test compiles a second time


def _drive(exe, out, names, **switches):
    paths = [G.write_model(n, out) for n in names]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1", **switches)
    p = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "done"
    load = {names[int(ln.split()[1])]: (int(ln.split()[2]), ln.split(None, 3)[3]) for ln in lines if ln.startswith("load ")}
    route = {}
    for ln in lines:
        if ln.startswith("route "):
            w = ln.split()
            assert len(w) == 4 + len(COLS), ln
            route[(names[int(w[1])], w[2])] = (int(w[3]), dict(zip(COLS, map(int, w[4:]))))
    fast = {names[int(ln.split()[1])]: (int(ln.split()[2]), ln.split(None, 3)[3] if len(ln.split(None, 3)) > 3 else "") for ln in lines if ln.startswith("fast ")}
    return load, route, fast


@pytest.fixture(scope="module")
def build(host_exe, tmp_path_factory):
    """(the driver on the product sources, the same with kws_generic.hip compiled -DKWS_DEV_SWITCHES -- the build that reads KWS_DEV_GENERIC_SCRATCH /
    KWS_DEV_CMVN_GLOBAL --, the scratch directory)"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_general_envelope_stub"))
    stub = os.path.join(out, "hip_stub_rec.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN +
                          ["-c", "-o", stub, os.path.join(ROOT, "tests", "ragged", "ragged_hip_stub.cpp")])
    drv = os.path.join(out, "driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "general_dsp", "general_dsp_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_")        # objects other host tests add to that directory
    objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_general_dsp_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + objs + [stub, drv, "-ldl", "-lpthread"])
    # the development build of the one unit that reads the two switches; its device code object's dummy word as tests/sanitize/Makefile makes them
    gen = os.path.join(out, "kws_generic_dev.o")
    subprocess.check_call([CLANG] + HOST_FLAGS + SAN + ["-DKWS_DEV_SWITCHES", "-c", "-o", gen, os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc", "kws_generic.hip")])
    rest = [p for p in objs if os.path.basename(p) not in ("kws_generic.o", "fatbin_syms.o")]
    undefined = subprocess.check_output(["nm", "-u", gen] + rest, text=True)
    syms = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin_")})
    with open(os.path.join(out, "fatbin_syms_dev.c"), "w") as f:
        f.write("".join("const unsigned long long %s = 0;\n" % s for s in syms))
    syms_o = os.path.join(out, "fatbin_syms_dev.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", syms_o, os.path.join(out, "fatbin_syms_dev.c")])
    exe_dev = os.path.join(out, "kws_general_dsp_san_dev")
    subprocess.check_call([CLANG] + SAN + ["-o", exe_dev] + rest + [gen, syms_o, stub, drv, "-ldl", "-lpthread"])
    return exe, exe_dev, out


@pytest.fixture(scope="module")
def run(build):
    exe, _, out = build
    return _drive(exe, out, G.NAMES + REFUSED)


@pytest.mark.parametrize("name", G.NAMES)
def test_served_shape_is_admitted_named_and_has_no_fast_mode(run, name):
    load, _, fast = run
    assert load[name] == (0, G.SERVED[name][1]), (name, load[name])
    assert fast[name][0] == UNSUPPORTED_MODEL and fast[name][1], (name, fast[name])     # no fast mode for a general plan, with a reason


@pytest.mark.parametrize("name", REFUSED)
def test_refused_shape_says_why(run, name):
    load, route, _ = run
    assert load[name][0] == UNSUPPORTED_MODEL and G.REFUSED[name][1] in load[name][1], (name, load[name])
    assert not [k for k in route if k[0] == name]


@pytest.mark.parametrize("name", G.NAMES)
def test_batch_calls_pick_the_route_of_the_shape(run, name):
    _, route, _ = run
    _, kernel, lds = G.SERVED[name]

    def spectral(r):
        if kernel == G.CHUNKED:                     # 49 frames: one chunk on the tuned kernel
            return (r["mfcc8"], r["coop"], r["scratch"]) == (1, 0, 0)
        if kernel == G.SCRATCH:
            return (r["mfcc8"], r["coop"], r["scratch"]) == (0, 0, 1)
        ok = (r["mfcc8"], r["coop"], r["scratch"]) == (0, 1, 0) and r["coop_w2"] + r["coop_w4"] == 1          # one build or the other, by its name
        ok = ok and r["coop_pairs"] == (0 if name in G.NO_PAIRS else 1)
        return ok and (r["coop_w2"] == 1 or name not in G.TWO_WAVE)

    def norm(r):
        return r["cmvn_nn"] == 0 and (r["cmvn_lds"], r["cmvn_global"]) == ((1, 0) if lds else (0, 1))
    for call in ("classify", "extract_mfcc"):
        rc, r = route[(name, call)]
        assert rc == 0 and spectral(r) and norm(r), (name, call, r)
    rc, r = route[(name, "mfcc")]                                                # the cepstra before cmvnw: the spectral launch alone
    assert rc == 0 and spectral(r) and r["cmvn_lds"] + r["cmvn_global"] + r["cmvn_nn"] == 0 and r["all"] == 1, (name, r)
    rc, r = route[(name, "cmvn_inference")]
    assert rc == 0 and norm(r) and r["mfcc8"] + r["coop"] + r["scratch"] == 0, (name, r)
    rc, r = route[(name, "classify")]                                            # the whole block: spectral, cmvnw (the int8 tensor in the same pass), the network
    assert r["all"] == 3, (name, r)


def test_every_route_has_a_shape(run):
    """cooperative kernel in its two-wave and its four-wave build, with and without pair loads; the scratch kernel; the tuned kernel over
    chunks; cmvnw in LDS and in global memory -- each reached by at least one shape of the table through a plain batch call."""
    _, route, _ = run
    seen = set()
    for name in G.NAMES:
        r = route[(name, "classify")][1]
        seen |= {k for k in ("mfcc8", "coop_w2", "coop_w4", "coop_pairs", "scratch", "cmvn_lds", "cmvn_global") if r[k]}
        if r["coop"] and not r["coop_pairs"]:
            seen.add("coop_samples")
    assert seen == {"mfcc8", "coop_w2", "coop_w4", "coop_pairs", "coop_samples", "scratch", "cmvn_lds", "cmvn_global"}, seen


def test_development_switches_force_the_scratch_kernel_and_the_global_cmvnw(build):
    """KWS_DEV_GENERIC_SCRATCH / KWS_DEV_CMVN_GLOBAL (read once per process, by the development build only) put small shapes on the forms the
    library otherwise keeps for fft 4096 and for matrices beyond 64 KB: what tests/general_envelope_worker.py then runs on the GPU really is
    the other form.  The product build ignores both (test_batch_calls_pick_the_route_of_the_shape ran without them; here: with them set)."""
    exe, exe_dev, out = build
    load, route, _ = _drive(exe_dev, out, list(G.FORCED_SCRATCH), KWS_DEV_GENERIC_SCRATCH="1")
    for name in G.FORCED_SCRATCH:
        assert G.SERVED[name][1] == G.LDS and load[name] == (0, G.SCRATCH), (name, load[name])
        for call in ("classify", "extract_mfcc", "mfcc"):
            rc, r = route[(name, call)]
            assert rc == 0 and (r["scratch"], r["coop"], r["mfcc8"]) == (1, 0, 0), (name, call, r)
    load, route, _ = _drive(exe_dev, out, list(G.FORCED_CMVN_GLOBAL), KWS_DEV_CMVN_GLOBAL="1")
    for name in G.FORCED_CMVN_GLOBAL:
        assert load[name] == (0, G.SERVED[name][1]), (name, load[name])
        for call in ("classify", "extract_mfcc", "cmvn_inference"):
            rc, r = route[(name, call)]
            assert rc == 0 and (r["cmvn_lds"], r["cmvn_global"], r["cmvn_nn"]) == (0, 1, 0), (name, call, r)
    assert any(G.SERVED[name][2] for name in G.FORCED_CMVN_GLOBAL)               # (at least one of them is in LDS when left alone)
    load, route, _ = _drive(exe, out, ["fft96", "win3"], KWS_DEV_GENERIC_SCRATCH="1", KWS_DEV_CMVN_GLOBAL="1")
    assert load["fft96"] == (0, G.LDS) and route[("fft96", "classify")][1]["coop"] == 1 and route[("win3", "classify")][1]["cmvn_lds"] == 1
