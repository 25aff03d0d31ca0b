"""kws_bank_* without a GPU: the symbols are exported and bound, and the host side -- membership rules, argument checks, the bookkeeping of
the three calls on every slide path, banks destroyed before their members -- runs under ASan + UBSan against the stub HIP runtime of
tests/sanitize (kernels do not run there).  The driver links the new units ON TOP of the host objects host_exe built from the fixed unit
list of tests/sanitize/Makefile: that the other host tests (scan, slide, live) still link from their own fixed lists shows that no
existing unit came to depend on the bank's."""
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
BANK_SYMBOLS = {"kws_bank_create", "kws_bank_destroy", "kws_bank_size", "kws_bank_member", "kws_bank_run_classifier_batch_device",
                "kws_bank_cmvn_inference_batch_device", "kws_bank_slide_recordings_device"}
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
DRIVER_MODELS = MFCC40 + ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm"]
BANKS = {"mfcc40": 4, "l476": 2, "l476_reversed": 2, "l432_alone": 1}
BAD_ARGUMENT = -20


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_bank_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert BANK_SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in BANK_SYMBOLS)
    for method in ("run_classifier_batch_device", "cmvn_inference_batch_device", "slide_recordings_device", "close"):
        assert callable(getattr(pkg.Bank, method)), method
    assert isinstance(pkg.Bank.members, property)
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in BANK_SYMBOLS)


@pytest.fixture(scope="module")
def bank_exe(host_exe, tmp_path_factory):
    """tests/bank/bank_host_driver.cpp linked with the host objects host_exe built, plus the bank's units and the pipelines' (the bank's slide
    lives in kws_bank_windows.cpp beside its routed form, and that unit names every pipeline's runner) compiled the same way: the unit list
    of tests/test_bank_windows_host.py.  What this adds goes to a directory of its own: the other host tests link every object they find
    next to host_exe."""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_bank_stub"))
    objs = []
    for unit, ext in (("kws_bank", "cpp"), ("kws_bank_kernels", "hip"), ("kws_bank_windows", "cpp"), ("kws_bank_windows_kernels", "hip"),
                      ("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip"),
                      ("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_slide_live", "cpp"), ("kws_slide_live_kernels", "hip"),
                      ("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")):
        o = os.path.join(out, "bank_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + [o for o in objs if "kernels" in o]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "bank_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "bank_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "bank_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "bank", "bank_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_")                 # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_bank_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), os.path.join(lib_dir, "hip_stub.o"),
                                                                         drv, "-ldl", "-lpthread"])
    return exe


def test_existing_units_do_not_depend_on_the_bank(host_exe):
    """the fixed unit list of tests/sanitize/Makefile linked without the bank's units (host_exe exists), and none of its objects refers to them"""
    out = os.path.dirname(host_exe)
    objs = [p for p in glob.glob(os.path.join(out, "kws_*.o"))]
    assert objs
    undefined = subprocess.check_output(["nm", "-u"] + objs).decode()
    assert "kws_bank" not in undefined and "kws_launch_bank" not in undefined


def test_bank_host_logic_under_sanitizers(bank_exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([bank_exe] + [os.path.join(MODELS, m) for m in DRIVER_MODELS], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln.split(None, 4) for ln in p.stdout.splitlines()]
    assert lines[-1] == ["done"]
    assert [ln for ln in lines if ln[0] == "load"] == [["load", str(i), "0"] for i in range(7)]
    # creation: the four 49x40 models, the l476 pair in either order, a bank of one -- members come back in the caller's order
    created = {ln[1]: ln[2:] for ln in lines if ln[0] == "create"}
    assert created == {name: ["0", str(k), "1"] for name, k in BANKS.items()}
    # refusals: the stated code, *out left NULL, and a message that names what is wrong
    refused = {ln[1]: (int(ln[2]), int(ln[3]), ln[4]) for ln in lines if ln[0] == "refuse"}
    assert set(refused) == {"l476_l432", "k0", "k17", "null_member", "twice", "mfcc40_l476", "null_out", "null_members"}
    for name, (rc, out_null, msg) in refused.items():
        assert rc == BAD_ARGUMENT and out_null == 1, (name, rc, out_null)
    assert "high_frequency" in refused["l476_l432"][2] and "member 1" in refused["l476_l432"][2]
    assert "num_cepstral" in refused["mfcc40_l476"][2]
    assert "17" in refused["k17"][2] and "0" in refused["k0"][2]
    assert "member 1 is NULL" in refused["null_member"][2]
    assert "0 and 2" in refused["twice"][2]
    assert {ln[1]: ln[2] for ln in lines if ln[0] == "usable"} == {"l476": "0", "l476_f32": "0", "l432": "0"}
    for bank in BANKS:
        args = {ln[2]: int(ln[3]) for ln in lines if ln[0] == "args" and ln[1] == bank}
        assert len(args) == 15 and all(rc == BAD_ARGUMENT for rc in args.values()), (bank, args)
        empty = {ln[2]: ln[3:] for ln in lines if ln[0] == "empty" and ln[1] == bank}
        assert empty == {k: ["0", "1"] for k in ("batch0", "cmvn0", "slide_r0", "slide_short")}, (bank, empty)
        calls = {ln[2]: int(ln[3]) for ln in lines if ln[0] == "call" and ln[1] == bank}
        assert len(calls) == 8 and all(rc == 0 for rc in calls.values()), (bank, calls)
        slides = {(int(ln[2]), int(ln[3])): int(ln[4]) for ln in lines if ln[0] == "slide" and ln[1] == bank}
        assert set(slides) == {(f, hop) for f in (0, 1, 2) for hop in (320, 1600, 1000, 16013)} and all(rc == 0 for rc in slides.values()), (bank, slides)
    assert ["size_null", "0"] in lines
