"""The banks' window pipelines without a GPU (kws_bank_scan_recordings_device, kws_bank_live_*, kws_bank_slide_live_*,
kws_bank_run_classifier_ragged_device): the symbols are exported, bound and declared, and the host side -- every refusal with its code and
without a launch, counts equal to the single-model functions', the front end launched once and the moving average once whatever K,
sessions and banks destroyed in both legal orders -- runs under ASan + UBSan against the stub HIP runtime of tests/sanitize (kernels do not
run there; its KWS_STUB_RECORD trace gives the launches of every bracketed call).  The driver links the bank's and the pipelines' units ON
TOP of the host objects host_exe built from the fixed unit list of tests/sanitize/Makefile, in a directory of its own; that the other host
tests (scan, live, slide, slide-live, ragged, bank) still link from their own fixed lists shows the link constraints of the runners."""
import collections
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
SYMBOLS = {"kws_bank_scan_recordings_device", "kws_bank_run_classifier_ragged_device",
           "kws_bank_live_create", "kws_bank_live_destroy", "kws_bank_live_reset", "kws_bank_live_window_count", "kws_bank_live_push_device",
           "kws_bank_slide_live_create", "kws_bank_slide_live_destroy", "kws_bank_slide_live_path", "kws_bank_slide_live_reset",
           "kws_bank_slide_live_window_count", "kws_bank_slide_live_push_device"}
UNITS = [("kws_bank", "cpp"), ("kws_bank_kernels", "hip"), ("kws_bank_windows", "cpp"), ("kws_bank_windows_kernels", "hip"),
         ("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip"),
         ("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_slide_live", "cpp"), ("kws_slide_live_kernels", "hip"),
         ("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")]
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
DRIVER_MODELS = MFCC40 + ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm"]
BANKS = {"mfcc40": 4, "l476": 2, "l476_reversed": 2, "l432_alone": 1}
BAD_ARGUMENT, DSP_ERROR = -20, -5
REFUSALS = {
    "scan_null_bank": BAD_ARGUMENT, "scan_null_scores": BAD_ARGUMENT, "scan_nothing_wanted": BAD_ARGUMENT, "scan_bad_slicing": DSP_ERROR,
    "scan_null_pcm": BAD_ARGUMENT,
    "live_create_slicing": DSP_ERROR, "live_create_s0": BAD_ARGUMENT, "live_create_null_bank": BAD_ARGUMENT,
    "live_push_null_member": BAD_ARGUMENT, "live_push_null_scores": BAD_ARGUMENT, "live_push_twice": BAD_ARGUMENT, "live_push_range": BAD_ARGUMENT,
    "live_push_null_counts": BAD_ARGUMENT, "live_push_null_session": BAD_ARGUMENT, "live_reset_range": BAD_ARGUMENT,
    "slide_create_hop0": BAD_ARGUMENT, "slide_create_flags": BAD_ARGUMENT, "slide_create_unserved": BAD_ARGUMENT, "slide_create_null_bank": BAD_ARGUMENT,
    "slide_push_nothing_wanted": BAD_ARGUMENT, "slide_push_null_scores": BAD_ARGUMENT, "slide_push_twice": BAD_ARGUMENT,
    "slide_push_null_session": BAD_ARGUMENT,
    "ragged_null_bank": BAD_ARGUMENT, "ragged_null_scores": BAD_ARGUMENT, "ragged_nothing_wanted": BAD_ARGUMENT, "ragged_no_frame": BAD_ARGUMENT,
    "ragged_too_long": BAD_ARGUMENT, "ragged_null_lengths": BAD_ARGUMENT, "ragged_huge_batch": BAD_ARGUMENT,
}
EMPTY = {"scan_r0", "scan_short", "live_push_n0", "live_push_zero_lengths", "slide_push_n0", "ragged_b0"}
# kernels behind the front end: the members' networks (the bank's own kernels and quantise pass among them) and the moving averages
BEHIND = ("kws_nn", "kws_bank_nn", "kws_quantize", "kws_bank_quantize", "kws_scan_maf", "kws_live_maf", "kws_bank_maf")


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_bank_window_symbols_are_exported_bound_and_declared():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    for method in ("scan_recordings_device", "live_streams", "slide_streams", "run_classifier_ragged_device"):
        assert callable(getattr(pkg.Bank, method)), method
    for m in ("push_device", "window_count", "reset", "close"):
        assert callable(getattr(pkg.BankLiveStreams, m)) and callable(getattr(pkg.BankSlideStreams, m)), m
    assert isinstance(pkg.BankSlideStreams.path, property)
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)
    assert "typedef struct kws_bank_live kws_bank_live;" in header and "typedef struct kws_bank_slide_live kws_bank_slide_live;" in header


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    """(stdout lines, {(bank, call): Counter of launched kernels by name without template arguments}) of one run of the driver"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_bank_windows_stub"))
    objs = []
    for unit, ext in UNITS:
        o = os.path.join(out, "bw_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + [o for o in objs if "kernels" in o]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "bw_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "bw_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "bank_windows_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv,
                                                                     os.path.join(ROOT, "tests", "bank_windows", "bank_windows_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_")          # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_bank_windows_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), os.path.join(lib_dir, "hip_stub.o"),
                                                                         drv, "-ldl", "-lpthread"])
    trace = os.path.join(out, "trace.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", KWS_STUB_RECORD=trace)
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in DRIVER_MODELS], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    launches, cur = {}, None
    for ln in open(trace):
        w = ln.split()
        if w[0] == "BEGIN":
            cur = launches.setdefault((w[1], w[2]), collections.Counter())
        elif w[0] == "END":
            cur = None
        elif w[0] == "launch" and cur is not None:
            name = ln.split(" | ", 1)[1].strip()
            name = name[5:] if name.startswith("void ") else name
            cur[name.split("<")[0].split("(")[0]] += 1
    return [ln.split() for ln in p.stdout.splitlines()], launches


def test_driver_ran_to_the_end_under_the_sanitizers(run):
    """every call that does work returns EI_IMPULSE_OK; sessions and banks were destroyed in both legal orders without a report (exit 0)"""
    lines, _ = run
    assert lines[-1] == ["done"]
    assert [ln for ln in lines if ln[0] == "load"] == [["load", str(i), "0"] for i in range(7)]
    for bank, K in BANKS.items():
        calls = {ln[2]: int(ln[3]) for ln in lines if ln[0] == "call" and ln[1] == bank}
        want = {"scan", "scan_in_place", "scan_single", "live_create", "live_push", "live_push_single", "ragged", "ragged_own_buffer", "ragged_features_only",
                "ragged_single", "live_push_member_fast", "mode_kept"} | {"slide_create_%d" % q for q in range(3)} | {"slide_push_%d" % q for q in range(3)} | \
               {"slide_push_%d_single" % q for q in range(3)} | ({"scan_skip0"} if K > 1 else set())
        assert set(calls) == want and all(rc == 0 for rc in calls.values()), (bank, calls)
        assert [ln[3:] for ln in lines if ln[0] == "nowindow" and ln[1] == bank] == [["0", "1"]], bank


def test_refusals_return_their_code_launch_nothing_and_change_nothing(run):
    lines, launches = run
    for bank in BANKS:
        refused = {ln[2]: (int(ln[3]), int(ln[4])) for ln in lines if ln[0] == "refuse" and ln[1] == bank}
        assert set(refused) == set(REFUSALS), (bank, set(refused) ^ set(REFUSALS))
        for name, code in REFUSALS.items():
            assert refused[name] == (code, 1), (bank, name, refused[name])             # the code; outputs, counts and mirrors untouched
            assert sum(launches[(bank, name)].values()) == 0, (bank, name, launches[(bank, name)])
        empty = {ln[2]: (int(ln[3]), int(ln[4])) for ln in lines if ln[0] == "empty" and ln[1] == bank}
        assert empty == {name: (0, 1) for name in EMPTY}, (bank, empty)
        assert all(sum(launches[(bank, name)].values()) == 0 for name in EMPTY), bank


def test_counts_are_the_single_model_functions(run):
    """every n_windows of every bank push and every kws_bank_*_window_count equal kws_live_window_count / kws_slide_live_window_count and the
    single-model pushes fed the same sequence (random subsets and lengths at the slicing's edges, finishes, a reset of two streams midway);
    the scan's windows are every member's kws_scan_window_count"""
    lines, _ = run
    for bank in BANKS:
        counts = {ln[2]: (int(ln[3]), int(ln[4])) for ln in lines if ln[0] == "counts" and ln[1] == bank}
        assert counts["scan"][0] > 0 and counts == {"scan": (counts["scan"][0], 0), "live": (120, 0), "slide_live_0": (60, 0), "slide_live_1": (60, 0), "slide_live_2": (60, 0)}, (bank, counts)


def test_front_end_once_and_one_moving_average_launch(run):
    """a bank call's launches in front of the networks are the single-model call's, kernel by kernel and count by count, whatever K; the
    continuous calls end in exactly one kws_bank_maf_kernel launch and in none of the single-model moving-average kernels"""
    _, launches = run
    pairs = [("scan", "scan_single"), ("scan_in_place", "scan_single"), ("live_push", "live_push_single"), ("ragged", "ragged_single"),
             ("ragged_own_buffer", "ragged_single")] + [("slide_push_%d" % q, "slide_push_%d_single" % q) for q in range(3)]
    for bank, K in BANKS.items():
        for name, single in pairs + ([("scan_skip0", "scan_single")] if K > 1 else []):
            got, ref = launches[(bank, name)], launches[(bank, single)]
            front = {k: v for k, v in ref.items() if not k.startswith(BEHIND)}
            assert front and {k: v for k, v in got.items() if not k.startswith(BEHIND)} == front, (bank, name, got, ref)
            assert any(k.startswith(("kws_nn", "kws_bank_nn")) for k in got), (bank, name, got)
        for name in ("scan", "scan_in_place", "live_push", "live_push_member_fast"):
            got = launches[(bank, name)]
            assert got["kws_bank_maf_kernel"] == 1 and got["kws_scan_maf_kernel"] == 0 and got["kws_live_maf_kernel"] == 0, (bank, name, got)
        assert launches[(bank, "scan_single")]["kws_scan_maf_kernel"] == 1 and launches[(bank, "live_push_single")]["kws_live_maf_kernel"] == 1
        # fast counters: no count kernel and no list reset in a bank call, a member in KWS_MODE_FAST included
        assert all(launches[(bank, name)]["kws_scan_count_kernel"] == 0 for name in ("scan", "live_push", "live_push_member_fast", "slide_push_0"))
        assert not any(k.startswith("kws_fast") for k in launches[(bank, "live_push_member_fast")]), bank
