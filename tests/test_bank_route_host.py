"""Routed bank calls without a GPU (kws_bank_run_classifier_routed_device, kws_bank_run_classifier_ragged_routed_device,
kws_bank_live_route, kws_bank_slide_live_route): the symbols are exported, bound and declared, and the host side -- every refusal with its
code and without a launch, NULL and all-member routes launching exactly what the unrouted call launches, one-hot routes launching the front
end once, one matrix-core launch per row width with a non-empty member, nothing for a member nobody names and one moving average whatever
K, and the list building against a restatement in Python -- runs under ASan + UBSan against the stub HIP runtime of tests/sanitize (kernels
do not run there; its KWS_STUB_RECORD trace gives the launches of every bracketed call).  The driver links the bank's and the pipelines'
units ON TOP of the host objects host_exe built from the fixed unit list of tests/sanitize/Makefile, as tests/test_bank_windows_host.py does,
with that test's unit list: the routed launchers live in the bank's existing kernel units."""
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
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
SYMBOLS = {"kws_bank_run_classifier_routed_device", "kws_bank_run_classifier_ragged_routed_device", "kws_bank_live_route",
           "kws_bank_slide_live_route"}
UNITS = [("kws_bank", "cpp"), ("kws_bank_kernels", "hip"), ("kws_bank_windows", "cpp"), ("kws_bank_windows_kernels", "hip"),
         ("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip"),
         ("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_slide_live", "cpp"), ("kws_slide_live_kernels", "hip"),
         ("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")]
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
DRIVER_MODELS = MFCC40 + ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm"]
BANKS = {"mfcc40": 4, "l476": 2, "l432_alone": 1}
BAD_ARGUMENT = -20
REFUSALS = {"routed_bad_bit", "routed_null_bank", "routed_null_pcm", "routed_null_scores",
            "ragged_routed_bad_bit", "ragged_routed_null_bank", "ragged_routed_null_scores", "ragged_routed_null_pcm",
            "live_route_pushed", "live_route_range", "live_route_bad_bit", "live_route_null_session", "live_route_null_routes",
            "slide_route_range", "slide_route_bad_bit", "slide_route_null_session"}
REFUSALS_MULTI = {"live_push_needed_null"}              # (a bank of one has no member a routed stream could leave out and still need)
# kernels behind the front end: the members' networks (the bank's own kernels and quantise passes among them) and the moving averages
BEHIND = ("kws_nn", "kws_dense", "kws_bank_nn", "kws_quantize", "kws_bank_quantize", "kws_scan_maf", "kws_live_maf", "kws_bank_maf")
# every routed call against the unrouted call whose trace it must repeat
SAME_AS_UNROUTED = [("batch_null_routes", "batch_unrouted"), ("batch_all_routes", "batch_unrouted"), ("ragged_null_routes", "ragged_unrouted"),
                    ("ragged_all_routes", "ragged_unrouted"), ("live_push_all_routes", "live_push_fresh"), ("slide_push_all_routes", "slide_push_fresh")]
ONE_HOT = [("batch_onehot", "batch_unrouted"), ("ragged_onehot", "ragged_unrouted"), ("live_push_onehot", "live_push_fresh"),
           ("slide_push_onehot", "slide_push_fresh")]


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_routed_symbols_are_exported_bound_and_declared():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert callable(pkg.Bank.run_classifier_routed_device)
    import inspect
    assert inspect.signature(pkg.Bank.run_classifier_ragged_device).parameters["routes"].default is None
    assert callable(pkg.BankLiveStreams.route) and callable(pkg.BankSlideStreams.route)
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    """(stdout lines, {(bank, call): Counter of launched kernels by name without template arguments}) of one run of the driver"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_bank_route_stub"))
    objs = []
    for unit, ext in UNITS:
        o = os.path.join(out, "br_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + [o for o in objs if "kernels" in o]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "br_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "br_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "bank_route_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "bank_route", "bank_route_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_")          # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_bank_route_san")
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
    return p.stdout.splitlines(), launches


def test_driver_ran_to_the_end_under_the_sanitizers(run):
    """every call that does work returns EI_IMPULSE_OK; nothing the sanitizers report (exit 0)"""
    lines, launches = run
    assert lines[-1] == "done"
    for bank, K in BANKS.items():
        calls = {ln.split()[2]: int(ln.split()[3]) for ln in lines if ln.startswith("call " + bank + " ")}
        assert calls and all(rc == 0 for rc in calls.values()), (bank, calls)
        want = {a for pair in SAME_AS_UNROUTED + ONE_HOT for a in pair} | {"slide_push_rerouted", "batch_first_only", "batch_last_only", "batch_none", "batch_b0", "live_push_unrouted_stream",
                                                                           "live_route_after_reset", "slide_route_change"}
        assert want | ({"live_push_only_needed"} if K > 1 else set()) <= set(calls), (bank, calls)


def test_refusals_return_their_code_launch_nothing_and_change_nothing(run):
    lines, launches = run
    for bank, K in BANKS.items():
        refused = {}
        for ln in lines:
            if ln.startswith("refuse " + bank + " "):
                head, msg = ln.split(" | ", 1)
                w = head.split()
                refused[w[2]] = (int(w[3]), int(w[4]), msg)
        want = REFUSALS | (REFUSALS_MULTI if K > 1 else set())
        assert set(refused) == want, (bank, set(refused) ^ want)
        for name in want:
            assert refused[name][:2] == (BAD_ARGUMENT, 1), (bank, name, refused[name])       # the code; outputs, counts and routes untouched
            assert sum(launches[(bank, name)].values()) == 0, (bank, name, launches[(bank, name)])
        # kws_last_error names the FIRST offending index and its mask
        assert "clip 3:" in refused["routed_bad_bit"][2] and "0x%x" % ((1 << K) - 1 | 1 << K) in refused["routed_bad_bit"][2], refused["routed_bad_bit"]
        assert "clip 4:" in refused["ragged_routed_bad_bit"][2] and "0x%x" % (1 << K) in refused["ragged_routed_bad_bit"][2], refused["ragged_routed_bad_bit"]
        assert "entry 1: stream 0 " in refused["live_route_pushed"][2], refused["live_route_pushed"]
        assert "0x%x" % (1 << K) in refused["live_route_bad_bit"][2] and "0x%x" % (1 << K) in refused["slide_route_bad_bit"][2]
        # a call without clips, and routes that name nobody: no network, and for the latter the front end alone
        assert sum(launches[(bank, "batch_b0")].values()) == 0
        none = launches[(bank, "batch_none")]
        assert none and not any(k.startswith(BEHIND) for k in none), (bank, none)
        assert {k: v for k, v in launches[(bank, "batch_unrouted")].items() if not k.startswith(BEHIND)} == dict(none), (bank, none)


def test_null_and_all_member_routes_launch_what_the_unrouted_call_launches(run):
    """the same kernels by name, the same counts: such a call IS the unrouted call; a session whose routes were all set to every member
    pushes like one that was never routed"""
    _, launches = run
    for bank in BANKS:
        for name, ref in SAME_AS_UNROUTED:
            assert launches[(bank, ref)] and launches[(bank, name)] == launches[(bank, ref)], (bank, name, launches[(bank, name)], launches[(bank, ref)])
            assert not any("routed" in k for k in launches[(bank, name)]), (bank, name)


def test_one_hot_routes_front_end_once_one_launch_per_row_width_and_one_moving_average(run):
    _, launches = run
    for bank, K in BANKS.items():
        if K == 1:
            # one member: one-hot routes name every member, the unrouted launches
            assert all(launches[(bank, name)] == launches[(bank, ref)] for name, ref in ONE_HOT), bank
            continue
        for name, ref in ONE_HOT:
            got, unrouted = launches[(bank, name)], launches[(bank, ref)]
            front = {k: v for k, v in unrouted.items() if not k.startswith(BEHIND)}
            assert front and {k: v for k, v in got.items() if not k.startswith(BEHIND)} == front, (bank, name, got, unrouted)
            # both banks hold int8 matrix-core members of ONE row width (64 bytes at 49x40, 16 at 49x13): one launch for them, none of the unrouted form
            assert got["kws_bank_nn_mfma_routed_kernel"] == 1 and got["kws_bank_nn_mfma_kernel"] == 0, (bank, name, got)
            assert got["kws_bank_quantize_kernel"] == 0 and got["kws_bank_quantize_routed_kernel"] == (1 if bank == "mfcc40" else 0), (bank, name, got)
            # the members that run their own launches run what they run in the unrouted call, launch for launch, over their lists
            own = lambda c: {k: v for k, v in c.items() if k.startswith(("kws_nn", "kws_dense"))}
            if name in ("batch_onehot", "ragged_onehot"):        # (the pushes name three streams: three of mfcc40's four members)
                assert own(got) == own(unrouted), (bank, name, got, unrouted)
        # a route changed between two pushes holds from the next push on: streams 4, 1, 2 then name members 1, 2, 3 of four (no matrix-core
        # member among them) / members 1, 0, 1 of two
        moved = launches[(bank, "slide_push_rerouted")]
        assert moved["kws_bank_nn_mfma_routed_kernel"] == (0 if bank == "mfcc40" else 1) and moved["kws_bank_nn_mfma_kernel"] == 0, (bank, moved)
        assert moved["kws_bank_quantize_routed_kernel"] == (1 if bank == "mfcc40" else 0), (bank, moved)
        live = launches[(bank, "live_push_onehot")]
        assert live["kws_bank_maf_routed_kernel"] == 1 and live["kws_bank_maf_kernel"] == 0 and live["kws_live_maf_kernel"] == 0, (bank, live)
        assert launches[(bank, "live_push_fresh")]["kws_bank_maf_kernel"] == 1 and launches[(bank, "live_push_fresh")]["kws_bank_maf_routed_kernel"] == 0
        # a member with an empty list contributes no launch: only the first member (int8, matrix-core shape) / only the last (float32)
        first, last = launches[(bank, "batch_first_only")], launches[(bank, "batch_last_only")]
        assert {k: v for k, v in first.items() if k.startswith(BEHIND)} == {"kws_bank_nn_mfma_routed_kernel": 1}, (bank, first)
        behind_last = {k: v for k, v in last.items() if k.startswith(BEHIND)}
        assert behind_last and all(k.startswith("kws_nn_f32") for k in behind_last), (bank, last)
        # a pushed stream that names nobody: no network at all
        lone = launches[(bank, "live_push_unrouted_stream")]
        assert not any(k.startswith(("kws_nn", "kws_dense", "kws_bank_nn", "kws_bank_quantize")) for k in lone), (bank, lone)
        if bank == "mfcc40":
            # the live push names members 0, 1, 2 of four: the fourth (float32, its own launches) stays out, so fewer float launches than unrouted
            f32 = lambda c: sum(v for k, v in c.items() if k.startswith("kws_nn_f32"))
            assert 0 < f32(launches[(bank, "live_push_onehot")]) < f32(launches[(bank, "live_push_fresh")]), bank


def _lists(routes, K):
    """the packed lists of csrc/kws_bank.h restated: member k's count, then the rows whose route names it, ascending"""
    out, at = [], [0]
    for k in range(K):
        rows = [i for i, r in enumerate(routes) if (r >> k) & 1]
        out += [len(rows)] + rows
        at.append(len(out))
    return out, at


def test_list_building_against_a_restatement(run):
    lines, _ = run
    seen = 0
    for ln in lines:
        if not ln.startswith("lists "):
            continue
        head, routes, packed, at = [part.split() for part in ln.split("|")]
        K, n = int(head[1]), int(head[2])
        routes = [int(x) for x in routes]
        assert len(routes) == n and all(r < (1 << K) for r in routes)
        want, want_at = _lists(routes, K)
        assert [int(x) for x in packed] == want and [int(x) for x in at] == want_at, (K, n)
        if n >= 37:
            assert 0 in routes and any(r for r in routes)                 # zero masks among the random ones
        seen += 1
    assert seen == 20
