"""Routed recording and cepstra-in bank calls without a GPU (kws_bank_scan_recordings_routed_device,
kws_bank_slide_recordings_routed_device, kws_bank_cmvn_inference_routed_device): the symbols are exported, bound and declared, and the host
side -- every refusal with its code, its named index and mask and without a launch, NULL and all-member routes launching exactly what the
unrouted call launches, one-hot routes launching the front end once, nothing for a member no recording with windows names, one moving
average per scan whatever K, and the per-window route table against a restatement in Python -- runs under ASan + UBSan against the stub
HIP runtime of tests/sanitize (kernels do not run there; its KWS_STUB_RECORD trace gives the launches of every bracketed call).  The driver
is a program of its own (tests/bank_route_recordings), linked as tests/test_bank_route_host.py links its driver: the bank's and the
pipelines' units ON TOP of the host objects host_exe built from the fixed unit list of tests/sanitize/Makefile."""
import collections
import ctypes
import glob
import inspect
import os
import subprocess

import pytest

from kws_testlib import MODELS, ROOT

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
SYMBOLS = {"kws_bank_scan_recordings_routed_device", "kws_bank_slide_recordings_routed_device", "kws_bank_cmvn_inference_routed_device"}
UNITS = [("kws_bank", "cpp"), ("kws_bank_kernels", "hip"), ("kws_bank_windows", "cpp"), ("kws_bank_windows_kernels", "hip"),
         ("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip"),
         ("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_slide_live", "cpp"), ("kws_slide_live_kernels", "hip"),
         ("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")]
MFCC40 = ["cfg2_mfcc40_int8.kwsm", "cfg2_mfcc40_f32.kwsm", "cfg5_dscnn_mfcc40_int8.kwsm", "cfg5_dscnn_mfcc40_f32.kwsm"]
DRIVER_MODELS = MFCC40 + ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "l432_trick_or_treat.kwsm"]
BANKS = {"mfcc40": 4, "l476": 2, "l432_alone": 1}
BAD_ARGUMENT, DSP_ERROR = -20, -5
REFUSALS = {
    "scan_routed_bad_bit": BAD_ARGUMENT, "scan_routed_null_bank": BAD_ARGUMENT, "scan_routed_null_pcm": BAD_ARGUMENT,
    "scan_routed_null_scores": BAD_ARGUMENT, "scan_routed_nothing_wanted": BAD_ARGUMENT, "scan_routed_bad_slicing": DSP_ERROR,
    "scan_routed_short_bad_bit": BAD_ARGUMENT,
    "scan_null_routes_null_pcm": BAD_ARGUMENT, "scan_null_routes_bad_slicing": DSP_ERROR, "scan_null_routes_nothing_wanted": BAD_ARGUMENT,
    "slide_routed_bad_bit": BAD_ARGUMENT, "slide_routed_null_bank": BAD_ARGUMENT, "slide_routed_null_pcm": BAD_ARGUMENT,
    "slide_routed_null_scores": BAD_ARGUMENT, "slide_routed_nothing_wanted": BAD_ARGUMENT, "slide_routed_bad_hop": BAD_ARGUMENT,
    "slide_routed_bad_flags": BAD_ARGUMENT, "slide_routed_short_bad_bit": BAD_ARGUMENT,
    "slide_null_routes_null_pcm": BAD_ARGUMENT, "slide_null_routes_bad_hop": BAD_ARGUMENT, "slide_null_routes_bad_flags": BAD_ARGUMENT,
    "cmvn_routed_bad_bit": BAD_ARGUMENT, "cmvn_routed_null_bank": BAD_ARGUMENT, "cmvn_routed_null_mfcc": BAD_ARGUMENT,
    "cmvn_routed_null_scores": BAD_ARGUMENT, "cmvn_routed_nothing_wanted": BAD_ARGUMENT,
    "cmvn_null_routes_null_mfcc": BAD_ARGUMENT, "cmvn_null_routes_nothing_wanted": BAD_ARGUMENT,
}
# calls that have nothing to do: EI_IMPULSE_OK and no launch.  R = 0 / B = 0 with a routes pointer whose one entry is a bad mask: no route
# is read (the batch routed call's rule: the routes [R] are checked, then the empty call returns -- *_short_bad_bit above is the other half)
EMPTY = {"scan_r0", "scan_short", "slide_r0", "slide_short", "cmvn_b0"}
# kernels behind the front end: the members' networks (the bank's own kernels and quantise passes among them) and the moving averages
BEHIND = ("kws_nn", "kws_dense", "kws_bank_nn", "kws_quantize", "kws_bank_quantize", "kws_scan_maf", "kws_live_maf", "kws_bank_maf")
SLIDE_FLAGS = ("", "_direct", "_shared")
SAME_AS_UNROUTED = ([("scan_null_routes", "scan_unrouted"), ("scan_all_routes", "scan_unrouted"), ("scan_all_but_short", "scan_unrouted"),
                     ("slide_all_but_short", "slide_unrouted"), ("cmvn_null_routes", "cmvn_unrouted"), ("cmvn_all_routes", "cmvn_unrouted")] +
                    [("slide_null_routes" + f, "slide_unrouted" + f) for f in SLIDE_FLAGS] + [("slide_all_routes" + f, "slide_unrouted" + f) for f in SLIDE_FLAGS])
ONE_HOT = ([("scan_onehot", "scan_unrouted"), ("scan_onehot_in_place", "scan_unrouted"), ("cmvn_onehot", "cmvn_unrouted")] +
           [("slide_onehot" + f, "slide_unrouted" + f) for f in SLIDE_FLAGS])
OTHER_CALLS = {"scan_first_only", "scan_last_only", "scan_none", "scan_short_names_last", "scan_first_only_no_buffer", "slide_none",
               "slide_short_names_last", "cmvn_first_only", "cmvn_last_only", "cmvn_none"}


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_routed_recording_symbols_are_exported_bound_and_declared():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    L = pkg.lib()
    assert all(getattr(L, s).argtypes for s in SYMBOLS)                  # bound: the prototypes are set
    for method in (pkg.Bank.scan_recordings_device, pkg.Bank.slide_recordings_device, pkg.Bank.cmvn_inference_batch_device):
        params = inspect.signature(method).parameters
        assert list(params)[-1] == "routes" and params["routes"].default is None, method
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)
    assert "Not routed in this version: the host-buffer and SDK forms." in header
    assert "Not routed in this version: recording scans" not in header


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    """(stdout lines, {(bank, call): Counter of launched kernels by name without template arguments}, {(bank, call, kernel): [grid x]}) of
    one run of the driver"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_bank_route_recordings_stub"))
    objs = []
    for unit, ext in UNITS:
        o = os.path.join(out, "brr_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + [o for o in objs if "kernels" in o]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "brr_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "brr_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "bank_route_recordings_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv,
                                                                      os.path.join(ROOT, "tests", "bank_route_recordings", "bank_route_recordings_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_")          # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_bank_route_recordings_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), os.path.join(lib_dir, "hip_stub.o"),
                                                                         drv, "-ldl", "-lpthread"])
    trace = os.path.join(out, "trace.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", KWS_STUB_RECORD=trace)
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in DRIVER_MODELS], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    launches, grids, cur, key = {}, collections.defaultdict(list), None, None
    for ln in open(trace):
        w = ln.split()
        if w[0] == "BEGIN":
            key = (w[1], w[2])
            cur = launches.setdefault(key, collections.Counter())
        elif w[0] == "END":
            cur = None
        elif w[0] == "launch" and cur is not None:
            name = ln.split(" | ", 1)[1].strip()
            name = name[5:] if name.startswith("void ") else name
            name = name.split("<")[0].split("(")[0]
            cur[name] += 1
            grids[key + (name,)].append(int(w[2].split("=")[1].split(",")[0]))
    return p.stdout.splitlines(), launches, grids


def _behind(c):
    return {k: v for k, v in c.items() if k.startswith(BEHIND)}


def _front(c):
    return {k: v for k, v in c.items() if not k.startswith(BEHIND)}


def _windows(lines, bank, what):
    (ln,) = [ln for ln in lines if ln.startswith("windows %s %s |" % (bank, what))]
    return [int(x) for x in ln.split("|")[1].split()]


def test_driver_ran_to_the_end_under_the_sanitizers(run):
    """every call that does work returns EI_IMPULSE_OK; nothing the sanitizers report (exit 0); the recordings are the ones the cases need"""
    lines, launches, _ = run
    assert lines[-1] == "done"
    for bank in BANKS:
        calls = {ln.split()[2]: int(ln.split()[3]) for ln in lines if ln.startswith("call " + bank + " ")}
        assert calls and all(rc == 0 for rc in calls.values()), (bank, calls)
        assert {a for pair in SAME_AS_UNROUTED + ONE_HOT for a in pair} | OTHER_CALLS | EMPTY == set(calls), (bank, set(calls))
        # recordings without a window between and after recordings that have some
        scan, slide = _windows(lines, bank, "scan"), _windows(lines, bank, "slide")
        assert scan[1] == scan[4] == 0 and all(scan[r] > 0 for r in (0, 2, 3, 5)), (bank, scan)
        assert slide[1] == slide[4] == 0 and slide[0] > 1 and slide[2] == 1 and slide[3] == 2, (bank, slide)


def test_refusals_return_their_code_name_the_index_and_mask_and_launch_nothing(run):
    lines, launches, _ = run
    for bank, K in BANKS.items():
        refused = {}
        for ln in lines:
            if ln.startswith("refuse " + bank + " "):
                head, msg = ln.split(" | ", 1)
                w = head.split()
                refused[w[2]] = (int(w[3]), int(w[4]), msg)
        assert set(refused) == set(REFUSALS), (bank, set(refused) ^ set(REFUSALS))
        for name, code in REFUSALS.items():
            assert refused[name][:2] == (code, 1), (bank, name, refused[name])       # the code; every output buffer untouched
            assert sum(launches[(bank, name)].values()) == 0, (bank, name, launches[(bank, name)])
        # kws_last_error names the FIRST offending index and its mask
        every = (1 << K) - 1
        assert "recording 2:" in refused["scan_routed_bad_bit"][2] and "0x%x" % (every | 1 << K) in refused["scan_routed_bad_bit"][2], refused["scan_routed_bad_bit"]
        assert "recording 3:" in refused["slide_routed_bad_bit"][2] and "0x%x" % (1 << K) in refused["slide_routed_bad_bit"][2], refused["slide_routed_bad_bit"]
        assert "row 3:" in refused["cmvn_routed_bad_bit"][2] and "0x%x" % (every | 1 << K) in refused["cmvn_routed_bad_bit"][2], refused["cmvn_routed_bad_bit"]
        # a bad route is refused although no recording of the call has a window: routes are checked before the empty call returns
        for name in ("scan_routed_short_bad_bit", "slide_routed_short_bad_bit"):
            assert "recording 1:" in refused[name][2] and "0x%x" % (1 << K) in refused[name][2], refused[name]
        # NULL routes: the unrouted call's own refusals, word for word what the routed form says for the same mistake
        assert refused["scan_null_routes_bad_slicing"] == refused["scan_routed_bad_slicing"]
        assert refused["slide_null_routes_bad_hop"] == refused["slide_routed_bad_hop"] and refused["slide_null_routes_bad_flags"] == refused["slide_routed_bad_flags"]
        # calls without a row: nothing is launched (with R = 0 / B = 0 the one bad mask behind `routes` is not read)
        for name in EMPTY:
            assert sum(launches[(bank, name)].values()) == 0, (bank, name, launches[(bank, name)])


def test_null_and_all_member_routes_launch_what_the_unrouted_call_launches(run):
    """the same kernels by name, the same counts: such a call IS the unrouted call; the routes of recordings without a window do not count"""
    _, launches, _ = run
    for bank in BANKS:
        for name, ref in SAME_AS_UNROUTED:
            assert launches[(bank, ref)] and launches[(bank, name)] == launches[(bank, ref)], (bank, name, launches[(bank, name)], launches[(bank, ref)])
            assert not any("routed" in k for k in launches[(bank, name)]), (bank, name)


def test_one_hot_routes_front_end_once_no_launch_for_an_unnamed_member_and_one_moving_average(run):
    lines, launches, grids = run
    for bank, K in BANKS.items():
        if K == 1:
            # one member: one-hot routes name every member, the unrouted launches
            assert all(launches[(bank, name)] == launches[(bank, ref)] for name, ref in ONE_HOT), bank
            continue
        for name, ref in ONE_HOT:
            got, unrouted = launches[(bank, name)], launches[(bank, ref)]
            assert _front(unrouted) and _front(got) == _front(unrouted), (bank, name, got, unrouted)
            # both banks hold int8 matrix-core members of ONE row width: one routed launch for them (one chunk), none of the unrouted form
            assert got["kws_bank_nn_mfma_routed_kernel"] == 1 and got["kws_bank_nn_mfma_kernel"] == 0, (bank, name, got)
            assert got["kws_bank_quantize_kernel"] == 0 and got["kws_bank_quantize_routed_kernel"] <= 1, (bank, name, got)
            if name.startswith("scan"):
                assert got["kws_bank_maf_scan_routed_kernel"] == 1 and got["kws_bank_maf_kernel"] == 0 and got["kws_scan_maf_kernel"] == 0, (bank, name, got)
                assert unrouted["kws_bank_maf_kernel"] == 1 and unrouted["kws_bank_maf_scan_routed_kernel"] == 0, (bank, unrouted)
            else:
                assert not any("maf" in k for k in got), (bank, name, got)
        # the scan's recordings with windows (0, 2, 3, 5) and the nine cepstral matrices name every member of either bank: the members that
        # run their own launches then run what they run in the unrouted call, launch for launch, over their lists
        own = lambda c: {k: v for k, v in c.items() if k.startswith(("kws_nn", "kws_dense"))}
        assert own(launches[(bank, "cmvn_onehot")]) == own(launches[(bank, "cmvn_unrouted")]), bank
        assert own(launches[(bank, "scan_onehot")]) == own(launches[(bank, "scan_unrouted")]), bank
        # routes that name nobody: the front end alone, no moving average
        for name, ref in (("scan_none", "scan_unrouted"), ("slide_none", "slide_unrouted"), ("cmvn_none", "cmvn_unrouted")):
            none = launches[(bank, name)]
            assert none and not _behind(none) and dict(none) == _front(launches[(bank, ref)]), (bank, name, none)
        # only the first member (int8, matrix-core shape) / only the last (float32)
        for what in ("scan", "cmvn"):
            first, last = _behind(launches[(bank, what + "_first_only")]), _behind(launches[(bank, what + "_last_only")])
            maf = {"kws_bank_maf_scan_routed_kernel": 1} if what == "scan" else {}
            assert first == dict({"kws_bank_nn_mfma_routed_kernel": 1}, **maf), (bank, what, first)
            nets = {k: v for k, v in last.items() if "maf" not in k}
            assert nets and all(k.startswith("kws_nn_f32") for k in nets) and {k: v for k, v in last.items() if "maf" in k} == maf, (bank, what, last)
        # only recordings WITHOUT a window name the last member: nothing is launched for it -- no float32 network, and the one moving-average
        # launch has threads for the first member's labels alone (recordings with windows x labels, 64 a block)
        (labels0,) = [int(ln.split("|")[1].split()[0]) for ln in lines if ln.startswith("labels %s |" % bank)]
        n_active = sum(1 for w in _windows(lines, bank, "scan") if w)
        for name in ("scan_short_names_last", "scan_first_only"):
            assert _behind(launches[(bank, name)]) == {"kws_bank_nn_mfma_routed_kernel": 1, "kws_bank_maf_scan_routed_kernel": 1}, (bank, name, launches[(bank, name)])
            assert grids[(bank, name, "kws_bank_maf_scan_routed_kernel")] == [(n_active * labels0 + 63) // 64], (bank, name)
        assert _behind(launches[(bank, "slide_short_names_last")]) == {"kws_bank_nn_mfma_routed_kernel": 1}, (bank, launches[(bank, "slide_short_names_last")])
        # a routed member without a score buffer is skipped: with the first member alone routed, the front end and nothing else
        lone = launches[(bank, "scan_first_only_no_buffer")]
        assert lone and not _behind(lone) and dict(lone) == _front(launches[(bank, "scan_unrouted")]), (bank, lone)


def _table(route, index, n_windows):
    """the per-window routes of csrc/kws_bank.h restated: entry i's route, n_windows[i] times, in entry order"""
    out = []
    for i, w in enumerate(n_windows):
        out += [route[index[i] if index is not None else i]] * w
    return out


def test_window_route_table_against_a_restatement(run):
    lines, _, _ = run
    seen = []
    for ln in lines:
        if not ln.startswith("table "):
            continue
        head, route, index, nw, table = [part.split() for part in ln.split("|")]
        route, nw, table = [int(x) for x in route], [int(x) for x in nw], [int(x) for x in table]
        index = None if index == ["-"] else [int(x) for x in index]
        assert int(head[1]) == len(nw) and (index is not None or len(route) == len(nw))
        assert table == _table(route, index, nw), ln
        seen.append((nw, index))
    assert len(seen) == 5
    # the first line: the scan's own counts, with recordings that have no window at the front, in the middle and at the end
    nw = seen[0][0]
    assert nw[0] == nw[1] == 0 and nw[2] > 0 and 0 in nw[3:-1] and any(nw[3:-1]) and nw[-1] == 0, nw
    assert not any(seen[1][0]) and seen[2][0] == [6] and seen[3][0] == [] and seen[4][1] == [4, 0, 2]
