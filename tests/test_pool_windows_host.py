"""The pool's window calls without a GPU (kws_pool_scan_recordings_device, kws_pool_slide_recordings_device, kws_pool_cmvn_inference_device,
kws_pool_slide_live_*; the contract is in include/kws/kws.h): the symbols are exported, bound and declared, and the host side -- every
refusal with its code, the named recording / row / entry and no launch; the front end's launches being the first member's own call's,
one pool network launch per gathered chunk whatever K, exactly one kws_pool_maf_scan_kernel per scan, neither pool kernel when nobody is
named, no launch of a member's own, the scan's or a bank's kernels; the per-window member table against a restatement here; a live one-shot
session taking a new member after a push -- runs under ASan + UBSan against the stub HIP runtime of tests/sanitize (kernels do not run
there; its KWS_STUB_RECORD trace gives the launches of every bracketed call).  The driver (tests/pool/pool_windows_host_driver.cpp, with
its own main) is built and linked as tests/test_pool_host.py builds its own.  Nothing is loaded into Python under a sanitizer."""
import collections
import ctypes
import glob
import os
import subprocess

import pytest

from kws_testlib import ROOT
from pool_testlib import POOL_NONE, write_tenants
from test_pool_host import BEHIND, CLANG, CSRC, FLAGS, OWN, SAN, UNITS

SYMBOLS = {"kws_pool_scan_recordings_device", "kws_pool_slide_recordings_device", "kws_pool_cmvn_inference_device", "kws_pool_slide_live_create",
           "kws_pool_slide_live_destroy", "kws_pool_slide_live_path", "kws_pool_slide_live_reset", "kws_pool_slide_live_assign",
           "kws_pool_slide_live_window_count", "kws_pool_slide_live_push_device"}
POOLS = {"six": 6, "alone": 1}
BAD_ARGUMENT = -20
# refusals of the pool's own (BAD_ARGUMENT), and the ones the first member's runner would make: the pool returns that runner's code
REFUSALS = {"scan_bad_index", "scan_null_scores", "scan_null_pool", "scan_null_member", "slide_bad_index", "slide_no_output", "slide_null_pool",
            "slide_null_member", "cmvn_bad_index", "cmvn_no_output", "cmvn_null_pool", "cmvn_null_member", "cmvn_null_mfcc", "sl_create_null_pool",
            "sl_assign_range", "sl_assign_twice", "sl_assign_bad_index", "sl_assign_null_session", "sl_assign_null_member", "sl_push_stream_range",
            "sl_push_stream_twice", "sl_push_no_output", "sl_push_null_session"}
RUNNER_REFUSALS = {"scan_null_lengths", "scan_bad_slicing", "slide_null_lengths", "slide_bad_hop", "slide_bad_flags", "slide_too_many_windows",
                   "sl_create_bad_hop"}
CALLS = {"own_scan", "scan_mixed", "scan_in_place", "scan_none", "scan_windowless", "scan_r0", "own_slide", "slide_mixed", "slide_features_only",
         "slide_none", "own_slide_two_chunks", "slide_two_chunks", "own_cmvn", "cmvn_robin", "cmvn_no_features", "cmvn_none", "cmvn_features_only",
         "cmvn_b0", "own_sl_push", "sl_push_unassigned", "sl_assign", "sl_push_assigned", "sl_unassign_after_push", "sl_push_after_unassign",
         "sl_assign_after_push", "sl_push_reassigned", "sl_reset", "sl_push_after_reset", "sl_push_empty", "sl_assign_two_chunks",
         "own_sl_push_two_chunks", "sl_push_two_chunks"}
NN, MAF_SCAN = "kws_pool_nn_mfma_kernel", "kws_pool_maf_scan_kernel"


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_pool_window_symbols_are_exported_bound_and_declared():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    for name in ("scan_recordings_device", "slide_recordings_device", "cmvn_inference_device", "slide_streams"):
        assert callable(getattr(pkg.Pool, name)), name
    for name in ("assign", "push_device", "window_count", "reset", "close"):
        assert callable(getattr(pkg.PoolSlideStreams, name)), name
    assert isinstance(pkg.PoolSlideStreams.path, property)
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in SYMBOLS) and "typedef struct kws_pool_slide_live kws_pool_slide_live;" in header


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    """(stdout lines, {(pool, call): Counter of launched kernels by name without template arguments}) of one run of the driver"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_pool_windows_stub"))
    objs = []
    for unit, ext in UNITS:
        o = os.path.join(out, "pool_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel units' host side refers to their device code objects: one dummy word each (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u"] + [o for o in objs if "kernels" in o]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "pool_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "pool_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    drv = os.path.join(out, "pool_windows_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "pool", "pool_windows_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_", "br_", "pool_")          # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_pool_windows_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), os.path.join(lib_dir, "hip_stub.o"),
                                                                         drv, "-ldl", "-lpthread"])
    models = write_tenants(out, "49x40", 6)
    trace = os.path.join(out, "trace.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", KWS_STUB_RECORD=trace)
    p = subprocess.run([exe] + models, capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
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


def _refused(lines, pool):
    out = {}
    for ln in lines:
        if ln.startswith("refuse " + pool + " "):
            head, msg = ln.split(" | ", 1)
            w = head.split()
            out[w[2]] = (int(w[3]), int(w[4]), int(w[5]), msg)
    return out


def test_driver_ran_to_the_end_under_the_sanitizers(run):
    """every call that does work returns EI_IMPULSE_OK; nothing the sanitizers report, no leak (exit 0)"""
    lines, _ = run
    assert lines[-1] == "done" and "pool six 6 6" in lines
    assert all(ln.split()[2] == "0" for ln in lines if ln.startswith("load "))
    for pool in POOLS:
        calls = {ln.split()[2]: int(ln.split()[3]) for ln in lines if ln.startswith("call " + pool + " ")}
        assert set(calls) == CALLS and all(rc == 0 for rc in calls.values()), (pool, set(calls) ^ CALLS, calls)
        # the pool's session runs the path the first member's own session runs
        path = [ln.split()[2:] for ln in lines if ln.startswith("path " + pool + " ")]
        assert len(path) == 1 and path[0][0] == path[0][1] and path[0][0] in ("1", "2"), path
        # n_windows of a push is what window_count said before it, for unassigned streams as for assigned ones
        counts = {ln.split()[2]: ln.split(" ", 3)[3].split(" | ") for ln in lines if ln.startswith("windows " + pool + " ")}
        assert set(counts) == {"sl_push_unassigned", "sl_push_assigned", "sl_push_reassigned", "sl_push_after_reset"}
        assert all(got == want for got, want in counts.values()), counts
        assert counts["sl_push_unassigned"][0] == counts["sl_push_assigned"][0] == "4 3 0"


def test_refusals_return_their_code_name_the_entry_and_launch_nothing(run):
    lines, launches = run
    for pool, K in POOLS.items():
        refused = _refused(lines, pool)
        assert set(refused) == REFUSALS | RUNNER_REFUSALS, (pool, set(refused) ^ (REFUSALS | RUNNER_REFUSALS))
        for name, (code, untouched, own_code, msg) in refused.items():
            assert untouched == 1, (pool, name, refused[name])                                 # outputs, counts and members as they were
            assert sum(launches[(pool, name)].values()) == 0, (pool, name, launches[(pool, name)])
            if name in REFUSALS:
                assert code == BAD_ARGUMENT, (pool, name, refused[name])
            else:
                assert code == own_code and code < 0, (pool, name, refused[name])              # the single-model runner's code
        msg = {k: v[3] for k, v in refused.items()}
        # kws_last_error names the FIRST offending recording, row or entry and its value
        for name in ("scan_bad_index", "slide_bad_index"):
            assert "recording 1: member %d " % K in msg[name] and "the pool's %d" % K in msg[name], msg[name]
        assert "row 3: member %d " % K in msg["cmvn_bad_index"], msg["cmvn_bad_index"]
        assert "entry 0: member %d " % K in msg["sl_assign_bad_index"], msg["sl_assign_bad_index"]
        assert "entry 0: stream 5 of 5" in msg["sl_assign_range"] and "entry 1: stream 4 named twice" in msg["sl_assign_twice"]
        assert "stream 5 of 5" in msg["sl_push_stream_range"] and "entry 1: stream 3 named twice" in msg["sl_push_stream_twice"]
        assert all("no output requested" in msg[k] for k in ("slide_no_output", "cmvn_no_output", "sl_push_no_output"))
        assert "too many windows" in msg["slide_too_many_windows"] and "hop" in msg["slide_bad_hop"] and "flags" in msg["slide_bad_flags"]
        assert refused["scan_bad_slicing"][0] == -5                                            # EI_IMPULSE_DSP_ERROR, as the stream API


def test_launches_front_end_once_one_network_launch_per_chunk_and_one_scan_moving_average(run):
    lines, launches = run
    front = lambda c: {k: v for k, v in c.items() if not k.startswith(BEHIND)}
    for pool in POOLS:
        L = lambda name: launches[(pool, name)]
        chunks = {ln.split()[2]: int(ln.split()[3]) for ln in lines if ln.startswith("chunks " + pool + " ")}
        assert chunks == {"slide_two_chunks": 2, "sl_push_two_chunks": 2}
        # the front end's launches are the first member's own call's; behind it one pool network launch per gathered chunk whatever K
        for name, own, n_nn in (("scan_mixed", "own_scan", 1), ("scan_in_place", "own_scan", 1), ("slide_mixed", "own_slide", 1),
                                ("slide_two_chunks", "own_slide_two_chunks", 2), ("cmvn_robin", "own_cmvn", 1), ("cmvn_no_features", "own_cmvn", 1),
                                ("sl_push_assigned", "own_sl_push", 1), ("sl_push_two_chunks", "own_sl_push_two_chunks", 2)):
            assert front(L(own)) and front(L(name)) == front(L(own)), (pool, name, L(name), L(own))
            assert L(name)[NN] == n_nn, (pool, name, L(name))
            assert not any(k.startswith(OWN) for k in L(name)), (pool, name, L(name))
            assert L(name)[MAF_SCAN] == (1 if name.startswith("scan") else 0) and L(name)["kws_pool_maf_live_kernel"] == 0, (pool, name, L(name))
        assert any(k.startswith("kws_nn") for k in L("own_scan")) and L("own_scan")["kws_scan_maf_kernel"] == 1
        assert sum(v for k, v in L("own_slide_two_chunks").items() if k.startswith("kws_nn")) == 2
        # nobody named (or only by recordings without windows), features only, no rows: the front end alone, neither pool kernel
        for name, own in (("scan_none", "own_scan"), ("scan_windowless", "own_scan"), ("slide_none", "own_slide"), ("slide_features_only", "own_slide"),
                          ("cmvn_none", "own_cmvn"), ("cmvn_features_only", "own_cmvn"), ("sl_push_unassigned", "own_sl_push")):
            assert front(L(name)) == front(L(own)) and not any(k.startswith(BEHIND) for k in L(name)), (pool, name, L(name))
        for name in ("scan_r0", "cmvn_b0", "sl_push_empty", "sl_assign", "sl_unassign_after_push", "sl_assign_after_push"):
            assert sum(L(name).values()) == 0, (pool, name, L(name))
        # a member may change after a push: no network while the stream names nobody, one launch once it has a member again
        assert L("sl_push_after_unassign")[NN] == 0 and L("sl_push_reassigned")[NN] == 1 and L("sl_push_after_reset")[NN] == 1
        assert front(L("sl_push_after_unassign")) == front(L("sl_push_reassigned")) and front(L("sl_push_reassigned"))


def test_window_member_table_against_the_restatement(run):
    """entry i has n_windows[i] windows of member assign[index[i]], or of assign[i] in the recording form (index == NULL)"""
    lines, _ = run
    seen = {"-": 0, "index": 0}
    for ln in lines:
        if not ln.startswith("table "):
            continue
        head, assign, index, nw, out = [part.split() for part in ln.split("|")]
        n = int(head[1])
        assign, nw, out = [int(x) for x in assign], [int(x) for x in nw], [int(x) for x in out]
        by_recording = index == ["-"]
        index = list(range(n)) if by_recording else [int(x) for x in index]
        assert len(index) == len(nw) == n and (len(assign) == n if by_recording else len(assign) == 12)
        want = [assign[index[i]] for i in range(n) for _ in range(nw[i])]
        assert out == want, ln
        if n >= 9:
            assert POOL_NONE in want and any(m != POOL_NONE for m in want) and 0 in nw
        seen["-" if by_recording else "index"] += 1
    assert seen == {"-": 4, "index": 4}
