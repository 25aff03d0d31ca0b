"""Pools without a GPU (kws_pool_*; the contract is in include/kws/kws.h): the symbols are exported, bound and declared, and the host side --
every refusal with its code, the named member / row / entry and no launch; the front end's launches being the single-model call's, exactly
one pool network launch whatever K and none when every row names nobody, one moving-average launch per push, no launch of any member's own
kernels; and the list and work-item building against the restatement in tests/pool_testlib.py -- runs under ASan + UBSan against the stub
HIP runtime of tests/sanitize (kernels do not run there; its KWS_STUB_RECORD trace gives the launches of every bracketed call).  The driver
(tests/pool/pool_host_driver.cpp, with its own main) links the pool's, the bank's and the pipelines' units ON TOP of the host objects
host_exe built from the fixed unit list of tests/sanitize/Makefile, as tests/test_bank_route_host.py does.  Nothing is loaded into Python
under a sanitizer."""
import collections
import ctypes
import glob
import os
import subprocess

import pytest

from kws_testlib import MODELS, ROOT
from pool_testlib import POOL_MAX, POOL_NONE, items_and_rows, write_tenants

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
SYMBOLS = {"kws_pool_create", "kws_pool_destroy", "kws_pool_size", "kws_pool_member", "kws_pool_score_stride", "kws_pool_item_rows",
           "kws_pool_run_classifier_device", "kws_pool_run_classifier_ragged_device", "kws_pool_live_create", "kws_pool_live_destroy",
           "kws_pool_live_reset", "kws_pool_live_assign", "kws_pool_live_window_count", "kws_pool_live_push_device"}
UNITS = [("kws_pool", "cpp"), ("kws_pool_kernels", "hip"),
         ("kws_bank", "cpp"), ("kws_bank_kernels", "hip"), ("kws_bank_windows", "cpp"), ("kws_bank_windows_kernels", "hip"),
         ("kws_scan", "cpp"), ("kws_scan_kernels", "hip"), ("kws_live", "cpp"), ("kws_live_kernels", "hip"),
         ("kws_slide", "cpp"), ("kws_slide_kernels", "hip"), ("kws_slide_live", "cpp"), ("kws_slide_live_kernels", "hip"),
         ("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")]
POOLS = {"six": 6, "alone": 1}
BAD_ARGUMENT, UNSUPPORTED_MODEL = -20, -18
CREATE_REFUSALS = {"k_zero": BAD_ARGUMENT, "k_above_max": BAD_ARGUMENT, "null_members": BAD_ARGUMENT, "null_member": BAD_ARGUMENT,
                   "same_handle_twice": BAD_ARGUMENT, "other_front_end": BAD_ARGUMENT, "float32_member": UNSUPPORTED_MODEL,
                   "float32_alone": UNSUPPORTED_MODEL, "other_family_member": UNSUPPORTED_MODEL, "null_out": BAD_ARGUMENT}
REFUSALS = {"bad_index", "no_output", "null_pool", "null_pcm", "null_member", "batch_too_large",
            "ragged_bad_index", "ragged_null_pool", "ragged_no_output", "ragged_null_member", "ragged_null_pcm", "ragged_null_lengths",
            "assign_pushed", "assign_range", "assign_twice", "assign_bad_index", "assign_null_session", "assign_null_member",
            "push_stream_range", "push_stream_twice", "push_null_scores", "push_null_session"}
CALLS = {"own_batch", "batch_robin", "batch_one", "batch_none", "batch_features_only", "batch_b0", "own_ragged", "ragged_robin", "own_live_push",
         "live_push_unassigned", "live_assign", "live_push_assigned", "live_push_in_place", "live_push_stream4", "live_reset", "live_assign_after_reset",
         "live_push_after_unassign", "live_push_finish", "live_assign_after_finish"}
# kernels behind the front end: a model's own networks and moving average, the bank's, the pool's
OWN = ("kws_nn", "kws_dense", "kws_scan_maf", "kws_live_maf", "kws_bank_")
BEHIND = OWN + ("kws_pool_",)


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_pool_symbols_are_exported_bound_and_declared():
    pkg = _pkg()
    assert SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    for name in ("run_classifier_device", "run_classifier_ragged_device", "live_streams", "score_stride", "members", "__len__", "close"):
        assert hasattr(pkg.Pool, name), name
    for name in ("assign", "push_device", "window_count", "reset", "close"):
        assert callable(getattr(pkg.PoolLiveStreams, name)), name
    assert pkg.POOL_NONE == POOL_NONE and pkg.POOL_MAX == POOL_MAX
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)
    assert "#define KWS_POOL_MAX %d" % POOL_MAX in header and "#define KWS_POOL_NONE 0xffffffffu" in header


@pytest.fixture(scope="module")
def run(host_exe, tmp_path_factory):
    """(stdout lines, {(pool, call): Counter of launched kernels by name without template arguments}) of one run of the driver"""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_pool_stub"))
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
    drv = os.path.join(out, "pool_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "pool", "pool_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_", "ragged_", "br_", "pool_")          # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_pool_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), os.path.join(lib_dir, "hip_stub.o"),
                                                                         drv, "-ldl", "-lpthread"])
    models = write_tenants(out, "49x40", 6) + write_tenants(out, "49x13", 1) + [os.path.join(MODELS, "cfg2_mfcc40_f32.kwsm"),
                                                                                 os.path.join(MODELS, "cfg5_dscnn_mfcc40_int8.kwsm")]
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
            out[w[2]] = (int(w[3]), int(w[4]), msg)
    return out


def test_driver_ran_to_the_end_under_the_sanitizers(run):
    """every call that does work returns EI_IMPULSE_OK; nothing the sanitizers report (exit 0)"""
    lines, _ = run
    assert lines[-1] == "done" and "accessors 6 1 1 0 0" in lines
    assert all(ln.split()[2] == "0" for ln in lines if ln.startswith("load "))
    for pool, K in POOLS.items():
        calls = {ln.split()[2]: int(ln.split()[3]) for ln in lines if ln.startswith("call " + pool + " ")}
        assert set(calls) == CALLS and all(rc == 0 for rc in calls.values()), (pool, calls)
        # tenants 0 .. 5 have 3, 4, 6, 3, 4, 6 labels; the pool of one holds tenant 2
        assert "pool %s %d 6" % (pool, K) in lines
        # an unassigned stream's windows are counted as an assigned stream's are
        counts = [ln.split()[3:] for ln in lines if ln.startswith("windows " + pool + " ")]
        assert len(counts) == 2 and counts[0] == counts[1] == ["4", "3", "2"], counts


def test_creation_refusals_name_the_member_and_the_reason(run):
    lines, launches = run
    refused = _refused(lines, "create")
    assert set(refused) == set(CREATE_REFUSALS), set(refused) ^ set(CREATE_REFUSALS)
    for name, code in CREATE_REFUSALS.items():
        assert refused[name][:2] == (code, 1), (name, refused[name])                           # the code; *out is NULL
        assert name == "null_out" or sum(launches[("create", name)].values()) == 0, name
    msg = {k: v[2] for k, v in refused.items()}
    assert "1 to %d members, not 0" % POOL_MAX in msg["k_zero"] and "not %d" % (POOL_MAX + 1) in msg["k_above_max"]
    assert "member 1 is NULL" in msg["null_member"] and "members 1 and 3 are the same handle" in msg["same_handle_twice"]
    assert "member 1 differs from member 0 in" in msg["other_front_end"]                       # (the bank's rule with its message)
    assert "member 2" in msg["float32_member"] and "float32" in msg["float32_member"] and "member 0" in msg["float32_alone"]
    assert "member 1" in msg["other_family_member"] and "outside the two-block matrix-core shape" in msg["other_family_member"]


def test_refusals_return_their_code_launch_nothing_and_change_nothing(run):
    lines, launches = run
    for pool, K in POOLS.items():
        refused = _refused(lines, pool)
        assert set(refused) == REFUSALS, (pool, set(refused) ^ REFUSALS)
        for name in REFUSALS:
            assert refused[name][:2] == (BAD_ARGUMENT, 1), (pool, name, refused[name])         # the code; outputs, counts and members untouched
            assert sum(launches[(pool, name)].values()) == 0, (pool, name, launches[(pool, name)])
        # kws_last_error names the FIRST offending row or entry and its value
        assert "clip 3: member %d " % K in refused["bad_index"][2] and "the pool's %d" % K in refused["bad_index"][2], refused["bad_index"]
        assert "clip 4: member %d " % K in refused["ragged_bad_index"][2], refused["ragged_bad_index"]
        assert "entry 1: stream 0 has been pushed to" in refused["assign_pushed"][2], refused["assign_pushed"]
        assert "entry 0: stream 5 of 5" in refused["assign_range"][2] and "entry 1: stream 4 named twice" in refused["assign_twice"][2]
        assert "entry 0: member %d " % K in refused["assign_bad_index"][2], refused["assign_bad_index"]
        assert "stream 5 of 5" in refused["push_stream_range"][2] and "named twice" in refused["push_stream_twice"][2]
        assert "no output requested" in refused["no_output"][2] and "too large" in refused["batch_too_large"][2]


def test_launches_front_end_once_one_network_launch_whatever_k_and_one_moving_average(run):
    _, launches = run
    front = lambda c: {k: v for k, v in c.items() if not k.startswith(BEHIND)}
    for pool in POOLS:
        L = lambda name: launches[(pool, name)]
        # the front end's launches are the single-model call's; behind it exactly one pool network launch, and no member's own kernel
        for name, own in (("batch_robin", "own_batch"), ("batch_one", "own_batch"), ("ragged_robin", "own_ragged"), ("live_push_assigned", "own_live_push")):
            assert front(L(own)) and front(L(name)) == front(L(own)), (pool, name, L(name), L(own))
            assert L(name)["kws_pool_nn_mfma_kernel"] == 1, (pool, name, L(name))
            assert not any(k.startswith(OWN) for k in L(name)), (pool, name, L(name))
        assert any(k.startswith("kws_nn") for k in L("own_batch")) and any(k.startswith("kws_live_maf") for k in L("own_live_push"))
        # rows that all name nobody, a call that wants features only, no rows: no network launch (the front end alone / nothing at all)
        for name in ("batch_none", "batch_features_only"):
            assert front(L(name)) == front(L("own_batch")) and not any(k.startswith(BEHIND) for k in L(name)), (pool, name, L(name))
        assert sum(L("batch_b0").values()) == 0
        # one moving-average launch per push that has windows, assigned or not; no network for unassigned streams
        for name in ("live_push_assigned", "live_push_in_place", "live_push_stream4"):
            assert L(name)["kws_pool_maf_live_kernel"] == 1 and L(name)["kws_pool_nn_mfma_kernel"] == 1, (pool, name, L(name))
            assert not any(k.startswith(OWN) for k in L(name)), (pool, name, L(name))
        for name in ("live_push_unassigned", "live_push_after_unassign"):
            assert L(name)["kws_pool_maf_live_kernel"] == 1 and L(name)["kws_pool_nn_mfma_kernel"] == 0, (pool, name, L(name))
            assert front(L(name)) == front(L("own_live_push")) and not any(k.startswith(OWN) for k in L(name)), (pool, name, L(name))
        assert sum(L("live_assign").values()) == 0


def test_list_and_item_building_against_the_restatement(run):
    lines, _ = run
    seen, spanning = 0, 0
    for ln in lines:
        if not ln.startswith("items "):
            continue
        head, member, items, rows = [part.split() for part in ln.split("|")]
        K, n, item_rows = int(head[1]), int(head[2]), int(head[3])
        member = [int(x) for x in member]
        assert len(member) == n and all(m < K or m == POOL_NONE for m in member)
        want_items, want_rows = items_and_rows(member, K, item_rows)
        got = [int(x) for x in items]
        assert len(got) % 4 == 0 and [tuple(got[i:i + 3]) for i in range(0, len(got), 4)] == want_items and not any(got[3::4]), (K, n, item_rows)
        assert [int(x) for x in rows] == want_rows, (K, n, item_rows)
        if n >= 37:
            assert POOL_NONE in member and any(m != POOL_NONE for m in member)
        spanning += any(c == item_rows for _, _, c in want_items) and any(k == 0 and c < item_rows for k, _, c in want_items)
        seen += 1
    assert seen == 48 and spanning >= 6
    # the accessor the GPU tests place their lists by: the driver's statically linked value is the built library's
    assert "item_rows %d" % ctypes.CDLL(_pkg().LIB_PATH).kws_pool_item_rows() in lines
