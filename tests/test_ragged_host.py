"""kws_run_classifier_ragged_device / kws_window_frame_count without a GPU: the symbols are exported and bound, and the host side -- the frame
count, every refusal of the contract, the descriptor table, staging and grouping, scratch growth and reuse -- runs under ASan + UBSan against
a stub HIP runtime that records launches (tests/ragged/ragged_hip_stub.cpp; kernels do not run there).  The driver links the new units ON
TOP of the host objects host_exe built from the fixed unit list of tests/sanitize/Makefile, as the bank's host test does: that host_exe
itself links shows that no existing unit came to depend on the new ones."""
import ctypes
import glob
import os
import subprocess

import pytest

from kws_testlib import MODELS, ROOT, OracleModel, synth_model_blob

CSRC = os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
# the flags of tests/sanitize/Makefile's host-only build of the library
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-ffp-contract=off",
         "-DKWS_BUILDING_LIBRARY", "-Wno-unused-value"] + SAN
RAGGED_SYMBOLS = {"kws_window_frame_count", "kws_run_classifier_ragged_device"}
DRIVER_MODELS = ["l476_no_yes.kwsm", "l476_no_yes_f32.kwsm", "cfg2_mfcc40_int8.kwsm"]        # + an MFE-block blob and a general-shape one
# a general-shape plan with a framing of its own: 321-sample frames every 161 (tests/test_gpu_generic_dsp.py: odd_stride_fft512)
GENERAL_KW = dict(seed=3, blocks=((8, 3, 7), (4, 3, 7)), n_labels=3, fft_length=512, frame_length=0.0200625, frame_stride=0.0100625, win_size=31)
BAD_ARGUMENT, UNSUPPORTED_MODEL = -20, -18


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    return load_package()


def test_ragged_symbols_are_exported_and_bound():
    pkg = _pkg()
    assert RAGGED_SYMBOLS <= set(pkg.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, s) for s in RAGGED_SYMBOLS)
    for method in ("run_classifier_ragged_device", "window_frame_count"):
        assert callable(getattr(pkg.Model, method)), method
    header = open(os.path.join(ROOT, "include", "kws", "kws.h")).read()
    assert all(s + "(" in header for s in RAGGED_SYMBOLS)


@pytest.fixture(scope="module")
def ragged_run(host_exe, tmp_path_factory):
    """tests/ragged/ragged_host_driver.cpp linked with the host objects host_exe built plus the two new units compiled the same way, against
    the launch-recording stub instead of tests/sanitize/hip_stub.cpp; run once on three shipped models, the MFE-block blob of
    tests/test_other_window_length.py and one general-shape blob."""
    lib_dir = os.path.dirname(host_exe)
    out = str(tmp_path_factory.mktemp("kws_ragged_stub"))
    objs = []
    for unit, ext in (("kws_ragged", "cpp"), ("kws_ragged_kernels", "hip")):
        o = os.path.join(out, "ragged_" + unit + ".o")
        subprocess.check_call([CLANG] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, unit + "." + ext)])
        objs.append(o)
    # the kernel unit's host side refers to its device code object: one dummy word (as tests/sanitize/Makefile does for the others)
    syms = subprocess.check_output(["nm", "-u", objs[1]]).decode().split()
    known = open(os.path.join(lib_dir, "fatbin_syms.c")).read()
    extra = sorted({s for s in syms if s.startswith("__hip_fatbin_") and s not in known})
    src = os.path.join(out, "ragged_fatbin_syms.c")
    with open(src, "w") as f:
        f.writelines("const unsigned long long %s = 0;\n" % s for s in extra)
    fo = os.path.join(out, "ragged_fatbin_syms.o")
    subprocess.check_call([CLANG, "-x", "c", "-c", "-o", fo, src])
    stub = os.path.join(out, "ragged_hip_stub.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN +
                          ["-c", "-o", stub, os.path.join(ROOT, "tests", "ragged", "ragged_hip_stub.cpp")])
    drv = os.path.join(out, "ragged_host_driver.o")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17"] + SAN + ["-c", "-o", drv, os.path.join(ROOT, "tests", "ragged", "ragged_host_driver.cpp")])
    skip = {"host_driver.o", "boundary_driver.o", "hip_stub.o", "fatbin_syms.o"}
    own = ("scan_", "slide_", "live_", "geometry_", "bank_")        # objects other host tests add to that directory
    lib_objs = [p for p in sorted(glob.glob(os.path.join(lib_dir, "*.o"))) if os.path.basename(p) not in skip and not os.path.basename(p).startswith(own)]
    exe = os.path.join(out, "kws_ragged_san")
    subprocess.check_call([CLANG] + SAN + ["-o", exe] + lib_objs + objs + [fo, os.path.join(lib_dir, "fatbin_syms.o"), stub, drv, "-ldl", "-lpthread"])
    general = os.path.join(out, "general.kwsm")
    open(general, "wb").write(synth_model_blob(**GENERAL_KW))
    from test_other_window_length import _mfe_blob
    mfe = os.path.join(out, "mfe.kwsm")
    open(mfe, "wb").write(_mfe_blob())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + [os.path.join(MODELS, m) for m in DRIVER_MODELS] + [mfe, general], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln.split(None, 6) for ln in p.stdout.splitlines()]
    assert lines[-1] == ["done"]
    assert [ln for ln in lines if ln[0] == "load"] == [["load", str(i), "0"] for i in range(5)]
    return lines, general


def test_existing_units_do_not_depend_on_the_ragged_units(host_exe):
    objs = glob.glob(os.path.join(os.path.dirname(host_exe), "kws_*.o"))
    assert objs
    undefined = subprocess.check_output(["nm", "-u"] + objs).decode()
    assert "ragged" not in undefined


def test_window_frame_count_is_the_oracles(ragged_run, oracle, l476):
    lines, general = ragged_run
    got = {ln[1]: [int(v) for v in " ".join(ln[2:]).split()] for ln in lines if ln[0] == "frames"}
    assert set(got) == {"0", "4"} and all(len(v) == 17001 for v in got.values())
    assert got["0"] == [max(0, oracle.num_frames(n, l476.cfg)) for n in range(17001)]
    assert got["0"][639:641] == [0, 1] and got["0"][16319:16321] == [49, 50]
    cfg = OracleModel(oracle, general).cfg
    assert got["4"] == [max(0, oracle.num_frames(n, cfg)) for n in range(17001)]
    assert got["4"] != got["0"]
    assert ["frames_null", "0"] in lines


def test_ragged_refusals_name_the_clip_and_launch_nothing(ragged_run):
    lines, _ = ragged_run
    for mi, is_float in enumerate((False, True, False, False, False)):
        refused = {ln[2]: (int(ln[3]), int(ln[4]), int(ln[5]), ln[6] if len(ln) > 6 else "") for ln in lines if ln[0] == "refuse" and ln[1] == str(mi)}
        want = {"len0_at3", "short_at3", "long_at3", "first_of_two_at5", "all_null", "null_handle", "null_pcm", "null_offsets", "null_lengths", "huge_batch"}
        assert set(refused) == want | ({"q_on_float"} if is_float else set()), (mi, sorted(refused))
        for name, (rc, launches, untouched, msg) in refused.items():
            assert rc == (UNSUPPORTED_MODEL if name == "q_on_float" else BAD_ARGUMENT) and launches == 0 and untouched == 1, (mi, name, rc, launches, untouched)
        for name in ("len0_at3", "short_at3", "long_at3"):
            assert "clip 3 has" in refused[name][3] and "kws_slide_recordings_device" in refused[name][3], refused[name][3]
        assert "clip 3 has 0 samples" in refused["len0_at3"][3]
        assert "clip 5 has 1 samples" in refused["first_of_two_at5"][3]                   # the FIRST offending index
        for name in ("null_pcm", "null_offsets", "null_lengths"):
            assert name[5:] in refused[name][3]
        ok = {ln[2]: [int(v) for v in ln[3:6]] for ln in lines if ln[0] == "ok" and ln[1] == str(mi)}
        assert ok == {"b0": [0, 0, 1], "b0_null_arrays": [0, 0, 1]}, (mi, ok)           # B == 0: EI_IMPULSE_OK, no launch, nothing written


def test_ragged_batch_sizes_and_scratch_reuse(ragged_run):
    lines, _ = ragged_run
    for mi, is_float in enumerate((False, True, False, False, False)):
        calls = {ln[2]: int(ln[3]) for ln in lines if ln[0] == "call" and ln[1] == str(mi)}
        want = {"b1", "b10_staged", "b5000_mixed", "b3_reuse", "b7000_aligned", "b64_features_only"} | (set() if is_float else {"b64_q_only"})
        assert set(calls) == want and all(rc == 0 for rc in calls.values()), (mi, calls)


def test_ragged_dsp_block_is_one_launch_whatever_the_lengths(ragged_run):
    lines, _ = ragged_run
    n = {(int(ln[1]), ln[2]): [int(v) for v in ln[3:6]] for ln in lines if ln[0] == "launches"}
    for mi in (0, 1, 2):                                   # MFCC block, tuned shapes: int8, float32, 40 cepstra
        assert n[(mi, "one_length")][:2] == [1, 1] and n[(mi, "all_frame_counts")][:2] == [1, 1], (mi, n)
        assert n[(mi, "one_length")] == n[(mi, "all_frame_counts")]
        assert n[(mi, "all_frame_counts_staged")][:2] == [2, 1]        # clips off the 16-byte grid: one staging launch in front
    for mi in (3, 4):                                      # MFE block, general shape: the grouped route, launches per distinct frame count
        assert n[(mi, "one_length")][1] == 0 and n[(mi, "all_frame_counts")][1] == 0
        assert n[(mi, "all_frame_counts")][0] > n[(mi, "one_length")][0] >= 3
