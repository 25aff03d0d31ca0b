"""No GPU: csrc/kws_fast_ticket.h -- which ticket of which of the fast kernel's eight ticket heads is which clip, and the walk of a wave whose home head is
past the last clip -- compiled for the host (tests/fast_ticket/fast_ticket_driver.cpp) and dealt out as whole launches: every wave of a grid as the
kernel's clip loop, one step per access to the ticket block, the waves' steps interleaved at random from a seed.

Per launch: every clip in [0, n_sel) is taken exactly once, every wave leaves, and after the last wave's clean-up every word of the block is zero -- the
next launch of the handle starts from what the plan uploaded.  The walk runs both written out draw by draw (any two walks interleave) and as the header's
own kws_fast_ticket_walk (the lines the kernel compiles).

Grids: stride = the grid's wave count in {1, 11, 12, 88, 96} (one wave; one workgroup of the 49x40 graph's eleven waves and of the twin's twelve; eight
workgroups of either: one per head) with every n_sel in 0 .. 3 stride + 17 -- no clip at all, fewer clips than waves, tickets that end in the middle of a
round of the heads --, and the full grids of 256 workgroups (2 816 and 3 072 waves) at the bench's 65 536 clips and one more."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

SMALL = ((1, 1), (11, 11), (12, 12), (88, 11), (96, 12))           # (stride, waves per workgroup)
LARGE = ((2816, 11), (3072, 12))
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("g++")
    if not cxx:
        pytest.skip("needs a C++ compiler")
    exe = str(tmp_path_factory.mktemp("fast_ticket") / "fast_ticket_driver")
    # a plain program with its own main: the sanitizers are linked in, nothing is preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "fast_ticket", "fast_ticket_driver.cpp")])
    return exe


def deal(driver, mode, seed, stride, wpw, lo, hi):
    out = subprocess.run([driver, mode, str(seed), str(stride), str(wpw), str(lo), str(hi)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    last = out[-1].split()
    assert last[0] == "CASES" and last[2] == "FAIL", out[-3:]
    assert int(last[1]) == hi - lo + 1, out[-3:]
    assert int(last[3]) == 0, out[:8]


@pytest.mark.parametrize("mode", ("steps", "walk"))
@pytest.mark.parametrize("stride,wpw", SMALL)
def test_every_clip_once_every_wave_out_every_word_zero(driver, mode, stride, wpw):
    for seed in SEEDS:
        deal(driver, mode, seed, stride, wpw, 0, 3 * stride + 17)


@pytest.mark.parametrize("mode", ("steps", "walk"))
@pytest.mark.parametrize("stride,wpw", LARGE)
def test_full_grids_at_the_bench_batch_and_one_more(driver, mode, stride, wpw):
    for seed in SEEDS:
        deal(driver, mode, seed, stride, wpw, 65536, 65537)
