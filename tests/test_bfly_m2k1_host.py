"""No GPU: csrc/kws_bfly_m2k1.h -- the m = 2, k = 1 radix-4 butterfly of the fast kernel's pass loop, written with the structure of its three twiddles
(six products instead of twelve) -- compiled for the host (tests/bfly_m2k1/bfly_m2k1_driver.cpp) and compared BIT FOR BIT with the plain kf_bfly4 and
the table's twiddles: the substitution must not move a bit of any output, the sign of a zero included.  The identity rests on the bit patterns of
KissFFT's table, which are asserted here too."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("g++")
    if not cxx:
        pytest.skip("needs a C++ compiler")
    exe = str(tmp_path_factory.mktemp("bfly_m2k1") / "bfly_m2k1_driver")
    # a plain program with its own main: the sanitizers are linked in, nothing is preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bfly_m2k1", "bfly_m2k1_driver.cpp")])
    return exe


def run(driver, *args):
    return subprocess.run([driver] + [str(a) for a in args], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()


def counts(lines):
    last = lines[-1].split()
    assert last[0] == "CASES" and last[2] == "MISMATCH", lines[-3:]
    return int(last[1]), int(last[3])


def test_the_table_has_the_bit_patterns_the_identity_rests_on(driver):
    out = run(driver, "table")
    tw = {int(t[1]): (t[2], t[3]) for t in (ln.split() for ln in out) if t[0] == "TW"}
    # cos / sin in double, cast to float (kiss_fft.cpp:351-357): (c, -c), (e, -1), (-c, -c) with one and the same c
    assert tw == {16: ("3f3504f3", "bf3504f3"), 32: ("248d3132", "bf800000"), 48: ("bf3504f3", "bf3504f3")}
    assert "OK 1" in out                            # what the fast plan checks before it lets the table reach the helper
    assert "REJECT 5 of 5" in out                   # ... and a table one bit off in a component the identity rests on is refused


def test_random_inputs_over_38_decades_give_the_plain_butterflys_bits(driver):
    out = run(driver, "random", 20250, 1200000)
    n, bad = counts(out)
    assert n >= 1000000 and bad == 0, out[-9:]


def test_zeros_of_either_sign_subnormals_and_infinities_give_the_plain_butterflys_bits(driver):
    """every +-0 combination, points with one zero component, subnormals, +-inf (two NaNs count as equal: payloads are not part of the claim)"""
    out = run(driver, "special")
    n, bad = counts(out)
    assert n >= 1000000 and bad == 0, out[-9:]
