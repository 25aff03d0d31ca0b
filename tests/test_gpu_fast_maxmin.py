"""-m gpu: csrc/kws_fast_maxmin.h -- the single-instruction maximum / minimum helpers of the fast kernel's network half -- built into a stand-alone device
program (tests/fast_maxmin/fast_maxmin_driver.hip, its own main) and held against fmaxf / fminf on the GPU: every pairing of zeros of either sign,
subnormals, infinities, quiet NaNs (either operand, both) and the extreme normal numbers, and 4 096 x 90 pairs with random bit patterns.  The program
prints how many of its cases differ in a bit (two NaN results count as equal); none may.  Signalling NaNs are outside the helpers' contract and not fed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.gpu


def test_helpers_give_fmaxf_and_fminf_bits_on_the_device(tmp_path):
    exe = str(tmp_path / "fast_maxmin_driver")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "ei-keyword-spotting_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "fast_maxmin", "fast_maxmin_driver.hip")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True, timeout=120).stdout.splitlines()
    print("\n".join(out))
    last = out[-1].split()
    assert last[0] == "CASES" and last[2] == "MISMATCH", out[-3:]
    assert int(last[1]) >= 9 * 4000 * 80 and int(last[3]) == 0, out[-9:]
