"""The A operand of the syndrome MFMA in its three-step form (csrc/t3_host.cpp, build_mfma_syndrome), proved on the CPU.
tests/cpp/synd_operand3.cpp builds the B bytes as fx2_set (csrc/t3_decode_fx2.h) does -- one T entry per symbol and scrambler state,
then the trits of the lane's 13th symbol into byte 2 of step 0's dwords 0, 1, 2 -- forms the 32 rows' integer dot products over the three
steps, folds them mod 3 and compares with rs_syndromes (csrc/t3_rs_core.h) of the descrambled block, for k = 24, 22, 20, 18:

  single   every position 0..25 x symbol value 0..26 x scrambler state 0..2 on an otherwise zero block: 2,106 blocks
  random   100,000 seeded blocks of random coded symbols and states

and counts the rows whose partial sums leave [-78, 78] (the bias 64 and the fold tables of the kernels are sized for that range)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ternary-image-codec_amd", "csrc")


@pytest.fixture(scope="module")
def tallies(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("synd3") / "synd_operand3")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "synd_operand3.cpp"),
                    os.path.join(CSRC, "t3_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    t = json.loads(r.stdout)
    t["exit"] = r.returncode
    return t


@pytest.mark.parametrize("k", [24, 22, 20, 18])
def test_three_step_operand(tallies, k):
    t = tallies["k%d" % k]
    assert t["single"]["n"] == 26 * 27 * 3 and t["random"]["n"] == 100000
    for name in ("single", "random"):
        assert t[name]["mismatch"] == 0 and t[name]["out_of_range"] == 0, (k, name, t[name])


def test_program_exit_status(tallies):
    assert tallies["exit"] == 0
