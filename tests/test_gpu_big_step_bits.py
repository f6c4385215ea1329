"""k_big_step gives the bits it gave before its loads, addresses and copy-home were rearranged.

Per case of tests/big_step_bits_cases.py (three matrices of tests/wide_chunk_cases.py; LU and Cholesky; batches of 1, 2
and 7; one LU case with pivot perturbation on): factor, read the factors back, run one fused refactor + solve, and compare
the SHA-256 of the bytes of Lx, Ux and x with tests/golden/big_step_bits.json, which tests/golden/make_big_step_bits.py
recorded from a build of the parent commit.  No tolerance: the arithmetic and its order are the same, so every bit is.
Each case first asserts from cs3_debug_launch_plan that its plans hold BIG_BLOCK steps (big_step_bits_cases.record), so
none of them runs k_front_wg instead; every case does at every batch listed, none was dropped."""
import json
import os

import pytest

import big_step_bits_cases as bb

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_step_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(bb.case_id(c) for c in bb.CASES)


@pytest.mark.parametrize("case", bb.CASES, ids=[bb.case_id(c) for c in bb.CASES])
def test_bits_equal_the_parent_commit(gpu, case):
    got = bb.record(gpu, case)
    want = GOLDEN[bb.case_id(case)]
    for key in ("Lx", "Ux", "x"):
        assert got[key] == want[key], "%s: %s differs from the parent commit's bits (sum %s, recorded %s)" % (
            bb.case_id(case), key, got["sum_" + key], want["sum_" + key])
