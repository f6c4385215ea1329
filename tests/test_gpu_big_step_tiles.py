"""k_big_step's panel tiles give the bits they gave when each of them computed its full 64 x 64 tile.

Per case of tests/big_step_tile_cases.py (five matrices whose block widths and ragged tile extents end at and beside the
multiples of 16; LU and Cholesky; batches of 1 and 2): factor, read the factors back, run one fused refactor + solve, and
compare the SHA-256 of the bytes of Lx, Ux and x with tests/golden/big_step_tile_bits.json, which
tests/golden/make_big_step_tile_bits.py recorded from a build of the parent commit.  No tolerance: every entry's sum has
the same terms in the same order whichever wave forms it.  Each case first asserts from cs3_debug_launch_plan that its
plans hold BIG_BLOCK steps (big_step_tile_cases.record); tests/test_big_step_tile_cases_cpu.py pins the fronts."""
import json
import os

import pytest

import big_step_tile_cases as tc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_step_tile_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(tc.case_id(c) for c in tc.CASES)


@pytest.mark.parametrize("case", tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_bits_equal_the_parent_commit(gpu, case):
    got = tc.record(gpu, case)
    want = GOLDEN[tc.case_id(case)]
    for key in ("Lx", "Ux", "x"):
        assert got[key] == want[key], "%s: %s differs from the parent commit's bits (sum %s, recorded %s)" % (
            tc.case_id(case), key, got["sum_" + key], want["sum_" + key])
