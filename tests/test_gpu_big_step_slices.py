"""k_big_step's four column slices give the bits that the two-wave elimination gave.

Per case of tests/big_step_slice_cases.py (thirteen matrices whose last block ends at and beside the multiples of 8, below
the root and at the root; LU and Cholesky; batches of 1 and 2; two LU shapes again with pivot perturbation on and a delta
below every pivot): factor, read the factors back, run one fused refactor + solve, and compare the SHA-256 of the bytes of
Lx, Ux and x with tests/golden/big_step_slice_bits.json, which tests/golden/make_big_step_slice_bits.py recorded from a
build of the parent commit.  No tolerance: every entry sees the same multiplications and FMAs in the same order whichever
wave holds its column.  Each case first asserts from cs3_debug_launch_plan that its plans hold BIG_BLOCK steps
(big_step_slice_cases.record); tests/test_big_step_slice_cases_cpu.py pins the fronts."""
import json
import os

import pytest

import big_step_slice_cases as ss

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_step_slice_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(ss.case_id(c) for c in ss.CASES)


def test_the_perturbed_records_equal_the_plain_ones():
    # (a delta below every pivot replaces nothing: the PivotRule<true> instance recorded the bits of the plain one)
    for name in ss.PERTURBED:
        plain, pert = GOLDEN["%s-lu-b1" % name], GOLDEN["%s-lu-b1-perturb" % name]
        assert all(plain[k] == pert[k] for k in ("Lx", "Ux", "x"))


@pytest.mark.parametrize("case", ss.CASES, ids=[ss.case_id(c) for c in ss.CASES])
def test_bits_equal_the_parent_commit(gpu, case):
    got = ss.record(gpu, case)
    want = GOLDEN[ss.case_id(case)]
    for key in ("Lx", "Ux", "x"):
        assert got[key] == want[key], "%s: %s differs from the parent commit's bits (sum %s, recorded %s)" % (
            ss.case_id(case), key, got["sum_" + key], want["sum_" + key])
