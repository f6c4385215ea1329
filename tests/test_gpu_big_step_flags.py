"""k_big_step reports a rejected pivot once per lane, behind its stores: every place where it checks one, on both sides.

The cases come from tests/big_step_flag_cases.py (pinned from the host analysis by tests/test_big_step_flag_cases_cpu.py):
a multiplier at the threshold in the diagonal tile (both column halves, a full and the partial block) and in a
block-column tile (upper and lower 32 rows, both halves, a partial tile); the pivot itself (exact zero, 1e301, a Cholesky
pivot of -+ 1e-6 a); two failures of one launch in different tiles, either order; two failures of ONE lane (the case that
tells the smallest column from the last one met); a NaN in A; a batch of 2 with one matrix failing.  The matrix is
accepted at tol = rho (1 - 1e-6) with the oracle's factors and rejected at tol = rho (1 + 1e-6) with fail_col equal to the
oracle's first off-diagonal pivot.  One handle per (matrix, kind, batch) for the whole module."""
import numpy as np
import pytest

import big_step_flag_cases as bc
import pivot_cases as pc
from helpers import assert_factor_equal, csc_to_scipy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(gpu):
    held = {}

    def get(name=bc.LU, batch=1):
        if (name, batch) not in held:
            m, n, Ap, Ai, _ = pc.matrix(name[0])
            held[name, batch] = gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_LU if name == bc.LU else gpu.CS3_CHOLESKY, batch=batch)
        return held[name, batch]

    yield get
    for F in held.values():
        F.close()


def _residual_ok(mat, Ax, x, b):
    m, n, Ap, Ai, _ = mat
    A = csc_to_scipy(m, n, Ap, Ai, Ax)
    return np.abs(A @ x - b).max() <= 1e-12 * (abs(A).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max())


def _accepted_with_the_oracles_factors(orc, F, mat, q, Ax, tol, what):
    m, n, Ap, Ai, _ = mat
    F.factor(Ax, tol)
    assert F.info.fail_col == -1, what
    Lp, Li, Lx, Up, Ui, Ux = F.factors()
    oL = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, tol)
    assert np.array_equal(oL[6], np.argsort(q)), what + ": the oracle left the diagonal"
    assert_factor_equal(n, (Lp, Li, Lx), oL[0:3], what + " L")
    assert_factor_equal(n, (Up, Ui, Ux), oL[3:6], what + " U")


def _rejected_at(gpu, orc, F, mat, q, Ax, tol, k, what):
    m, n, Ap, Ai, _ = mat
    assert pc.first_off_diagonal(orc, n, Ap, Ai, Ax, q, tol) == k, what
    with pytest.raises(gpu.SingularMatrix):
        F.factor(Ax, tol)
    assert F.info.fail_col == k, "%s: fail_col %d, the oracle's first off-diagonal pivot is %d" % (what, F.info.fail_col, k)


@pytest.mark.parametrize("label", list(bc.MULTIPLIER_SITES), ids=[s.replace(" ", "_") for s in bc.MULTIPLIER_SITES])
def test_multiplier_at_the_threshold(gpu, orc, handles, label):
    mat, FR, s = bc.analysis(gpu)
    p = bc.multiplier_cases(gpu, orc)[label]
    assert p.rho is not None and p.weight >= pc.MIN_WEIGHT, "pivot_cases keeps no target for " + label
    F = handles()
    _accepted_with_the_oracles_factors(orc, F, mat, FR.q, p.Ax, p.rho * (1 - pc.MARGIN), label)
    _rejected_at(gpu, orc, F, mat, FR.q, p.Ax, p.rho * (1 + pc.MARGIN), p.target.k, label)
    _accepted_with_the_oracles_factors(orc, F, mat, FR.q, p.Ax, p.rho * (1 - pc.MARGIN), label + " again")


TWO = [("pair", label) for label in bc.PAIR_SITES] + [("lane", label) for label in bc.ONE_LANE_SITES]


@pytest.mark.parametrize("which,label", TWO, ids=[label.replace(" ", "_") for _, label in TWO])
def test_two_failures_in_one_launch_report_the_smaller_column(gpu, orc, handles, which, label):
    """pair: one failure in the diagonal tile and one in a block-column tile, the smaller column in either.  lane: one row
    fails at two columns that one lane holds, and no other lane sees the smaller one."""
    mat, FR, s = bc.analysis(gpu)
    t1, t2, Ax2, tol = (bc.pair_cases(gpu, orc) if which == "pair" else bc.one_lane_cases(gpu, orc))[label]
    F = handles()
    _accepted_with_the_oracles_factors(orc, F, mat, FR.q, Ax2, pc.RHOS[0] * (1 - pc.MARGIN), label)
    _rejected_at(gpu, orc, F, mat, FR.q, Ax2, tol, t1.k, label)


@pytest.mark.parametrize("site", range(len(bc.DIAGONAL_SITES)), ids=["b%d_c%d" % bj for bj in bc.DIAGONAL_SITES])
def test_the_pivot_itself_lu(gpu, orc, handles, site):
    """An exact zero and a value of 1e301 on the diagonal are rejected at their column, whatever the tolerance."""
    mat, FR, s = bc.analysis(gpu)
    m, n, Ap, Ai, Ax = mat
    k = bc.diagonal_columns(FR, s)[site]
    F = handles()
    for tol in (1e-3, 0.0):
        for what, bad in (("zero", bc.with_zero_column(Ap, Ai, Ax, FR.q, k)), ("1e301", bc.with_entry(Ap, Ai, Ax, FR.q, k, k, 1e301))):
            with pytest.raises(gpu.SingularMatrix):
                F.factor(bad, tol)
            assert F.info.fail_col == k, (what, tol, F.info.fail_col)
    _accepted_with_the_oracles_factors(orc, F, mat, FR.q, Ax, 1e-3, "the handle recovers")


@pytest.mark.parametrize("site", range(len(bc.DIAGONAL_SITES)), ids=["b%d_c%d" % bj for bj in bc.DIAGONAL_SITES])
def test_the_pivot_itself_cholesky(gpu, orc, handles, site):
    """A pivot of -1e-6 a is reported at its column; one of +1e-6 a is accepted there and the oracle's next step fails
    (the last pivot has none: accepted, with the oracle's L)."""
    mat, FR, s = bc.analysis(gpu, bc.CHOL)
    m, n, Ap, Ai, Ax = mat
    k = bc.diagonal_columns(FR, s)[site]
    F = handles(bc.CHOL)
    neg = pc.engineer_chol(orc, n, Ap, Ai, Ax, FR.q, k, -1.0)
    assert pc.chol_fail_step(orc, n, Ap, Ai, neg, FR.q) == k
    with pytest.raises(gpu.NotPositiveDefinite):
        F.factor(neg)
    assert F.info.fail_col == k
    pos = pc.engineer_chol(orc, n, Ap, Ai, Ax, FR.q, k, +1.0)
    later = pc.chol_fail_step(orc, n, Ap, Ai, pos, FR.q)
    if later is None:
        assert k == n - 1
    else:
        with pytest.raises(gpu.NotPositiveDefinite):
            F.factor(pos)
        assert F.info.fail_col == later
    good = pos if later is None else Ax
    F.factor(good)
    assert F.info.fail_col == -1
    assert_factor_equal(n, F.factors()[:3], pc.oracle_chol(orc, n, Ap, Ai, good, FR.q), "cholesky L")


@pytest.mark.parametrize("label", ["pivot", "diag", "col"])
def test_a_nan_that_reaches_the_big_front_is_rejected_at_its_column(gpu, orc, handles, label):
    mat, FR, s = bc.analysis(gpu)
    m, n, Ap, Ai, Ax = mat
    k, i = bc.nan_entries(FR, Ap, Ai, s)[label]
    F = handles()
    for tol in (1e-3, 0.0):
        with pytest.raises(gpu.SingularMatrix):
            F.factor(bc.with_entry(Ap, Ai, Ax, FR.q, i, k, np.nan), tol)
        assert F.info.fail_col == k, (label, tol, F.info.fail_col)
    _accepted_with_the_oracles_factors(orc, F, mat, FR.q, Ax, 1e-3, "the handle recovers")


@pytest.mark.parametrize("slot", [0, 1])
def test_batch_of_two_one_matrix_failing(gpu, orc, handles, slot):
    """The chain path with two matrices per launch (blockIdx.z): the failing one in either slot, its neighbour benign."""
    mat, FR, s = bc.analysis(gpu, bc.LU, 2)
    m, n, Ap, Ai, Ax = mat
    assert FR.cls[s] == "big_step" and FR.batch == 2
    F = handles(bc.LU, 2)
    b = np.random.default_rng(slot).standard_normal((2, n, 1))
    for label in ("diag hi", "col lower lo"):
        p = bc.multiplier_cases(gpu, orc)[label]
        AX = np.stack([1.5 * Ax, 1.5 * Ax])
        AX[slot] = p.Ax
        F.factor(AX, p.rho * (1 - pc.MARGIN))
        assert F.info.fail_col == -1
        oL = orc.csc_lu_f(n, n, Ap, Ai, p.Ax, FR.q, p.rho * (1 - pc.MARGIN))
        got = F.factors(b=slot)
        assert_factor_equal(n, got[0:3], oL[0:3], label + " L")
        assert_factor_equal(n, got[3:6], oL[3:6], label + " U")
        x = F.solve(b)
        assert _residual_ok(mat, p.Ax, x[slot, :, 0], b[slot, :, 0]) and _residual_ok(mat, AX[1 - slot], x[1 - slot, :, 0], b[1 - slot, :, 0])
        with pytest.raises(gpu.SingularMatrix):
            F.factor(AX, p.rho * (1 + pc.MARGIN))
        assert F.info.fail_col == p.target.k, (label, slot)
    F.factor(np.stack([Ax, 1.5 * Ax]), 1e-3)
    assert F.info.fail_col == -1
