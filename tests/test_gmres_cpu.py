"""GMRES refinement on held factors, what the CPU can say: the NumPy reference (tests/gmres_ref.py) on the engineered cases
of tests/gmres_cases.py, and the argument checks of the C ABI, which need no device.

Measured with this file (scipy's splu of A0 as the solve): on diag_case(300, 7, r) the reference needs r iterations from
x0 = M^-1 b and r + 1 from x0 = 0; the stationary corrections grow about 3.5 x per round; GMRES(2) on r = 3 takes 6
iterations and GMRES(3) on r = 5 takes 8; the recurrence's residual and the true one differ by at most 2.0e-16 (relative
to ||b||) at the end of a cycle."""
import ctypes as C
import inspect

import numpy as np
import pytest

import gmres_cases as gc
from csparse3_amd import csc, csc_hip


@pytest.mark.parametrize("r", [1, 3, 5])
def test_reference_ends_in_r_iterations_where_the_stationary_rounds_grow(r):
    case = gc.diag_case(300, 7, r)
    warm = gc.reference(case)
    assert warm.iters == r and warm.relres <= 1e-12
    cold = gc.reference(case, x0=np.zeros(300))
    assert cold.iters == r + 1 and cold.relres <= 1e-12
    want = np.linalg.solve(case.A.toarray(), case.b)
    for res in (warm, cold):
        assert np.abs(res.x - want).max() <= 1e-10 * np.abs(want).max()
    corr = gc.stationary_corrections(case, 6)
    print("r=%d stationary corrections %s" % (r, ["%.2e" % c for c in corr]))
    assert all(b > a for a, b in zip(corr, corr[1:])), corr


@pytest.mark.parametrize("r,restart", gc.RESTART_CASES)
def test_reference_restart_cases_have_a_count_that_rounding_cannot_move(r, restart):
    rc = gc.restart_case(r, restart)
    print("r=%d restart=%d history %s rtol %.3e iters %d" % (r, restart, ["%.2e" % h for h in rc.history], rc.rtol, rc.iters))
    assert rc.iters > restart, "the case must restart"
    assert rc.ref.relres <= rc.rtol
    below = [h for h in rc.ref.history if h <= rc.rtol]
    above = [h for h in rc.ref.history if h > rc.rtol]
    assert below and min(above) >= 3.0 * rc.rtol and max(below) <= rc.rtol / 3.0
    # monotone, restarts included
    assert all(b <= a * (1 + 1e-12) for a, b in zip(rc.ref.history, rc.ref.history[1:]))


def test_reference_recurrence_agrees_with_the_true_residual():
    gap = gc.reference_gap()
    print("reference: max |estimate - true| / ||b|| at a cycle's end = %.3e" % gap)
    assert 0.0 < gap <= 1e-14


def test_reference_special_cases():
    case = gc.diag_case(300, 7, 3)
    zero = gc.reference(case, b=np.zeros(300), x0=np.ones(300))
    assert zero.iters == 0 and zero.relres == 0.0 and not zero.x.any()
    x = np.linalg.solve(case.A.toarray(), case.b)
    done = gc.reference(case, x0=x)
    assert done.iters == 0 and np.array_equal(done.x, x)
    b = case.b.copy()
    b[5] = np.nan
    bad = gc.reference(case, b=b, x0=np.zeros(300))
    assert bad.iters == 0 and np.isnan(bad.relres)
    short = gc.reference(case, max_iters=2)
    assert short.iters == 2 and short.relres > 1e-12


# ---- the C ABI without a device ---------------------------------------------------------------------------------------

def test_limits():
    lim = csc_hip.gmres_limits()
    assert (lim.max_restart, lim.rhs_tile) == (32, 64)
    assert lim.chunk_rows >= 256 and lim.chunk_rows % 256 == 0
    assert csc_hip.lib().cs3_gmres_limits(None) == csc_hip.CS3_ERR_ARG


def _call(h, Ax, B, X, k=1, restart=30, max_iters=10, rtol=1e-12, trans=0):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    return csc_hip.lib().cs3_gmres(h, p(Ax), p(B), p(X), k, restart, max_iters, rtol, trans, None, None)


def test_argument_checks_need_no_device():
    case = gc.diag_case(300, 7, 1)
    m, n, Ap, Ai, Ax = case.mat
    b, x = case.b.copy(), np.zeros(n)
    ARG, STATE = csc_hip.CS3_ERR_ARG, csc_hip.CS3_ERR_STATE
    with csc_hip.Factorization(m, n, Ap, Ai) as F:
        h = F._h
        assert _call(None, Ax, b, x) == ARG
        assert _call(h, None, b, x) == ARG
        assert _call(h, Ax, None, x) == ARG
        assert _call(h, Ax, b, None) == ARG
        assert _call(h, Ax, b, x, k=0) == ARG
        assert _call(h, Ax, b, x, restart=0) == ARG
        assert _call(h, Ax, b, x, restart=csc_hip.gmres_limits().max_restart + 1) == ARG
        assert _call(h, Ax, b, x, max_iters=-1) == ARG
        for rtol in (-1e-3, np.inf, np.nan):
            assert _call(h, Ax, b, x, rtol=rtol) == ARG
        # valid arguments, no factorisation yet
        assert _call(h, Ax, b, x) == STATE
        assert _call(h, Ax, b, x, restart=1, max_iters=0, rtol=0.0, trans=1) == STATE
        dev = csc_hip.lib().cs3_gmres_dev
        assert dev(h, None, None, None, 1, 30, 10, 1e-12, 0, None, None, None) == ARG
        # the basis diagnostic: a bad pointer or count first, then "no gmres call yet"
        basis = csc_hip.lib().cs3_debug_gmres_basis
        buf = np.zeros(n)
        pv = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert basis(None, pv, 1) == ARG
        assert basis(h, None, 1) == ARG
        assert basis(h, pv, -1) == ARG
        assert basis(h, pv, csc_hip.gmres_limits().max_restart + 2) == ARG
        assert basis(h, pv, 0) == STATE and basis(h, pv, 1) == STATE
        assert basis(h, pv, csc_hip.gmres_limits().max_restart + 1) == STATE
        assert "no cs3_gmres call" in csc_hip.lib().cs3_last_error().decode()
    with csc_hip.Factorization(m, n, Ap, Ai, schur=[0, 1]) as S:
        assert _call(S._h, Ax, b, x) == ARG
        assert "Schur" in csc_hip.lib().cs3_last_error().decode()


def test_stationary_refinement_is_the_default_everywhere():
    for fn in (csc_hip.Factorization.solve_refined, csc_hip.csc_lusol_f, csc.CscMat.solve, csc.lusol):
        p = inspect.signature(fn).parameters
        assert p["refine"].default == "stationary", fn
        assert list(p)[-1] == "refine", "%s: refine is appended, nothing reordered" % fn
