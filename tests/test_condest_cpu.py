"""Condition estimates and log-determinants without a GPU: the NumPy port of dlacn2 (tests/lacn2_ref.py) against LAPACK
itself (SciPy's dgecon, which calls dlacn2), and the argument and state errors of the new entry points, which come before
anything touches the device (null Ax / cond first, then a missing factorisation)."""
import numpy as np
import pytest
import scipy.linalg as sla
from scipy.linalg import lapack

from csparse3_amd import synth
from lacn2_ref import lacn2


def test_port_matches_lapack_dgecon():
    """>= 200 seeded dense matrices, n = 2 .. 60, some badly conditioned: the port driven by the same LU as dgecon gives
    1 / (anorm * rcond) within 1e-12 and never exceeds the exact ||A^-1||_1."""
    rng = np.random.default_rng(2024)
    nsolves = set()
    for t in range(240):
        n = int(rng.integers(2, 61))
        A = rng.standard_normal((n, n))
        if t % 3 == 1:
            A[:, 0] = A[:, 1] * (1.0 + 1e-6 * rng.standard_normal(n))          # nearly singular
        elif t % 3 == 2:
            A += n * np.eye(n)                                                  # well conditioned
        lu = sla.lu_factor(A)
        anorm = np.abs(A).sum(axis=0).max()
        rcond, info = lapack.dgecon(lu[0], anorm, norm="1")
        assert info == 0
        est, k = lacn2(n, lambda b: sla.lu_solve(lu, b), lambda b: sla.lu_solve(lu, b, trans=1))
        nsolves.add(k)
        want = 1.0 / (anorm * rcond)
        assert abs(est - want) <= 1e-12 * want, "t=%d n=%d: %.17g vs dgecon %.17g" % (t, n, est, want)
        exact = np.abs(np.linalg.inv(A)).sum(axis=0).max()
        assert est <= exact * (1.0 + 1e-12), "t=%d: estimate above the norm" % t
    assert nsolves >= {4, 5}, nsolves


def test_port_edge_cases():
    assert lacn2(0, None, None) == (0.0, 0)
    est, k = lacn2(1, lambda b: b / -4.0, lambda b: b / -4.0)
    assert (est, k) == (0.25, 1)
    est, k = lacn2(3, lambda b: b * np.nan, lambda b: b)
    assert est == np.inf and k == 1


def _handles(hip):
    m, n, Ap, Ai, Ax, b, xt = synth.toy10()
    yield hip.Factorization(m, n, Ap, Ai), Ax
    ei, ej = synth.spd_grid_pattern(60, seed=1)
    m, n, Ap, Ai, Ax = synth.spd_grid_matrix(60, ei, ej, seed=2)
    yield hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY, batch=3), np.tile(Ax, 3)


def test_before_a_factorisation_every_form_is_a_state_error(hip):
    for F, Ax in _handles(hip):
        with F:
            for call in (lambda: F.condest(Ax), lambda: F.condest_dev(8, 8), lambda: F.condest_dev(8, 8, 8),
                         lambda: F.slogdet(), lambda: F.slogdet_dev(8, 8)):
                with pytest.raises(hip.Cs3Error) as e:
                    call()
                assert e.value.code == hip.CS3_ERR_STATE, str(e.value)


def test_null_arguments_are_checked_first(hip):
    for F, Ax in _handles(hip):
        with F:
            for call in (lambda: F.condest_dev(0, 8), lambda: F.condest_dev(8, 0), lambda: F.condest_dev(0, 0, 8),
                         lambda: F.slogdet_dev(0, 8), lambda: F.slogdet_dev(8, 0)):
                with pytest.raises(hip.Cs3Error) as e:
                    call()
                assert e.value.code == hip.CS3_ERR_ARG, str(e.value)
