"""The matrices of tests/sweep_cases.py against the host analysis and the CPU oracle alone (no GPU): every case has two
wide big fronts below the root with the shapes that tests/test_gpu_big_fronts_below_root.py is written for, they sweep
as SK_BIG for batches below 16 and as SK_BLOCK from 16 on, and the high-precision substitution that the GPU tests use
as their reference agrees with the oracle's four sweeps."""
import numpy as np
import pytest

import pivot_cases as pc
import sweep_cases as sc
from helpers import RTOL, backward_error_ratio, backward_error_ratio_dense, lower_transposed, permuted

KINDS = ("lu", "chol")
BATCHES = (1, 2, 4, 15, 16, 50)
FRINGE = 40


def _handle(hip, name, kind, batch, fringe=0):
    m, n, Ap, Ai, _ = sc.case_matrix(name, symmetric=kind == "chol", fringe=fringe)
    return hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU, batch=batch)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_two_big_fronts_below_the_root(hip, name, kind, batch):
    with _handle(hip, name, kind, batch) as F:
        assert F.n == sc.ORDER[name]
        K = sc.solve_kinds(hip, F)
    wide = sc.wide_fronts(K)
    assert tuple((int(K.r[s]), int(K.w[s])) for s in wide) == sc.FRONTS[name]
    root = wide[-1]
    assert K.parent[root] == -1 and [int(K.parent[s]) for s in wide[:-1]] == [root, root]
    # both non-root fronts on one level: one launch group with count 2 (blockIdx.z > 0)
    assert all(K.parent[s] != t for s in wide[:-1] for t in wide[:-1])
    want = "big" if batch < 16 else "block"
    assert [K.kind[s] for s in wide] == [want] * 3
    # the factor classes (k_big_step alone and in a batch, k_front_wg from 48 matrices on)
    assert [K.cls[s] for s in wide] == ["wg" if batch >= 48 else "big_step"] * 3


@pytest.mark.parametrize("batch", (1, 4))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["w72", "w140"])
def test_fringe_feeds_small_fronts_into_a_big_front_below_the_root(hip, name, kind, batch):
    with _handle(hip, name, kind, batch, fringe=FRINGE) as F:
        K = sc.solve_kinds(hip, F)
    fed = [s for s in range(len(K.w)) if K.r[s] <= 32 and K.parent[s] >= 0 and K.kind[K.parent[s]] == "big"
           and K.parent[K.parent[s]] >= 0]
    assert len(fed) >= 1
    assert all(K.kind[s] == "small" for s in fed)
    below_root = [s for s in sc.wide_fronts(K) if K.parent[s] >= 0]
    assert len(below_root) >= 2 and all(K.kind[s] == "big" and K.r[s] > K.w[s] for s in below_root)


def _oracle_factors(orc, name, kind):
    m, n, Ap, Ai, Ax = sc.case_matrix(name, symmetric=kind == "chol")
    q = orc.csc_amd_f(1, n, n, Ap, Ai)
    if kind == "chol":
        Lp, Li, Lx = pc.oracle_chol(orc, n, Ap, Ai, Ax, q)
        return n, (Lp, Li, Lx), None
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, 1e-3)
    assert np.array_equal(pinv, np.argsort(q))
    return n, (Lp, Li, Lx), (Up, Ui, Ux)


def _right_hand_sides(n, k, seed):
    B = np.random.default_rng(seed).standard_normal((n, k))
    B[:, 1] *= 2.0 ** 200
    B[:, 2] *= 2.0 ** -200
    B[:, 3] = 0.0
    return B


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["w72", "w100"])
def test_substitute_agrees_with_the_oracles_sweeps(orc, name, kind):
    """substitute() on the oracle's own factors (columns in the oracle's order: only the diagonal's place is fixed)
    against cs_lsolve, cs_usolve, cs_ltsolve and cs_utsolve, per column."""
    n, L, U = _oracle_factors(orc, name, kind)
    B = _right_hand_sides(n, 5, seed=3)
    sweeps = [(L, True, False, orc.csc_lsolve_f), (L, True, True, orc.csc_ltsolve_f)]
    if U is not None:
        sweeps += [(U, False, False, orc.csc_usolve_f), (U, False, True, orc.csc_utsolve_f)]
    for G, lower, trans, fn in sweeps:
        X = sc.substitute(n, *G, B, lower, trans)
        assert X.dtype == np.longdouble and X.shape == B.shape
        for j in range(B.shape[1]):
            want = B[:, j].copy()
            fn(n, *G, want)
            scale = np.abs(want).max()
            assert np.abs(X[:, j] - want).max() <= RTOL * scale, (lower, trans, j)
            if j == 3:
                assert scale == 0.0 and not X[:, j].any()
        # ... and it solves the system it states, to the componentwise bound of a float64 substitution, far below it
        ratio = sc.substitution_error_ratio(sc.dense(n, *G, trans=trans), X, B)
        assert (ratio <= 1.0).all(), (lower, trans, ratio)


def test_substitution_error_ratio_sees_one_slightly_wrong_entry(orc):
    """A relative error of 1e-9 in one entry of x is far beyond the componentwise bound 2 n u."""
    n, L, _ = _oracle_factors(orc, "w72", "lu")
    B = _right_hand_sides(n, 4, seed=5)[:, :1]
    X = sc.substitute(n, *L, B, True, False).astype(np.float64)
    T = sc.dense(n, *L)
    assert sc.substitution_error_ratio(T, X, B)[0] <= 2 * n
    # the LAST entry feeds no other row, so its row of the residual is its own error alone
    X2 = X.copy()
    X2[n - 1] *= 1 + 1e-9
    assert sc.substitution_error_ratio(T, X2, B)[0] > 2 * n


@pytest.mark.parametrize("kind", KINDS)
def test_dense_backward_error_is_the_sparse_one(orc, kind):
    """helpers.backward_error_ratio_dense (exact float64 products of 21-bit pieces) against backward_error_ratio (one
    np.longdouble term per (i, k, j)) on the oracle's factors: both add about n terms in np.longdouble, 2^-11 u each."""
    n, L, U = _oracle_factors(orc, "w72", kind)
    m, n, Ap, Ai, Ax = sc.case_matrix("w72", symmetric=kind == "chol")
    A = permuted(n, Ap, Ai, Ax, orc.csc_amd_f(1, n, n, Ap, Ai))
    U = lower_transposed(n, L) if U is None else U
    want, bad = backward_error_ratio(n, A, L, U)
    got, bad_dense = backward_error_ratio_dense(n, A, L, U)
    assert bad == bad_dense == 0 and 1.0 < want <= 2 * n
    assert abs(got - want) <= 2 * n * 2.0 ** -11
    Lx = L[2].copy()
    Lx[np.argmin(np.abs(Lx))] *= 1 + 1e-9                          # 1e-9 relative on the smallest entry of L
    assert backward_error_ratio_dense(n, A, (L[0], L[1], Lx), U)[0] > 2 * n
