"""Matching + scaling on the host (cs3_match_scale, cs3_analyze_matched, cs3_get_matching): no device needed.

The scaled matrix is rebuilt here with the header's product order and checked against its definition; the transversal's
weight against an independent solver (SciPy's min_weight_full_bipartite_matching on the same costs); and, with the
library's own pivot order q, the oracle's partial pivoting must keep every diagonal of B at tol = 1e-3 and 1e-2 -- the
condition every comparison of tests/test_gpu_matching.py rests on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import min_weight_full_bipartite_matching

import match_cases as mc
import pivot_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12               # |B| <= 1 and |B_jj| = 1 up to the rounding of exp / log
_i32p, _f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _match(hip, c):
    return hip.match_scale(c.n, c.Ap, c.Ai, c.Ax)


def _optimum(c):
    """The largest sum_j log |a_{sigma(j), j}| over all transversals, by SciPy.  (+1 on every cost: that function takes a
    stored zero for a missing edge; a full matching has n edges, so the shift is n.)"""
    keep = c.Ax != 0.0
    col = np.repeat(np.arange(c.n), np.diff(c.Ap))[keep]
    row, a = c.Ai[keep], np.abs(c.Ax[keep])
    cmax = np.zeros(c.n)
    np.maximum.at(cmax, col, a)
    cost = np.log(cmax[col]) - np.log(a)
    G = sp.coo_matrix((cost + 1.0, (row, col)), shape=(c.n, c.n)).tocsr()
    r, cc = min_weight_full_bipartite_matching(G)
    return float(np.log(cmax).sum() - (np.asarray(G[r, cc]).ravel() - 1.0).sum())


@pytest.fixture(scope="module")
def optimum():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _optimum(mc.case(name))
        return cache[name]
    return get


def test_the_cases_with_a_known_permutation_are_the_dominant_scrambles():
    assert tuple(k for k in mc.NAMES if mc.case(k).expect_rowperm is not None) == mc.KNOWN


# 1. the definition
@pytest.mark.parametrize("name", mc.NAMES)
def test_scaled_matrix_is_bounded_by_one_with_a_unit_diagonal(hip, name):
    c = mc.case(name)
    rowperm, dr, dc = _match(hip, c)
    assert np.array_equal(np.sort(rowperm), np.arange(c.n)), "rowperm is not a permutation"
    assert np.isfinite(dr).all() and np.isfinite(dc).all() and (dr > 0).all() and (dc > 0).all()
    Bp, Bi, Bx = mc.scaled(c, c.Ax, rowperm, dr, dc)
    col = np.repeat(np.arange(c.n), np.diff(c.Ap))
    on_diag = Bi == col
    assert np.count_nonzero(on_diag) == c.n
    big, dev = np.abs(Bx).max() - 1.0, np.abs(np.abs(Bx[on_diag]) - 1.0).max()
    print("%s: max |B| - 1 = %.2e, max ||B_jj| - 1| = %.2e" % (name, big, dev))
    assert big <= BOUND and dev <= BOUND


# 2. optimality
@pytest.mark.parametrize("name", mc.NAMES)
def test_transversal_has_the_largest_product(hip, optimum, name):
    c = mc.case(name)
    rowperm = _match(hip, c)[0]
    got, want = mc.weight(c, rowperm), optimum(name)
    print("%s: sum log |a| = %.12g, SciPy %.12g" % (name, got, want))
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want))
    if c.expect_rowperm is not None:
        assert np.array_equal(rowperm, c.expect_rowperm)


# 3. determinism, and rows in any order inside a column
@pytest.mark.parametrize("name", mc.NAMES)
def test_same_bits_every_run_and_unsorted_columns(hip, optimum, name):
    c = mc.case(name)
    a, b = _match(hip, c), _match(hip, c)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    s = mc.shuffled_columns(c)
    rowperm, dr, dc = _match(hip, s)
    want = optimum(name)
    assert abs(mc.weight(s, rowperm) - want) <= 1e-9 * max(1.0, abs(want))
    if c.expect_rowperm is not None:
        assert np.array_equal(rowperm, c.expect_rowperm)
    Bx = mc.scaled(s, s.Ax, rowperm, dr, dc)[2]
    assert np.abs(Bx).max() - 1.0 <= BOUND


# 4. errors
def _raw(hip, n, Ap, Ai, Ax, null=None):
    Ap, Ai, Ax = np.asarray(Ap, dtype=np.int32), np.asarray(Ai, dtype=np.int32), np.asarray(Ax, dtype=np.float64)
    rowperm, dr, dc = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    args = [Ap.ctypes.data_as(_i32p), Ai.ctypes.data_as(_i32p), Ax.ctypes.data_as(_f64p), rowperm.ctypes.data_as(_i32p),
            dr.ctypes.data_as(_f64p), dc.ctypes.data_as(_f64p)]
    if null is not None:
        args[null] = None
    rc = hip.lib().cs3_match_scale(n, *args)
    return rc, hip.lib().cs3_last_error().decode()


def test_structurally_singular_patterns_are_pivot_errors(hip):
    # an empty column; two columns whose only entry is in the same row
    rc, msg = _raw(hip, 3, [0, 1, 1, 2], [0, 2], [1.0, 1.0])
    assert rc == hip.CS3_ERR_PIVOT and "2 of 3" in msg
    rc, msg = _raw(hip, 3, [0, 1, 2, 4], [1, 1, 0, 2], [1.0, 2.0, 3.0, 4.0])
    assert rc == hip.CS3_ERR_PIVOT and "2 of 3" in msg
    with pytest.raises(hip.SingularMatrix):
        hip.match_scale(3, [0, 1, 1, 2], [0, 2], [1.0, 1.0])


def test_a_stored_zero_counts_as_absent(hip):
    # [[1, 1, 0], [0, 0.0, 1], [1, 0, 0]]: (1, 1) is a stored zero, so column 1 can only take row 0, column 0 then row 2
    Ap, Ai = [0, 2, 4, 5], [0, 2, 0, 1, 1]
    rowperm, dr, dc = hip.match_scale(3, Ap, Ai, [1.0, 1.0, 1.0, 0.0, 1.0])
    assert list(rowperm) == [2, 0, 1]
    # the only transversal of [[0, 1, 0], [1, 0, 0], [0, 0, x]] passes through x = 0.0
    rc, msg = _raw(hip, 3, [0, 1, 2, 3], [1, 0, 2], [1.0, 1.0, 0.0])
    assert rc == hip.CS3_ERR_PIVOT and "2 of 3" in msg
    assert _raw(hip, 3, [0, 1, 2, 3], [1, 0, 2], [1.0, 1.0, 1e-300])[0] == 0


def test_bad_arguments(hip):
    Ap, Ai = [0, 1, 2], [0, 1]
    assert _raw(hip, 2, Ap, Ai, [1.0, np.nan])[0] == hip.CS3_ERR_ARG
    assert _raw(hip, 2, Ap, Ai, [np.inf, 1.0])[0] == hip.CS3_ERR_ARG
    for k in range(6):
        assert _raw(hip, 2, Ap, Ai, [1.0, 1.0], null=k)[0] == hip.CS3_ERR_ARG, "null argument %d" % k
    assert _raw(hip, 2, [0, 1, 2], [0, 2], [1.0, 1.0])[0] == hip.CS3_ERR_ARG          # row index out of range
    assert _raw(hip, 2, [0, 2, 1], [0, 1], [1.0, 1.0])[0] == hip.CS3_ERR_ARG          # Ap not monotone
    # the pattern is checked before the values, the values before the transversal
    assert _raw(hip, 2, [0, 1, 2], [0, 2], [np.nan, 1.0])[0] == hip.CS3_ERR_ARG
    assert _raw(hip, 2, [0, 2, 2], [0, 1], [np.nan, 1.0])[0] == hip.CS3_ERR_ARG


def test_analyze_matched_reports_what_match_scale_reports(hip):
    c = mc.case("kkt400")
    h = C.c_void_p()
    lib = hip.lib()
    p = lambda a, t: a.ctypes.data_as(t)                                   # noqa: E731
    bad = c.Ax.copy()
    bad[7] = np.nan
    assert lib.cs3_analyze_matched(1, c.n, p(c.Ap, _i32p), p(c.Ai, _i32p), p(bad, _f64p), None, 1, C.byref(h)) == hip.CS3_ERR_ARG
    assert not h
    assert lib.cs3_analyze_matched(1, c.n, p(c.Ap, _i32p), p(c.Ai, _i32p), None, None, 1, C.byref(h)) == hip.CS3_ERR_ARG
    assert lib.cs3_analyze_matched(1, c.n, p(c.Ap, _i32p), p(c.Ai, _i32p), p(c.Ax, _f64p), None, 0, C.byref(h)) == hip.CS3_ERR_ARG
    zero = np.where(np.repeat(np.arange(c.n), np.diff(c.Ap)) == 3, 0.0, c.Ax)          # column 3 holds stored zeros only
    assert lib.cs3_analyze_matched(1, c.n, p(c.Ap, _i32p), p(c.Ai, _i32p), p(zero, _f64p), None, 1, C.byref(h)) == hip.CS3_ERR_PIVOT
    assert "%d of %d" % (c.n - 1, c.n) in lib.cs3_last_error().decode()


def test_get_matching_on_a_plain_handle_is_a_state_error(hip):
    c = mc.case("jac200")
    with hip.Factorization(c.n, c.n, c.Ap, c.Ai) as F:
        with pytest.raises(hip.Cs3Error) as e:
            F.matching()
        assert e.value.code == hip.CS3_ERR_STATE
        assert not F.matched


# 5. the matched analysis
@pytest.mark.parametrize("name", mc.NAMES)
def test_oracle_keeps_every_diagonal_of_the_scaled_matrix(hip, orc, name):
    c = mc.case(name)
    want = _match(hip, c)
    with hip.Factorization(c.n, c.n, c.Ap, c.Ai, batch=c.batch, match_values=c.Ax) as F:
        assert F.matched
        got = F.matching()
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes()
        assert F.match_time > 0.0
        q = F.ordering()["q"]
        info = F.info
        FR = pc.fronts(hip, F)
    assert info.n == c.n and info.nnz_a == len(c.Ax) and info.batch == c.batch
    for cls in c.classes:
        assert cls in FR.cls, "%s no longer reaches %s" % (name, cls)
    values = mc.batch_values(c) if c.batch > 1 else c.Ax[None, :]
    for Ax in values:
        Bp, Bi, Bx = mc.scaled(c, Ax, *got)
        for tol in (1e-3, 1e-2):
            assert pc.first_off_diagonal(orc, c.n, Bp, Bi, Bx, q, tol) is None, "%s: tol %g" % (name, tol)


def test_analysis_is_the_plain_analysis_of_the_permuted_pattern(hip):
    """A matched handle analyses (Ap, rowinv[Ai]); order and q_given apply to B."""
    c = mc.case("kkt400")
    rowperm = _match(hip, c)[0]
    Bi = np.argsort(rowperm).astype(np.int32)[c.Ai]
    with hip.Factorization(c.n, c.n, c.Ap, c.Ai, match_values=c.Ax) as F, hip.Factorization(c.n, c.n, c.Ap, Bi) as P:
        fo, po = F.ordering(), P.ordering()
        for k in fo:
            assert np.array_equal(fo[k], po[k]), k
        for a, b in zip(F.factors(values=False), P.factors(values=False)):
            assert a is b or np.array_equal(a, b)
    q = np.random.default_rng(3).permutation(c.n).astype(np.int32)
    with hip.Factorization(c.n, c.n, c.Ap, c.Ai, q=q, match_values=c.Ax) as F:
        assert np.array_equal(F.ordering()["q_amd"], q)
    with pytest.raises(AssertionError):
        hip.Factorization(c.n, c.n, c.Ap, c.Ai, kind=hip.CS3_CHOLESKY, match_values=c.Ax)


def test_cscmat_keeps_matched_and_plain_analyses_apart(hip):
    from csparse3_amd.csc import CscMat
    c = mc.case("kkt400")
    A = CscMat(c.n, c.n, indptr=c.Ap, indices=c.Ai, data=c.Ax.copy())
    F = A._analysis(hip.CS3_LU, hip.ORDER_AMD, None, True)
    assert F.matched and A._analysis(hip.CS3_LU, hip.ORDER_AMD, None, True) is F
    rowperm = F.matching()[0].copy()
    A.data *= 1.5                                                            # new values, same pattern: the matching is kept
    assert A._analysis(hip.CS3_LU, hip.ORDER_AMD, None, True) is F and np.array_equal(F.matching()[0], rowperm)
    P = A._analysis(hip.CS3_LU, hip.ORDER_AMD, None, False)
    assert P is not F and not P.matched
    P.close()


# 6. header
def test_matching_symbols_are_declared_and_exported(hip):
    header = open(os.path.join(ROOT, "include", "csparse3_amd.h")).read()
    names = set(re.findall(r"\b(cs3_[a-z0-9_]+)\s*\(", header))
    for name in ("cs3_match_scale", "cs3_analyze_matched", "cs3_get_matching"):
        assert name in names, name + " is not declared in the header"
        assert hasattr(hip.lib(), name), "libcsparse3_hip.so does not export " + name
