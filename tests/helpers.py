"""Shared comparison helpers for the parity tests."""
import numpy as np
import scipy.sparse as sp

RTOL = 1e-10   # BASELINE.json north_star: factors and solutions within 1e-10 relative


def canon(n, Gp, Gi, Gx):
    """Row-sorted copy of a CSC triple (the oracle's columns are in DFS order)."""
    G = sp.csc_matrix((np.asarray(Gx, dtype=np.float64), np.asarray(Gi), np.asarray(Gp)), shape=(n, n))
    G.sort_indices()
    return G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data.copy()


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 1.0
    if scale == 0.0:
        scale = 1.0
    return float(np.abs(got - want).max() / scale) if want.size else 0.0


def assert_factor_equal(n, got, want, what):
    """Pattern bit-exact, values within RTOL (norm-wise) of the oracle."""
    gp, gi, gx = canon(n, *got)
    wp, wi, wx = canon(n, *want)
    assert np.array_equal(gp, wp), what + ": column pointers differ"
    assert np.array_equal(gi, wi), what + ": row indices differ"
    err = rel_err(gx, wx)
    assert err <= RTOL, "%s: relative error %.3e > %.1e" % (what, err, RTOL)
    return err


def csc_to_scipy(m, n, Ap, Ai, Ax):
    return sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))


def symmetrized(n, Ap, Ai):
    A = sp.csc_matrix((np.ones(Ap[n]), Ai[:Ap[n]], Ap), shape=(n, n))
    S = (A + A.T).tocsc()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32)


def permuted(n, Ap, Ai, Ax, q):
    """P A Q for the static pivot order q (rows and columns both taken in the order q): entry (k, l) is A[q[k], q[l]]."""
    A = csc_to_scipy(n, n, Ap, Ai[:Ap[n]], Ax[:Ap[n]]).tocsr()[q][:, q].tocsc()
    A.sort_indices()
    return A


U_ROUND = 2.0 ** -53   # unit roundoff of float64


def backward_error_ratio(n, A_perm, L, U):
    """max_ij |P A Q - L U|_ij / (u (|L||U|)_ij) over the entries with (|L||U|)_ij > 0, and the number of entries
    where (|L||U|)_ij == 0 but (P A Q)_ij != 0.  Every product L_ik U_kj is formed and summed in np.longdouble (64-bit
    mantissa: the reference's own rounding is 2^-11 of the unit it measures), one term per (i, k, j), grouped by (i, j)."""
    Lp, Li, Lx = canon(n, *L)
    Up, Ui, Ux = canon(n, *U)
    ucol = np.repeat(np.arange(n, dtype=np.int64), np.diff(Up))
    cnt = (Lp[1:] - Lp[:-1])[Ui].astype(np.int64)              # entries of L's column k for every U(k, j)
    start = np.zeros(len(cnt) + 1, dtype=np.int64)
    np.cumsum(cnt, out=start[1:])
    rep = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    lidx = Lp[Ui][rep].astype(np.int64) + (np.arange(start[-1], dtype=np.int64) - start[rep])
    key = Li[lidx].astype(np.int64) + ucol[rep] * n
    prod = Lx[lidx].astype(np.longdouble) * Ux[rep].astype(np.longdouble)
    A = A_perm.tocoo()
    key = np.concatenate([key, A.row.astype(np.int64) + A.col.astype(np.int64) * n])
    val = np.concatenate([prod, -A.data.astype(np.longdouble)])
    mag = np.concatenate([np.abs(prod), np.zeros(A.nnz, dtype=np.longdouble)])
    order = np.argsort(key, kind="stable")
    key, val, mag = key[order], val[order], mag[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    E = np.abs(np.add.reduceat(val, first))
    W = np.add.reduceat(mag, first)
    zero = W == 0
    nz_bad = int(np.count_nonzero(E[zero] != 0))
    ratio = float((E[~zero] / (np.longdouble(U_ROUND) * W[~zero])).max()) if (~zero).any() else 0.0
    return ratio, nz_bad


def assert_backward_error(n, A_perm, L, U, what="", oracle_ratio=None, bound=None):
    """Higham's componentwise bound for any LU (or Cholesky, U = L') computed in float64, in any summation order, with
    or without FMA:  |P A Q - L U|_ij <= gamma_n (|L||U|)_ij,  asserted as 2 n u (the factor 2 covers multipliers formed
    by a reciprocal multiply: one more rounding per entry of L), and exactly zero where (|L||U|)_ij = 0.  `bound`
    (in units of u) replaces 2 n by something sharper; `oracle_ratio` only goes into the message.  Returns the ratio
    max |E|_ij / (u (|L||U|)_ij)."""
    ratio, nz_bad = backward_error_ratio(n, A_perm, L, U)
    lim = 2.0 * n if bound is None else bound
    note = "" if oracle_ratio is None else " (oracle %.2f)" % oracle_ratio
    assert nz_bad == 0, "%s: %d entries of P A Q outside the pattern of |L||U|" % (what, nz_bad)
    assert ratio <= lim, "%s: max |PAQ - LU| / (u |L||U|) = %.2f%s > %.1f" % (what, ratio, note, lim)
    return ratio


def lower_transposed(n, L):
    """U = L' as a CSC triple (the Cholesky form of assert_backward_error)."""
    Lp, Li, Lx = canon(n, *L)
    T = sp.csc_matrix((Lx, Li, Lp), shape=(n, n)).T.tocsc()
    T.sort_indices()
    return T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()
