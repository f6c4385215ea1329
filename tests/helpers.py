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


def _exact_pieces(A, axis, bits=21):
    """A = sum of the returned float64 matrices, exactly; every entry of a piece is an integer multiple of its row's
    (axis 1) or column's (axis 0) grid 2^(e - bits + 1), at most 2^(bits - 1) of them, where 2^e bounds what was left of
    that row or column.  (fl((x + sigma) - sigma) with sigma = 1.5 2^k rounds x to a multiple of 2^(k - 52).)"""
    pieces = []
    R = np.array(A, dtype=np.float64, copy=True)
    while R.any():
        assert len(pieces) < 32, "entries too far apart to split"
        e = np.frexp(np.abs(R).max(axis=axis, keepdims=True))[1]           # max < 2^e (0 for an empty row: its piece is 0)
        sigma = np.ldexp(1.5, e + 52 - bits + 1)
        P = (R + sigma) - sigma
        R = R - P                                                           # exact: P is R rounded to the grid
        pieces.append(P)
    return pieces


def backward_error_ratio_dense(n, A_perm, L, U):
    """backward_error_ratio for factors that are nearly dense (n of a few hundred), where one term per (i, k, j) is
    n^3 / 3 terms: L U is formed from float64 matrix products that are EXACT -- L's rows and U's columns are split into
    pieces of 21 bits (_exact_pieces), so that a sum of n <= 2048 products of two pieces fits 53 bits in any order --
    and the products are added up in np.longdouble, as the sparse form adds its terms.  |L||U| is a float64 product
    (relative error n u, on a ratio that is compared with 2 n)."""
    assert n <= 2048
    Ld = sp.csc_matrix((np.asarray(L[2], dtype=np.float64), np.asarray(L[1]), np.asarray(L[0])), shape=(n, n)).toarray()
    Ud = sp.csc_matrix((np.asarray(U[2], dtype=np.float64), np.asarray(U[1]), np.asarray(U[0])), shape=(n, n)).toarray()
    S = np.zeros((n, n), dtype=np.longdouble)
    for PL in _exact_pieces(Ld, axis=1):
        for PU in _exact_pieces(Ud, axis=0):
            S += PL @ PU
    E = np.abs(S - A_perm.toarray().astype(np.longdouble))
    W = np.abs(Ld) @ np.abs(Ud)
    zero = W == 0
    nz_bad = int(np.count_nonzero(E[zero] != 0))
    ratio = float((E[~zero] / (np.longdouble(U_ROUND) * W[~zero])).max()) if (~zero).any() else 0.0
    return ratio, nz_bad


def assert_backward_error(n, A_perm, L, U, what="", oracle_ratio=None, bound=None, dense=False):
    """Higham's componentwise bound for any LU (or Cholesky, U = L') computed in float64, in any summation order, with
    or without FMA:  |P A Q - L U|_ij <= gamma_n (|L||U|)_ij,  asserted as 2 n u (the factor 2 covers multipliers formed
    by a reciprocal multiply: one more rounding per entry of L), and exactly zero where (|L||U|)_ij = 0.  `bound`
    (in units of u) replaces 2 n by something sharper; `oracle_ratio` only goes into the message.  Returns the ratio
    max |E|_ij / (u (|L||U|)_ij).  dense: through backward_error_ratio_dense."""
    ratio, nz_bad = (backward_error_ratio_dense if dense else backward_error_ratio)(n, A_perm, L, U)
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
