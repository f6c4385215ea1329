"""NumPy / SciPy reference of the low-rank-modified solves (cs3_updates_*): the Sherman-Morrison-Woodbury formula exactly
as include/csparse3_amd.h states it, with A^-1 by SuperLU and S_c by scipy.linalg.lu (LAPACK partial pivoting: largest
|.|, ties to the lowest row), plus the case builders the tests share.

A case is (rows, cols, vals): the triplets of dA_c, duplicates adding."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def delta_matrix(n, case):
    rows, cols, vals = case
    return sp.coo_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=(n, n)).tocsc()


def direct_solve(A, case, b):
    """x = (A + dA_c)^-1 b by a factorisation of the modified matrix: the definition."""
    return spla.splu((A + delta_matrix(A.shape[0], case)).tocsc()).solve(b)


def capacitance(Zcols, rows_all, case):
    """(R, C, D, S) of one case; Zcols[:, k] = A^-1 e_{rows_all[k]}."""
    rows, cols, vals = (np.asarray(a) for a in case)
    R, ri = np.unique(rows, return_inverse=True)
    Cc, ci = np.unique(cols, return_inverse=True)
    D = np.zeros((len(R), len(Cc)))
    np.add.at(D, (ri, ci), np.asarray(vals, dtype=np.float64))
    where = np.searchsorted(rows_all, R)
    G = Zcols[np.ix_(Cc, where)]
    return R, Cc, D, np.eye(len(R)) + D @ G, where


def solve_updates_ref(A, b, cases, sing_tol=0.0):
    """-> (X [n, ncases], rpiv [ncases], cond_S [ncases]); a case with rpiv <= sing_tol (sing_tol > 0) or an exactly zero
    pivot has a NaN column."""
    n = A.shape[0]
    lu = spla.splu(A.tocsc())
    x0 = lu.solve(np.asarray(b, dtype=np.float64))
    touched = [np.asarray(c[0], dtype=np.int64) for c in cases if len(c[0])]
    rows_all = np.unique(np.concatenate(touched)) if touched else np.zeros(0, dtype=np.int64)
    Z = np.empty((n, len(rows_all)))
    for k0 in range(0, len(rows_all), 256):
        E = np.zeros((n, len(rows_all[k0:k0 + 256])))
        E[rows_all[k0:k0 + 256], np.arange(E.shape[1])] = 1.0
        Z[:, k0:k0 + 256] = lu.solve(E)
    X = np.empty((n, len(cases)))
    rpiv = np.empty(len(cases))
    cond = np.ones(len(cases))
    for c, case in enumerate(cases):
        if len(case[0]) == 0:
            X[:, c], rpiv[c] = x0, 1.0
            continue
        R, Cc, D, S, where = capacitance(Z, rows_all, case)
        P, L, U = sla.lu(S)
        piv = np.abs(np.diag(U))
        rpiv[c] = piv.min() / max(1.0, np.abs(S).max())
        if piv.min() == 0.0 or (sing_tol > 0 and rpiv[c] <= sing_tol):
            X[:, c] = np.nan
            cond[c] = np.inf
            continue
        y = sla.solve_triangular(U, sla.solve_triangular(L, P.T @ (D @ x0[Cc]), lower=True, unit_diagonal=True))
        X[:, c] = x0 - Z[:, where] @ y
        cond[c] = np.linalg.cond(S)
    return X, rpiv, cond


def offdiag_pairs(A):
    """All (i, j), i < j, with both a_ij and a_ji stored, sorted: the branches of the network behind A."""
    Ac = A.tocsc()
    P = sp.csc_matrix((np.ones(Ac.nnz), Ac.indices, Ac.indptr), shape=Ac.shape)
    T = sp.triu(P.multiply(P.T), k=1).tocoo()
    order = np.lexsort((T.col, T.row))
    return np.stack([T.row[order], T.col[order]], axis=1).astype(np.int64)


def branch_outage(A, i, j):
    """Remove a_ij and a_ji and take |a_ij|, |a_ji| off the two diagonals (as synth._graph_to_matrix builds them)."""
    aij, aji = A[i, j], A[j, i]
    return (np.array([i, j, i, j]), np.array([j, i, i, j]), np.array([-aij, -aji, -abs(aij), -abs(aji)]))


def branch_outages(A, count, seed):
    """`count` branch outages by seed (all of them, in order, when count is None or there are no more)."""
    pairs = offdiag_pairs(A)
    if count is not None and count < len(pairs):
        pairs = pairs[np.random.default_rng(seed).choice(len(pairs), size=count, replace=False)]
    Ac = A.tocsc()
    return [branch_outage(Ac, int(i), int(j)) for i, j in pairs]


def singular_case(A, i):
    """dA = -A[i, :]: rank 1, A + dA has a zero row."""
    row = A.tocsr()[i].tocoo()
    return (np.full(row.nnz, i), row.col.copy(), -row.data)


def flatten(cases):
    """-> ([(rows, cols)], cx) as Factorization.updates_plan / solve_updates take them."""
    vals = [np.asarray(c[2], dtype=np.float64) for c in cases]
    return [(c[0], c[1]) for c in cases], (np.concatenate(vals) if vals else np.zeros(0))
