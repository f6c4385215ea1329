"""References for the selected inversion (cs3_selinv_*): the dense inverse, and a NumPy restatement of the per-front
recurrence driven by the handle's ordering, supernodes, front structures and factors -- the arithmetic selinv.hip does,
front by front, so that a wrong entry can be traced to its front.  The restatement is itself held to the dense inverse
(tests/test_selinv_cpu.py).  Used by tests/test_selinv_cpu.py and tests/test_gpu_selinv.py.
"""
import numpy as np

BOUND = 1e-10                 # max |Z - Z_ref| <= BOUND * max |Z_ref|: the project's factor-parity bar
COND_MAX = 1e4                # every test matrix is at most this ill-conditioned (1-norm)


def dense(n, Ap, Ai, Ax):
    """A CSC matrix as a dense float64 array (duplicates add)."""
    A = np.zeros((n, n))
    nz = int(Ap[n])
    np.add.at(A, (np.asarray(Ai[:nz]), np.repeat(np.arange(n), np.diff(Ap))), np.asarray(Ax[:nz], dtype=np.float64))
    return A


def dense_inverse(n, Ap, Ai, Ax):
    """(A^-1, cond_1(A)) by np.linalg.inv."""
    A = dense(n, Ap, Ai, Ax)
    Z = np.linalg.inv(A)
    return Z, float(np.abs(A).sum(axis=0).max() * np.abs(Z).sum(axis=0).max())


def entries_of(Z, n, Ap, Ai, trans=False):
    """Z at the stored positions of a CSC pattern: Z[Ai[p], j], or Z[j, Ai[p]] with trans."""
    nz = int(Ap[n])
    rows, cols = np.asarray(Ai[:nz]), np.repeat(np.arange(n), np.diff(Ap))
    return Z[cols, rows] if trans else Z[rows, cols]


def max_error(got, ref):
    """max |got - ref| / max |ref| (inf when anything is not finite)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def fronts(hip, F):
    """The fronts of a handle from what the ABI hands out: (sn_ptr, sn_parent, sn_level, structures); structures[s] is the
    sorted row structure of supernode s in pivot-order labels, its own columns first: the columns of s and every row of L
    in one of them (cs3_get_factors' pattern; amalgamation only merges columns, so the union is the front)."""
    sn_ptr, sn_parent, sn_level = F.supernodes()
    Lp, Li = F.factors(values=False)[:2]
    structures = []
    for s in range(len(sn_parent)):
        c0, c1 = int(sn_ptr[s]), int(sn_ptr[s + 1])
        rows = np.union1d(np.arange(c0, c1), Li[Lp[c0]:Lp[c1]])
        assert (rows[:c1 - c0] == np.arange(c0, c1)).all()
        structures.append(rows.astype(np.int64))
    return sn_ptr, sn_parent, sn_level, structures


def top_down(sn_parent, sn_level):
    """Supernodes with every parent before its children: level descending."""
    return sorted(range(len(sn_parent)), key=lambda s: (-int(sn_level[s]), s))


def restated_positions(hip, F, Ap, Ai, front):
    """The extraction maps restated: with the fronts' r x r blocks laid out back to back in the order `front`
    (cs3_debug_selinv_plan), the offset of Z(pinv i, pinv j) for every entry of A and of Z(pinv i, pinv i) for every i:
    the block of the front of min(pinv i, pinv j), at the positions of the two labels in its structure."""
    sn_ptr, _, _, st = fronts(hip, F)
    n = F.n
    z_off, total = {}, 0
    for s in front:
        z_off[int(s)] = total
        total += len(st[int(s)]) ** 2
    col2sn = np.repeat(np.arange(len(st)), np.diff(sn_ptr))
    pinv = F.ordering()["pinv"]

    def position(k, l):
        s = int(col2sn[min(k, l)])
        at = {int(v): i for i, v in enumerate(st[s])}
        return z_off[s] + at[k] + at[l] * len(st[s])

    cols = np.repeat(np.arange(n), np.diff(Ap))
    entry = np.array([position(int(pinv[Ai[p]]), int(pinv[cols[p]])) for p in range(int(Ap[n]))], dtype=np.int64)
    diag = np.array([position(int(pinv[i]), int(pinv[i])) for i in range(n)], dtype=np.int64)
    return entry, diag, total


def dense_factors(F, b=0):
    """(L, U) of matrix b as dense arrays in pivot-order labels, from factors() (Cholesky: U = L')."""
    Lp, Li, Lx, Up, Ui, Ux = F.factors(b)
    L = dense(F.n, Lp, Li, Lx)
    return L, (dense(F.n, Up, Ui, Ux) if Up is not None else L.T.copy())


def host_factors(F, A, cholesky=False):
    """The same factors on the host, for tests without a GPU: B = A[q][:, q] = L U by elimination with the diagonal
    pivots the library takes (unit L), or B = L L' by np.linalg.cholesky."""
    q = F.ordering()["q"]
    B = np.array(A[np.ix_(q, q)], dtype=np.float64)
    if cholesky:
        L = np.linalg.cholesky(B)
        return L, L.T.copy()
    n = len(B)
    for k in range(n):
        B[k + 1:, k] /= B[k, k]
        B[k + 1:, k + 1:] -= np.outer(B[k + 1:, k], B[k, k + 1:])
    return np.tril(B, -1) + np.eye(n), np.triu(B)


def restated_inverse(hip, F, L, U):
    """Z = (Q' A Q)^-1 on the pattern of L + U by the per-front recurrence, from dense factors in pivot-order labels: a
    dense [n, n] array, NaN outside the pattern.  Per front, parents first:
        X = L21 L11^-1, Y = U11^-1 U12, Z_CC from the parent, Z_CP = -Z_CC X, Z_PC = -Y Z_CC, Z_PP = U11^-1 L11^-1 - Y Z_CP."""
    n = F.n
    sn_ptr, sn_parent, sn_level, st = fronts(hip, F)
    Z = np.full((n, n), np.nan)
    for s in top_down(sn_parent, sn_level):
        w = int(sn_ptr[s + 1] - sn_ptr[s])
        P, C = st[s][:w], st[s][w:]
        X = L[np.ix_(C, P)] @ np.linalg.inv(L[np.ix_(P, P)])
        Y = np.linalg.inv(U[np.ix_(P, P)]) @ U[np.ix_(P, C)]
        Zcc = Z[np.ix_(C, C)]
        assert np.isfinite(Zcc).all(), "front %d: its update block is not inside its ancestors' fronts" % s
        Zcp = -Zcc @ X
        Z[np.ix_(C, P)] = Zcp
        Z[np.ix_(P, C)] = -Y @ Zcc
        Z[np.ix_(P, P)] = np.linalg.inv(U[np.ix_(P, P)]) @ np.linalg.inv(L[np.ix_(P, P)]) - Y @ Zcp
    return Z
