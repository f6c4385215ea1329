"""References for the selected inversion (cs3_selinv_*): the dense inverse, and a NumPy restatement of the per-front
recurrence driven by the handle's ordering, supernodes, front structures and factors -- the arithmetic selinv.hip does,
front by front, so that a wrong entry can be traced to its front.  The restatement is itself held to the dense inverse
(tests/test_selinv_cpu.py).  Used by tests/test_selinv_cpu.py and tests/test_gpu_selinv.py, and, with the error measure
per block of a front (front_block_errors), by tests/test_selinv_edge_cases_cpu.py and tests/test_gpu_selinv_edges.py.
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


def front_block_errors(hip, F, Zl, Zu, Zref):
    """max |Z - Z_ref| / max |Z_ref| over every block of every front ALONE, so that a wrong block cannot hide behind the
    larger entries of another one.  (Zl, Zu) are F.inverse_on_factors() -- Z at the positions of factors()' L and U, in
    pivot-order labels, Zu None for Cholesky -- and Zref is the dense inverse in the caller's labels.  The blocks of the
    front of supernode s with pivots P and update rows C: 'PP' (the stored entries of Z(P, P): the lower triangle from Zl,
    the upper one from Zu), 'CP' (Z(C, P), from Zl) and 'PC' (Z(P, C), from Zu; absent for Cholesky).
    -> [(supernode, r, w, block, error)] for the blocks that hold an entry; anything not finite in a block makes it inf."""
    sn_ptr, _, _, st = fronts(hip, F)
    n, ns = F.n, len(st)
    q = F.ordering()["q"]
    Zp = Zref[np.ix_(q, q)]
    col2sn = np.repeat(np.arange(ns), np.diff(sn_ptr))
    Lp, Li, _, Up, Ui, _ = F.factors(values=False)
    num = {b: np.zeros(ns) for b in ("PP", "CP", "PC")}
    den = {b: np.zeros(ns) for b in ("PP", "CP", "PC")}
    parts = [(Zl, Lp, Li, "CP", False)] + ([(Zu, Up, Ui, "PC", True)] if Zu is not None else [])
    for got, Gp, Gi, off, upper in parts:
        nz = int(Gp[n])
        rows, cols = np.asarray(Gi[:nz]), np.repeat(np.arange(n), np.diff(Gp))
        want = Zp[rows, cols]
        got = np.asarray(got[:nz], dtype=np.float64)
        diff = np.where(np.isfinite(got), np.abs(got - want), np.inf)
        piv = rows if upper else cols                          # the label that is a pivot of the front: min(row, col)
        assert ((rows <= cols) if upper else (rows >= cols)).all()
        sn = col2sn[piv]
        inside = col2sn[rows] == col2sn[cols]
        for block, mask in (("PP", inside), (off, ~inside)):
            np.maximum.at(num[block], sn[mask], diff[mask])
            np.maximum.at(den[block], sn[mask], np.abs(want[mask]))
    out = []
    for s in range(ns):
        r, w = len(st[s]), int(sn_ptr[s + 1] - sn_ptr[s])
        for block in ("PP", "CP", "PC"):
            if den[block][s] > 0.0 or num[block][s] > 0.0:
                out.append((s, r, w, block, float(num[block][s] / den[block][s]) if den[block][s] > 0.0 else np.inf))
    return out


def worst_block(blocks):
    """The block of front_block_errors() with the largest error, as text."""
    s, r, w, block, err = max(blocks, key=lambda b: b[4])
    return "%.3e in Z_%s of front %d (r = %d, w = %d)" % (err, block, s, r, w)


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
