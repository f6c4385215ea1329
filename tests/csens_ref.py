"""NumPy restatement of the complex sparse right-hand-side path (cs3_cplx_sens_*: csrc/cplxsens.hip and csens_run in
csrc/apps.cpp) and of complex Schur handles (cs3_cplx_plan_create_schur, cs3_cplx_schur_get).

scatter and combine work on SEPARATE real and imaginary float64 arrays, every product and every sum a NumPy call of its
own in the order the header states (cplx_ref.cmul; NumPy's complex multiplication is never used); the real solve between
them is a callback, so the same code runs on numpy.linalg.solve (tests without a GPU) and on the handle's own solve_dev
(the bit-for-bit tests).  The dense references at the end use NumPy complex arithmetic: they are the definition.

An operand is a sens_ref.Op(ncols, indptr, indices, values) with complex values, or None for the identity."""
import numpy as np

import cplx_ref as ref
from sens_ref import LEFT, RIGHT, Op, choose_side, tiles  # noqa: F401  (re-exported for the tests)

N, T, H = ref.N, ref.T, ref.H


def canon_bits(a):
    """The bit patterns of `a` with every NaN replaced by one NaN (IEEE 754 leaves the sign and payload of a produced NaN
    to the implementation); everything else is compared bit for bit, signed zeros included."""
    f = np.array(ref.bits(a).view(np.float64), copy=True)
    f[np.isnan(f)] = np.nan
    return f.view(np.uint64)


def same(got, want):
    g, w = canon_bits(got), canon_bits(want)
    if np.shape(got) == np.shape(want) and np.array_equal(g, w):
        return True
    if np.shape(got) != np.shape(want):
        print("shapes differ: %s against %s" % (np.shape(got), np.shape(want)))
    else:
        bad = np.flatnonzero(g != w)
        print("%d of %d words differ; first: %s" % (len(bad), len(g), [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad[:6]]))
    return False


def glue(side, op):
    """(inner op, conjugate): the table of the header.  Side left solves with the transpose of op(A): inner T for op N,
    inner N for op T, and for op H inner N between two conjugations (A^-H = conj(A^-T))."""
    if side == RIGHT:
        return op, False
    return (T if op == N else N), op == H


def _ranked_columns(indptr, c0, t):
    """For rank r = 0, 1, ...: (entries that are the r-th of their column, their tile columns), columns c0 .. c0 + t."""
    indptr = np.asarray(indptr, dtype=np.int64)
    lens = indptr[c0 + 1:c0 + t + 1] - indptr[c0:c0 + t]
    for r in range(int(lens.max()) if t else 0):
        j = np.flatnonzero(lens > r)
        yield indptr[c0 + j] + r, j


def _pack_entry(inner, conj, sr, si, i, vr, vi):
    """pack_inner of the numbers (vr, vi) at rows i: cs3_cplx_pack_dev's expressions, after the table's conjugation."""
    if conj:
        vi = -vi
    with np.errstate(all="ignore"):
        if inner == N:
            return ref.cmul(sr[i], si[i], vr, vi)
    return (vr, -vi) if inner == T else (vr, vi)


def scatter(n, w, op, c0, t, inner, conj, sr, si):
    """The tile T [2n, w]: columns j < t hold pack_inner of column c0 + j of `op` -- Re u added to row 2i, Im u to row
    2i + 1 of a zeroed tile, duplicates in storage order; an identity operand STORES pack_inner((1, +0)) -- and the
    columns behind t stay zero.  sr, si [n]."""
    Tl = np.zeros((2 * n, w))
    if op is None:
        i = c0 + np.arange(t)
        ur, ui = _pack_entry(inner, conj, sr, si, i, np.ones(t), np.zeros(t))
        Tl[2 * i, np.arange(t)], Tl[2 * i + 1, np.arange(t)] = ur, ui
        return Tl
    vr, vi = ref.split(op.values)
    rows = np.asarray(op.indices, dtype=np.int64)
    with np.errstate(all="ignore"):
        for e, j in _ranked_columns(op.indptr, c0, t):
            i = rows[e]
            ur, ui = _pack_entry(inner, conj, sr, si, i, vr[e], vi[e])
            Tl[2 * i, j] = Tl[2 * i, j] + ur
            Tl[2 * i + 1, j] = Tl[2 * i + 1, j] + ui
    return Tl


def unpacked(Tl, inner, conj, sr, si):
    """(yr, yi) [n, w]: cs3_cplx_unpack_dev's expressions on every pair of rows, then the table's conjugation."""
    yr, yi = ref.unpack(inner, Tl[None], sr[None], si[None])
    return yr[0], (-yi[0] if conj else yi[0])


def combine(Tl, t, op, ng, inner, conj, sr, si):
    """(outr, outi) [ng, t]: out[g, j] = sum over the entries (i, v) of column g of `op` of v * y[i, j], the first product
    starting the sum, later ones added component by component in storage order; an empty column gives (+0, +0); an
    identity operand hands y over."""
    yr, yi = unpacked(Tl, inner, conj, sr, si)
    yr, yi = yr[:, :t], yi[:, :t]
    if op is None:
        return yr[:ng].copy(), yi[:ng].copy()
    outr, outi = np.zeros((ng, t)), np.zeros((ng, t))
    vr, vi = ref.split(op.values)
    rows = np.asarray(op.indices, dtype=np.int64)
    with np.errstate(all="ignore"):
        for r, (e, g) in enumerate(_ranked_columns(op.indptr, 0, ng)):
            pr, pi = ref.cmul(vr[e, None], vi[e, None], yr[rows[e]], yi[rows[e]])
            if r == 0:
                outr[g], outi[g] = pr, pi
            else:
                outr[g], outi[g] = outr[g] + pr, outi[g] + pi
    return outr, outi


def y_restated(n, B, Ct, side, op, sr, si, tile_list, solve, parts=7, tile_in=None):
    """Y [p, k] complex as cs3_cplx_sens_solve computes it.  side: RIGHT or LEFT (already chosen); tile_list: sens_ref.tiles
    of the solved-for columns; solve(T [2n, w], trans) -> the real solve of the handle, plain or transposed.
    parts: the mask of cs3_debug_cplx_sens_parts; without the scatter the tiles come from tile_in(c0, w)."""
    k = n if B is None else B.ncols
    p = n if Ct is None else Ct.ncols
    inner, conj = glue(side, op)
    solved, other = (B, Ct) if side == RIGHT else (Ct, B)
    ng = p if side == RIGHT else k
    Y = np.zeros((p, k), dtype=np.complex128)
    last = None
    for c0, t, w in tile_list:
        Tl = scatter(n, w, solved, c0, t, inner, conj, sr, si) if parts & 1 else tile_in(c0, w)
        if parts & 2:
            Tl = solve(Tl, inner != N)
        last = Tl
        if parts & 4:
            outr, outi = combine(Tl, t, other, ng, inner, conj, sr, si)
            if side == RIGHT:
                Y[:, c0:c0 + t] = ref.join(outr, outi)
            else:
                Y[c0:c0 + t, :] = ref.join(outr, outi).T
    return Y, last


def dense_solve_callback(n, Ap, Ai, Az, rotate=True, border=()):
    """(sr, si [n], solve) for ONE matrix: the restated rotation and values, numpy.linalg.solve on the dense real form."""
    Azr, Azi = ref.split(Az, (1, -1))
    sr, si = rotation_with_border(n, Ap, Ai, Azr, Azi, rotate, border)
    M = ref.dense_real(n, Ap, Ai, ref.values(n, Ap, Ai, Azr, Azi, sr, si)[0])
    return sr[0], si[0], (lambda Tl, trans: np.linalg.solve(M.T if trans else M, Tl))


# ---------------------------------------------------------------- the definition, in NumPy complex arithmetic --

def dense_op(op, n):
    """The n x ncols complex matrix of an operand, duplicates added."""
    D = np.zeros((n, op.ncols), dtype=np.complex128)
    cols = np.repeat(np.arange(op.ncols), np.diff(np.asarray(op.indptr)))
    np.add.at(D, (np.asarray(op.indices), cols), np.asarray(op.values, dtype=np.complex128))
    return D


def y_dense(A, B, Ct, op):
    """C op(A)^-1 B for the dense complex A; B / Ct None: the identity."""
    n = A.shape[0]
    X = np.linalg.solve(ref.apply_op(op, A), np.eye(n, dtype=np.complex128) if B is None else dense_op(B, n))
    return X if Ct is None else dense_op(Ct, n).T @ X


def split_border(n, border):
    border = np.asarray(border, dtype=np.int64)
    interior = np.setdiff1d(np.arange(n), border)
    return interior, border


def schur_dense(A, border):
    """(S, bound): S = A22 - A21 A11^-1 A12 on `border` (in its order), and |A22| + |A21| |A11^-1| |A12|, the size that the
    rounding errors of any elimination are proportional to."""
    interior, border = split_border(A.shape[0], border)
    A11, A12 = A[np.ix_(interior, interior)], A[np.ix_(interior, border)]
    A21, A22 = A[np.ix_(border, interior)], A[np.ix_(border, border)]
    inv = np.linalg.inv(A11)
    return A22 - A21 @ inv @ A12, np.abs(A22) + np.abs(A21) @ np.abs(inv) @ np.abs(A12), float(np.linalg.cond(A11))


# ---------------------------------------------------------------- plans with a border --

def rotation_with_border(n, Ap, Ai, Azr, Azi, rotate, border):
    """cplx_ref.rotation with the border rows left at (1, +0): their diagonal lists are empty in the plan's tables."""
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate)
    border = np.asarray(border, dtype=np.int64)
    sr[:, border], si[:, border] = 1.0, 0.0
    return sr, si


def interior_pattern(n, Ap, Ai, border):
    """(interior, A11p, A11i): A with the border rows and columns removed, entries in A's order, renumbered."""
    interior, border = split_border(n, border)
    label = np.full(n, -1, dtype=np.int64)
    label[interior] = np.arange(len(interior))
    A11p, A11i = [0], []
    for j in interior:
        rows = np.asarray(Ai[Ap[j]:Ap[j + 1]], dtype=np.int64)
        A11i += [int(v) for v in label[rows] if v >= 0]
        A11p.append(len(A11i))
    return interior, np.array(A11p, dtype=np.int32), np.array(A11i, dtype=np.int32)


def schur_order(border, q_interior):
    """-> (q2_interior, schur2): both doubled as cs3_cplx_plan_order doubles."""
    return ref.doubled_order(q_interior), ref.doubled_order(border)
