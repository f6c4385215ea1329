"""NumPy restatement of the complex plan (include/csparse3_amd.h, "complex matrices"): the real-equivalent pattern, the
doubled order, the rotation, values, pack, unpack and residual.  Everything numeric works on SEPARATE real and imaginary
float64 arrays, with every product and every sum a NumPy call of its own, in the order the header states -- nothing can
fuse, and NumPy's complex multiplication (whose rounding is its own business) is never used.  Arrays carry the batch in
front: values [batch, nnz], right-hand sides [batch, n, k], their real forms [batch, 2n, k]."""
import numpy as np

N, T, H = 0, 1, 2


def bits(a):
    """The bit patterns of a float64 or complex128 array, flat."""
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        a = a.astype(np.complex128, copy=False).view(np.float64)
    return a.astype(np.float64, copy=False).reshape(-1).view(np.uint64)


def split(z, shape=None):
    """complex array -> (re, im), contiguous float64 copies."""
    z = np.asarray(z, dtype=np.complex128)
    if shape is not None:
        z = z.reshape(shape)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def join(re, im):
    out = np.empty(re.shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def cmul(ar, ai, br, bi):
    """(ar + j ai)(br + j bi): four rounded products, then one subtraction and one addition."""
    p1, p2, p3, p4 = ar * br, ai * bi, ar * bi, ai * br
    return p1 - p2, p3 + p4


def entry_columns(n, Ap):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(Ap[:n + 1], dtype=np.int64)))


def real_pattern(n, Ap, Ai):
    """-> (Rp int32[2n + 1], Ri int32[4 nnz])."""
    Ap = np.asarray(Ap, dtype=np.int64)[:n + 1]
    nnz = int(Ap[n])
    Ai = np.asarray(Ai, dtype=np.int64)[:nnz]
    Rp = np.empty(2 * n + 1, dtype=np.int64)
    Rp[0:2 * n:2] = 4 * Ap[:n]
    Rp[1:2 * n:2] = 4 * Ap[:n] + 2 * np.diff(Ap)
    Rp[2 * n] = 4 * nnz
    Ri = np.empty(4 * nnz, dtype=np.int64)
    lo, hi = positions(n, Ap)
    Ri[lo], Ri[lo + 1], Ri[hi], Ri[hi + 1] = 2 * Ai, 2 * Ai + 1, 2 * Ai, 2 * Ai + 1
    return Rp.astype(np.int32), Ri.astype(np.int32)


def positions(n, Ap):
    """For every entry (storage order): its first position in real column 2j and in real column 2j + 1."""
    Ap = np.asarray(Ap, dtype=np.int64)[:n + 1]
    col = entry_columns(n, Ap)
    t = np.arange(int(Ap[n]), dtype=np.int64) - Ap[col]
    lo = 4 * Ap[col] + 2 * t
    return lo, lo + 2 * (Ap[col + 1] - Ap[col])


def doubled_order(q):
    q = np.asarray(q, dtype=np.int64)
    q2 = np.empty(2 * len(q), dtype=np.int32)
    q2[0::2], q2[1::2] = 2 * q, 2 * q + 1
    return q2


def _ranked(group):
    """Entries 0 .. len - 1 with group keys `group` (entries of a group in ascending entry order): -> a list over
    t = 0, 1, ... of (the entries that are the t-th of their group, their groups)."""
    order = np.argsort(group, kind="stable")
    g = group[order]
    start = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]])) if len(g) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(g)) - np.repeat(start, np.diff(np.concatenate([start, [len(g)]])))
    out = []
    for t in range(int(rank.max()) + 1 if len(g) else 0):
        sel = rank == t
        out.append((order[sel], g[sel]))
    return out


def rotation(n, Ap, Ai, Azr, Azi, rotate=True):
    """-> (sr, si) [batch, n]."""
    batch = Azr.shape[0]
    sr, si = np.ones((batch, n)), np.zeros((batch, n))
    if not rotate:
        return sr, si
    nnz = int(Ap[n])
    col = entry_columns(n, Ap)
    dpos = np.flatnonzero(np.asarray(Ai[:nnz], dtype=np.int64) == col)
    dr, di = np.zeros((batch, n)), np.zeros((batch, n))
    have = np.zeros(n, dtype=bool)
    for t, (sel, rows) in enumerate(_ranked(col[dpos])):
        e = dpos[sel]
        if t == 0:
            dr[:, rows], di[:, rows] = Azr[:, e], Azi[:, e]
            have[rows] = True
        else:
            dr[:, rows] = dr[:, rows] + Azr[:, e]
            di[:, rows] = di[:, rows] + Azi[:, e]
    with np.errstate(all="ignore"):
        m = np.maximum(np.abs(dr), np.abs(di))                     # (propagates NaN)
        good = have[None, :] & np.isfinite(m) & (m > 0.0)
        sr = np.where(good, dr / m, 1.0)
        si = np.where(good, (-di) / m, 0.0)
    return sr, si


def values(n, Ap, Ai, Azr, Azi, sr, si):
    """-> Rx [batch, 4 nnz]."""
    nnz = int(Ap[n])
    row = np.asarray(Ai[:nnz], dtype=np.int64)
    with np.errstate(all="ignore"):
        wr, wi = cmul(sr[:, row], si[:, row], Azr[:, :nnz], Azi[:, :nnz])
    lo, hi = positions(n, Ap)
    Rx = np.full((Azr.shape[0], 4 * nnz), np.nan)
    Rx[:, lo], Rx[:, lo + 1], Rx[:, hi], Rx[:, hi + 1] = wr, wi, -wi, wr
    return Rx


def pack(op, Zr, Zi, sr, si):
    """Z [batch, n, k] -> Y [batch, 2n, k]."""
    batch, n, k = Zr.shape
    with np.errstate(all="ignore"):
        if op == N:
            ur, ui = cmul(sr[:, :, None], si[:, :, None], Zr, Zi)
        elif op == H:
            ur, ui = Zr, Zi
        else:
            ur, ui = Zr, -Zi
    Y = np.empty((batch, 2 * n, k))
    Y[:, 0::2, :], Y[:, 1::2, :] = ur, ui
    return Y


def unpack(op, Y, sr, si, Zr=None, Zi=None):
    """Y [batch, 2n, k] -> (Zr, Zi) [batch, n, k]; with Zr, Zi given the result is added to them."""
    yr, yi = Y[:, 0::2, :], Y[:, 1::2, :]
    with np.errstate(all="ignore"):
        if op == H:
            yr, yi = cmul(sr[:, :, None], -si[:, :, None], yr, yi)
        elif op == T:
            yr, yi = cmul(sr[:, :, None], si[:, :, None], yr, -yi)
        if Zr is not None:
            yr, yi = Zr + yr, Zi + yi
    return np.ascontiguousarray(yr), np.ascontiguousarray(yi)


def residual(op, n, Ap, Ai, Azr, Azi, Br, Bi, Xr, Xi):
    """R = B - op(A) X, (Rr, Ri) [batch, n, k]: the accumulator starts at b and subtracts term by term; op N walks a row
    by ascending column (storage order inside a column), ops T and H walk a column in storage order."""
    nnz = int(Ap[n])
    row = np.asarray(Ai[:nnz], dtype=np.int64)
    col = entry_columns(n, Ap)
    out_of, x_of = (row, col) if op == N else (col, row)
    ar, ai = Azr[:, :nnz], (-Azi[:, :nnz] if op == H else Azi[:, :nnz])
    Rr, Ri = Br.copy(), Bi.copy()
    with np.errstate(all="ignore"):
        for e, g in _ranked(out_of):
            tr, ti = cmul(ar[:, e, None], ai[:, e, None], Xr[:, x_of[e], :], Xi[:, x_of[e], :])
            Rr[:, g, :] = Rr[:, g, :] - tr
            Ri[:, g, :] = Ri[:, g, :] - ti
    return Rr, Ri


def dense_real(n, Ap, Ai, Rx):
    """The dense real form [2n, 2n] of one matrix from its real pattern and values (entries stored twice add up)."""
    Rp, Ri = real_pattern(n, Ap, Ai)
    M = np.zeros((2 * n, 2 * n))
    col = np.repeat(np.arange(2 * n), np.diff(Rp))
    np.add.at(M, (Ri, col), Rx)
    return M


def dense_complex(n, Ap, Ai, Az):
    A = np.zeros((n, n), dtype=np.complex128)
    np.add.at(A, (np.asarray(Ai[:Ap[n]]), entry_columns(n, Ap)), np.asarray(Az)[:Ap[n]])
    return A


def apply_op(op, A):
    return A if op == N else (A.T if op == T else A.conj().T)


def solve_through_real_form(op, n, Ap, Ai, Az, b, rotate):
    """op(A) x = b for ONE matrix through the restated plan and numpy.linalg.solve on the dense real form; b [n, k]."""
    Azr, Azi = split(Az, (1, -1))
    sr, si = rotation(n, Ap, Ai, Azr, Azi, rotate)
    M = dense_real(n, Ap, Ai, values(n, Ap, Ai, Azr, Azi, sr, si)[0])
    Br, Bi = split(b, (1, n, -1))
    Y = pack(op, Br, Bi, sr, si)
    X2 = np.linalg.solve(M if op == N else M.T, Y[0])[None]
    return join(*unpack(op, X2, sr, si))[0]
