"""References for the complex selected inversion (cs3_cplx_selinv_*).

restate(): the definitions of the header on separate real and imaginary arrays, every product rounded on its own, from
what the REAL handle hands out -- Factorization.inverse_entries(trans=0 / 1) on the real pattern of 4 nnz entries -- and
the plan's rotation().  The complex getters can then be required bit for bit.  The restatement is itself held to
numpy.linalg.inv of the complex matrix (tests/test_cselinv_cpu.py), fed with the real form of a dense inverse.

dense_inverse(): numpy.linalg.inv of the complex matrix with its 1-norm condition number.
"""
import numpy as np

import cplx_ref as ref

from selinv_ref import BOUND, COND_MAX                     # noqa: F401  (the project's bar: 1e-10 max |Z_ref| under cond_1 <= 1e4)


def same_bits(got, want):
    """Bit for bit, signed zeros included."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(ref.bits(got), ref.bits(want))


def first_diagonal_entry(n, Ap, Ai):
    """[n]: the first stored (i, i) of every column, -1 where there is none."""
    nnz = int(Ap[n])
    col = ref.entry_columns(n, Ap)
    e = np.flatnonzero(np.asarray(Ai[:nnz], dtype=np.int64) == col)
    first = np.full(n, -1, dtype=np.int64)
    first[col[e][::-1]] = e[::-1]
    return first


def restate(n, Ap, Ai, ZRe, ZRt, s, ZRd=None):
    """ZRe, ZRt [batch, 4 nnz]: ZR at the stored positions of the real pattern and at their transposes; s [batch, n]
    complex.  ZRd [batch, n, 2] = (ZR(2i, 2i), ZR(2i + 1, 2i)), only needed when a row has no stored diagonal (otherwise
    the pair is read at the first stored (i, i), the same two numbers).
    -> dict of complex128 [batch, .]: entries, entries_t, diagonal, thevenin."""
    nnz = int(Ap[n])
    s = np.asarray(s, dtype=np.complex128)
    batch = s.size // n if n else 1
    ZRe, ZRt = np.asarray(ZRe, dtype=np.float64).reshape(batch, 4 * nnz), np.asarray(ZRt, dtype=np.float64).reshape(batch, 4 * nnz)
    sr, si = ref.split(s.reshape(batch, n))
    row, col = np.asarray(Ai[:nnz], dtype=np.int64), ref.entry_columns(n, Ap)
    lo, hi = ref.positions(n, Ap)                                               # Rp[2j] + 2t, Rp[2j + 1] + 2t
    # Minv(i, j) = (ZR(2i, 2j), ZR(2i + 1, 2j)); Z(i, j) = Minv(i, j) * s_j
    zr, zi = ref.cmul(ZRe[:, lo], ZRe[:, lo + 1], sr[:, col], si[:, col])
    # Minv(j, i) = (ZR(2j, 2i), ZR(2j + 1, 2i)): the transposes of the real entries (2i, 2j) and (2i, 2j + 1); times s_i
    tr, ti = ref.cmul(ZRt[:, lo], ZRt[:, hi], sr[:, row], si[:, row])
    if ZRd is None:
        first = first_diagonal_entry(n, Ap, Ai)
        assert (first >= 0).all(), "a row without a stored diagonal: pass ZRd"
        mdr, mdi = ZRe[:, lo[first]], ZRe[:, lo[first] + 1]
    else:
        ZRd = np.asarray(ZRd, dtype=np.float64).reshape(batch, n, 2)
        mdr, mdi = ZRd[:, :, 0], ZRd[:, :, 1]
    dr, di = ref.cmul(mdr, mdi, sr, si)
    # T = ((Z_ii + Z_jj) - Z_ij) - Z_ji, component by component
    thr = ((dr[:, row] + dr[:, col]) - zr) - tr
    thi = ((di[:, row] + di[:, col]) - zi) - ti
    return {"entries": ref.join(zr, zi), "entries_t": ref.join(tr, ti), "diagonal": ref.join(dr, di), "thevenin": ref.join(thr, thi)}


def restate_from_handle(F, Ap, Ai):
    """restate() on a factorised ComplexFactorization of the pattern (Ap, Ai), every diagonal stored."""
    return restate(F.n, Ap, Ai, F.real.inverse_entries(trans=False), F.real.inverse_entries(trans=True), F.plan.rotation())


def dense_inverse(n, Ap, Ai, Az):
    """(A^-1 complex [n, n], cond_1(A))."""
    A = ref.dense_complex(n, Ap, Ai, Az)
    Z = np.linalg.inv(A)
    cond = float(np.abs(A).sum(axis=0).max() * np.abs(Z).sum(axis=0).max()) if n else 1.0
    return Z, cond


def dense_results(Z, n, Ap, Ai):
    """The four results from a dense complex Z."""
    nnz = int(Ap[n])
    row, col = np.asarray(Ai[:nnz], dtype=np.int64), ref.entry_columns(n, Ap)
    d = Z.diagonal()
    return {"entries": Z[row, col], "entries_t": Z[col, row], "diagonal": d.copy(), "thevenin": ((d[row] + d[col]) - Z[row, col]) - Z[col, row]}


def real_form(Z):
    """[2n, 2n]: every entry w of the complex Z as [[Re w, -Im w], [Im w, Re w]], rows and columns interleaved."""
    n = Z.shape[0]
    R = np.empty((2 * n, 2 * n))
    R[0::2, 0::2], R[1::2, 1::2] = Z.real, Z.real
    R[1::2, 0::2], R[0::2, 1::2] = Z.imag, -Z.imag
    return R


def real_handle_outputs(ZR, n, Ap, Ai):
    """(ZRe, ZRt [4 nnz], ZRd [n, 2]): what the real handle's getters would return for a dense real ZR [2n, 2n]."""
    Rp, Ri = ref.real_pattern(n, Ap, Ai)
    rcol = np.repeat(np.arange(2 * n), np.diff(Rp))
    i2 = 2 * np.arange(n)
    return ZR[Ri, rcol], ZR[rcol, Ri], np.stack([ZR[i2, i2], ZR[i2 + 1, i2]], axis=1)


def max_error(got, want, scale):
    """max |got - want| / scale (inf when anything is not finite; 0 for empty arrays)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - want).max() / scale)
