"""NumPy restatement of the complex low-rank-modified solves (cs3_cplx_updates_*: csrc/cplxupd.hip and cupd_run in
csrc/apps.cpp), on SEPARATE real and imaginary float64 arrays with every product, quotient and sum a NumPy call of its own
in the order the header states (cplx_ref.cmul, cdiv below; NumPy's complex arithmetic is never used in the restatement).
The real solve between the steps is a callback, as in csens_ref: numpy.linalg.solve on the dense real form for the tests
without a GPU, the handle's own solve_dev for the GPU tests.  The dense reference at the end is NumPy complex128: it is
the definition.

A case is (rows, cols, vals) with complex vals: the triplets of dA_c, duplicates adding in triplet order."""
import collections

import numpy as np

import cplx_ref as ref

MAX_RANK = 16


def cdiv(ar, ai, br, bi):
    """(ar + j ai) / (br + j bi) as the header writes it: den = br br + bi bi, ((ar br + ai bi) / den, (ai br - ar bi) / den)."""
    den = br * br + bi * bi
    return (ar * br + ai * bi) / den, (ai * br - ar * bi) / den


def cabs1(r, i):
    return np.abs(r) + np.abs(i)


# ------------------------------------------------------------------- the plan --

def tile_columns(cases, tiles):
    """For every tile (first case, cases, touched rows, width) of a plan: the rows of its columns, in order of first use
    (a case's rows ascending), padded with -1 to the width."""
    out = []
    for c0, nc, t, w in tiles:
        seen, cur = set(), []
        for case in cases[c0:c0 + nc]:
            for r in np.unique(np.asarray(case[0], dtype=np.int64)):
                if int(r) not in seen:
                    seen.add(int(r))
                    cur.append(int(r))
        assert len(cur) == t
        out.append(np.array(cur + [-1] * (w - t), dtype=np.int64))
    return out


# ------------------------------------------------------------------ the steps --

def units(n, unit_row, sr, si):
    """The tile Z [2n, w]: column j holds pack_N((1, +0)) = s_row (1, +0) in the pair of row unit_row[j]; negative: zero."""
    unit_row = np.asarray(unit_row, dtype=np.int64)
    Z = np.zeros((2 * n, len(unit_row)))
    j = np.flatnonzero(unit_row >= 0)
    i = unit_row[j]
    with np.errstate(all="ignore"):
        ur, ui = ref.cmul(sr[i], si[i], np.ones(len(i)), np.zeros(len(i)))
    Z[2 * i, j], Z[2 * i + 1, j] = ur, ui
    return Z


Cap = collections.namedtuple("Cap", "yr yi rpiv flag picks pivots margins Sr Si")


def capacitance(Zr, Zi, x0r, x0i, case, zcol, sing_tol=0.0):
    """One case on the solved tile (Zr, Zi [n, t]: the real and imaginary rows of the pairs) and x0.  zcol: the tile
    columns of its rows R_c, ascending.  -> Cap: y [r], rpiv, flag, the rows picked, cabs1 of the pivots, per step the
    relative margin between the two best candidates, and S as formed."""
    rows, cols, vals = np.asarray(case[0], dtype=np.int64), np.asarray(case[1], dtype=np.int64), np.asarray(case[2], dtype=np.complex128)
    R, ri = np.unique(rows, return_inverse=True)
    Cc, ci = np.unique(cols, return_inverse=True)
    r, s = len(R), len(Cc)
    if r == 0:
        return Cap(np.zeros(0), np.zeros(0), 1.0, 0, [], [], [], None, None)
    with np.errstate(all="ignore"):
        Dr, Di = np.zeros((r, s)), np.zeros((r, s))
        np.add.at(Dr, (ri, ci), np.ascontiguousarray(vals.real))       # (unbuffered: in triplet order)
        np.add.at(Di, (ri, ci), np.ascontiguousarray(vals.imag))
        Gr, Gi = Zr[np.ix_(Cc, zcol)], Zi[np.ix_(Cc, zcol)]             # s x r
        Sr, Si = np.eye(r), np.zeros((r, r))
        br, bi = np.zeros(r), np.zeros(r)
        for a in range(s):
            pr, pi = ref.cmul(Dr[:, a, None], Di[:, a, None], Gr[None, a, :], Gi[None, a, :])
            Sr, Si = Sr + pr, Si + pi
            pr, pi = ref.cmul(Dr[:, a], Di[:, a], x0r[Cc[a]], x0i[Cc[a]])
            br, bi = br + pr, bi + pi
        S0r, S0i = Sr.copy(), Si.copy()
        smax = float(np.fmax.reduce(cabs1(Sr, Si).ravel(), initial=0.0))
        Ur, Ui = np.concatenate([Sr, br[:, None]], axis=1), np.concatenate([Si, bi[:, None]], axis=1)
        pmin, zero, picks, pivots, margins = np.inf, False, [], [], []
        for k in range(r):
            cand = cabs1(Ur[k:, k], Ui[k:, k])
            nan = np.flatnonzero(np.isnan(cand))
            p = k + (int(nan[0]) if len(nan) else int(np.argmax(cand)))   # a NaN above every number; ties to the lowest row
            pv = float(cand[p - k])
            if len(cand) > 1 and not len(nan):
                top = np.sort(cand)[::-1]
                margins.append(float((top[0] - top[1]) / top[0]) if top[0] > 0 else 0.0)
            picks.append(p)
            pivots.append(pv)
            if not pv > 0.0:
                pmin, zero = pv, True
                break
            pmin = pv if pv < pmin else pmin
            if p != k:
                Ur[[k, p]], Ui[[k, p]] = Ur[[p, k]], Ui[[p, k]]
            lr, li = cdiv(Ur[k + 1:, k], Ui[k + 1:, k], Ur[k, k], Ui[k, k])
            pr, pi = ref.cmul(lr[:, None], li[:, None], Ur[None, k, k + 1:], Ui[None, k, k + 1:])
            Ur[k + 1:, k + 1:] = Ur[k + 1:, k + 1:] - pr
            Ui[k + 1:, k + 1:] = Ui[k + 1:, k + 1:] - pi
        yr, yi = np.zeros(r), np.zeros(r)
        if not zero:
            for k in range(r - 1, -1, -1):
                yr[k], yi[k] = cdiv(Ur[k, r], Ui[k, r], Ur[k, k], Ui[k, k])
                pr, pi = ref.cmul(Ur[:k, k], Ui[:k, k], yr[k], yi[k])
                Ur[:k, r], Ui[:k, r] = Ur[:k, r] - pr, Ui[:k, r] - pi
        rp = pmin / max(1.0, smax) if not np.isnan(pmin) else np.nan
    flag = int(zero or (sing_tol > 0.0 and rp <= sing_tol))
    return Cap(yr, yi, rp, flag, picks, pivots, margins, S0r, S0i)


def apply(Zr, Zi, x0r, x0i, zcol, cap):
    """x_c [n] as (re, im): x0 minus the products Z[:, zcol_j] y_j over ascending j; (NaN, NaN) for a flagged case."""
    if cap.flag:
        return np.full(len(x0r), np.nan), np.full(len(x0r), np.nan)
    xr, xi = x0r.copy(), x0i.copy()
    with np.errstate(all="ignore"):
        for j in range(len(cap.yr)):
            pr, pi = ref.cmul(Zr[:, zcol[j]], Zi[:, zcol[j]], cap.yr[j], cap.yi[j])
            xr, xi = xr - pr, xi - pi
    return xr, xi


def x0_restated(n, b, sr, si, solve):
    """(x0r, x0i): pack_N(b) = s b, the handle's k = 1 solve, the raw join."""
    brr, bii = ref.split(b)
    with np.errstate(all="ignore"):
        ur, ui = ref.cmul(sr, si, brr, bii)
    y = np.empty((2 * n, 1))
    y[0::2, 0], y[1::2, 0] = ur, ui
    y = solve(y, False)
    return np.ascontiguousarray(y[0::2, 0]), np.ascontiguousarray(y[1::2, 0])


def solve_restated(n, cases, tiles, b, sr, si, solve, sing_tol=0.0):
    """-> (X [n, ncases] complex, rpiv, [Cap], the last tile of unit right-hand sides) as cs3_cplx_updates_solve computes
    them.  tiles: the rows of ComplexUpdatesPlan.tiles(); solve(T [2n, w], trans) -> the handle's real solve."""
    x0r, x0i = x0_restated(n, b, sr, si, solve)
    X = np.empty((n, len(cases)), dtype=np.complex128)
    rpiv = np.empty(len(cases))
    caps, last = [None] * len(cases), None
    for (c0, nc, t, w), unit_row in zip(tiles, tile_columns(cases, tiles)):
        Zr = Zi = np.zeros((n, max(w, 1)))
        if t > 0:
            last = units(n, unit_row, sr, si)
            Z = solve(last, False)
            Zr, Zi = np.ascontiguousarray(Z[0::2]), np.ascontiguousarray(Z[1::2])
        pos = {int(row): j for j, row in enumerate(unit_row) if row >= 0}
        for c in range(c0, c0 + nc):
            zcol = np.array([pos[int(r)] for r in np.unique(np.asarray(cases[c][0], dtype=np.int64))], dtype=np.int64)
            cap = capacitance(Zr, Zi, x0r, x0i, cases[c], zcol, sing_tol)
            xr, xi = apply(Zr, Zi, x0r, x0i, zcol, cap)
            X[:, c], rpiv[c], caps[c] = ref.join(xr, xi), cap.rpiv, cap
    return X, rpiv, caps, last


def exact_inverse_callback(A):
    """(sr, si, solve) with s = 1 and the solve of the real form done through the dense complex inverse of A: what the
    restatement gives when Z is exact to rounding."""
    n = A.shape[0]
    inv = np.linalg.inv(A)

    def solve(T, trans):
        assert not trans
        Y = inv @ ref.join(np.ascontiguousarray(T[0::2]), np.ascontiguousarray(T[1::2]))
        out = np.empty_like(T)
        out[0::2], out[1::2] = Y.real, Y.imag
        return out
    return np.ones(n), np.zeros(n), solve


# ---------------------------------------------------------------- the definition, in NumPy complex arithmetic --

def delta_dense(n, case):
    D = np.zeros((n, n), dtype=np.complex128)
    np.add.at(D, (np.asarray(case[0], dtype=np.int64), np.asarray(case[1], dtype=np.int64)), np.asarray(case[2], dtype=np.complex128))
    return D


def x_dense(A, case, b):
    """(x, cond_1(A + dA_c)) by numpy.linalg.solve on the dense modified matrix."""
    M = A + delta_dense(A.shape[0], case)
    return np.linalg.solve(M, b), float(np.real(np.linalg.cond(M, 1)))


def x_woodbury(inv, x0, cases):
    """X [n, ncases] by the formula in NumPy complex arithmetic with the dense inverse (LAPACK for S_c): the reference for
    lists too long for a dense solve per case.  A singular S_c gives a NaN column."""
    X = np.empty((inv.shape[0], len(cases)), dtype=np.complex128)
    for c, case in enumerate(cases):
        if len(case[0]) == 0:
            X[:, c] = x0
            continue
        R, ri = np.unique(np.asarray(case[0], dtype=np.int64), return_inverse=True)
        Cc, ci = np.unique(np.asarray(case[1], dtype=np.int64), return_inverse=True)
        D = np.zeros((len(R), len(Cc)), dtype=np.complex128)
        np.add.at(D, (ri, ci), np.asarray(case[2], dtype=np.complex128))
        S = np.eye(len(R)) + D @ inv[np.ix_(Cc, R)]
        with np.errstate(all="ignore"):
            X[:, c] = x0 - inv[:, R] @ np.linalg.solve(S, D @ x0[Cc]) if np.isfinite(S).all() and np.linalg.cond(S) < 1e13 else np.nan
    return X


def accuracy_bound(cond1, x):
    """1e3 cond_1(A + dA_c) 2^-53 max |x_c|: the form tests/test_gpu_csens.py uses."""
    return 1e3 * cond1 * 2.0 ** -53 * float(np.abs(x).max())


def flatten(cases):
    """-> ([(rows, cols)], cz) as ComplexFactorization.updates_plan / solve_updates take them."""
    vals = [np.asarray(c[2], dtype=np.complex128) for c in cases]
    return [(c[0], c[1]) for c in cases], (np.concatenate(vals) if vals else np.zeros(0, dtype=np.complex128))
