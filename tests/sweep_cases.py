"""Matrices whose wide big fronts sit BELOW the root, a classifier for the solve kind of every front, and a plain
high-precision substitution, for tests/test_sweep_cases_cpu.py and tests/test_gpu_big_fronts_below_root.py.

The matrix: dense diagonal blocks of orders `ds`, each densely coupled to one dense separator of order `s` and to no
other block.  With four blocks the analysis (AMD, relaxed amalgamation) keeps two of them as fronts of their own --
w = d pivots, r = d + s rows, parent = the root -- and folds the other two into the root; with fewer blocks everything
merges into one front.  So one level holds two wide big fronts that have a contribution block and a parent, which no
other matrix of the suite has (there the only front with w > 64 and r > 136 is the root).  `fringe` hangs a chain of
small nodes off every block: fronts of order <= 32 whose parent is a big front that itself has a parent.

Which kernel sweeps a front is decided by the analysis from r, w and the batch (symbolic.cpp: solve_kind);
`solve_kinds()` restates that rule, so that a change of dispatch or of the amalgamation's prices makes the tests'
assertions fail instead of leaving the wide-big-front kernels silently untested.
"""
import collections

import numpy as np

import pivot_cases as pc

# name -> (ds, s); FRONTS: the (r, w) of the fronts with w > 64, in supernode order (the root last)
CASES = {"w72": ((72,) * 4, 70), "w100": ((100,) * 4, 70), "w140": ((140,) * 4, 30), "w200": ((200,) * 4, 70)}
ORDER = {"w72": 358, "w100": 470, "w140": 590, "w200": 870}
FRONTS = {"w72": ((142, 72), (142, 72), (214, 214)), "w100": ((170, 100), (170, 100), (270, 270)),
          "w140": ((170, 140), (170, 140), (310, 310)), "w200": ((270, 200), (270, 200), (470, 470))}
BIG_BATCH_MAX = 15            # symbolic.cpp: a batch of 16 or more sweeps its wide big fronts with the block kernel
SMALL_RMAX, WAVE_RMAX, WAVE_WMAX, BIG_RMIN = 32, 128, 64, 137      # symbolic.cpp: solve_kind (small_rmax; r <= 128, w <= 64; r > 136)


# ------------------------------------------------------------------ construction --

Pattern = collections.namedtuple("Pattern", "n Ap Ai ei ej order")
_PATTERNS = {}


def _pattern(ds, s, fringe):
    key = (tuple(ds), s, fringe)
    if key in _PATTERNS:
        return _PATTERNS[key]
    starts = np.concatenate([[0], np.cumsum(ds)]).astype(np.int64)
    sep0 = int(starts[-1])
    n = sep0 + s + fringe * len(ds)
    sep = np.arange(sep0, sep0 + s)
    ei, ej = [], []
    for k, d in enumerate(ds):
        blk = np.arange(starts[k], starts[k] + d)
        i, j = np.triu_indices(d, 1)                                       # the block itself
        ei.append(blk[i]); ej.append(blk[j])
        i, j = np.meshgrid(blk, sep, indexing="ij")                        # block x separator
        ei.append(i.ravel()); ej.append(j.ravel())
        c0 = sep0 + s + k * fringe                                         # the chain: node t - 1, and two nodes of the block
        for t in range(fringe):
            if t > 0:
                ei.append(np.array([c0 + t - 1])); ej.append(np.array([c0 + t]))
            ei.append(blk[[(2 * t) % d, (2 * t + 1) % d]]); ej.append(np.array([c0 + t, c0 + t]))
    i, j = np.triu_indices(s, 1)
    ei.append(sep[i]); ej.append(sep[j])
    ei, ej = np.concatenate(ei).astype(np.int64), np.concatenate(ej).astype(np.int64)
    assert (ei < ej).all() and len(np.unique(ei * n + ej)) == len(ei)
    rows = np.concatenate([ej, ei, np.arange(n)])                          # lower triangle, upper triangle, diagonal
    cols = np.concatenate([ei, ej, np.arange(n)])
    order = np.lexsort((rows, cols))                                       # by column, rows sorted inside a column
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    _PATTERNS[key] = Pattern(n, Ap.astype(np.int32), rows[order].astype(np.int32), ei, ej, order)
    return _PATTERNS[key]


def blocks_on_separator(ds, s, seed, fringe=0, symmetric=False):
    """-> (m, n, Ap, Ai, Ax).  Off-diagonal entries -U(0.1, 1), drawn independently for the two triangles (symmetric: the
    same value, for Cholesky); diagonal = the column's absolute sum + 1, so every diagonal pivot is its column's largest
    entry.  The pattern does not depend on the seed: matrices of different seeds form a batch."""
    P = _pattern(ds, s, fringe)
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.1, 1.0, size=len(P.ei))                             # entry (ej, ei), column ei
    up = lo if symmetric else rng.uniform(0.1, 1.0, size=len(P.ei))        # entry (ei, ej), column ej
    diag = 1.0 + np.bincount(P.ei, weights=lo, minlength=P.n) + np.bincount(P.ej, weights=up, minlength=P.n)
    Ax = np.concatenate([-lo, -up, diag])[P.order]
    return P.n, P.n, P.Ap, P.Ai, Ax


_VALUES = {}


def case_matrix(name, symmetric=False, fringe=0):
    """The pattern of case `name` with the values of matrix 0 of its batches."""
    ds, s = CASES[name]
    return blocks_on_separator(ds, s, _seed(name, 0), fringe, symmetric)


def _seed(name, i):
    return 1000 * int(name[1:]) + i


def case_values(name, batch, symmetric=False, fringe=0):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own (built once; read-only)."""
    key = (name, batch, symmetric, fringe)
    if key not in _VALUES:
        ds, s = CASES[name]
        AX = np.stack([blocks_on_separator(ds, s, _seed(name, i), fringe, symmetric)[4] for i in range(batch)])
        AX.setflags(write=False)
        _VALUES[key] = AX
    return _VALUES[key]


# ----------------------------------------------------------------- classification --

Kinds = collections.namedtuple("Kinds", "r w parent kind cls")


def solve_kinds(hip, F):
    """r, w, parent and solve kind ('il', 'small', 'wave', 'big', 'block') of every supernode of the handle F, and its
    factor class (pivot_cases.fronts).  The kind restates symbolic.cpp's solve_kind."""
    FR = pc.fronts(hip, F)
    kind = ["il" if FR.cls[s] == "il" else kind_of(int(FR.r[s]), int(FR.w[s]), F.batch) for s in range(len(FR.w))]
    return Kinds(FR.r, FR.w, np.asarray(FR.parent), kind, FR.cls)


def kind_of(r, w, batch):
    """symbolic.cpp's solve_kind for a front (r, w) that is not matrix-interleaved."""
    if r <= SMALL_RMAX:
        return "small"
    if r <= WAVE_RMAX and w <= WAVE_WMAX:
        return "wave"
    if w > WAVE_WMAX and r >= BIG_RMIN and batch <= BIG_BATCH_MAX:
        return "big"
    return "block"


def wide_fronts(K):
    """Supernodes with w > 64, in supernode order."""
    return [s for s in range(len(K.w)) if K.w[s] > 64]


# ---------------------------------------------------------------------- reference --

def substitute(n, Gp, Gi, Gx, B, lower, trans):
    """Column-oriented substitution in np.longdouble with a triangular CSC factor as Factorization.factors() returns it --
    L (lower) with the diagonal FIRST in its column, U (not lower) with the diagonal LAST -- for every column of B
    ([n] or [n, k]) at once:
      lower, not trans: L x = b (cs_lsolve)      not lower, not trans: U x = b (cs_usolve)
      lower, trans:     L' x = b (cs_ltsolve)    not lower, trans:     U' x = b (cs_utsolve)
    -> x as np.longdouble, shaped like B."""
    X = np.array(B, dtype=np.longdouble, copy=True)
    x = X.reshape(n, -1)
    Gx = np.asarray(Gx, dtype=np.longdouble)
    forward = lower != trans                               # L x = b and U' x = b run down the columns, the others up
    for j in (range(n) if forward else range(n - 1, -1, -1)):
        lo, hi = int(Gp[j]), int(Gp[j + 1])
        dg = lo if lower else hi - 1
        assert Gi[dg] == j, "column %d: the diagonal is not where the layout puts it" % j
        off = slice(lo + 1, hi) if lower else slice(lo, hi - 1)
        rows, vals = Gi[off], Gx[off]
        if trans:                                          # x_j = (b_j - sum_i G_ij x_i) / G_jj
            x[j] = (x[j] - vals @ x[rows]) / Gx[dg]
        else:                                              # x_j = b_j / G_jj, then b_i -= G_ij x_j
            x[j] = x[j] / Gx[dg]
            x[rows] -= vals[:, None] * x[j][None, :]
    return X


def dense64(n, Gp, Gi, Gx, trans=False):
    """A CSC matrix as a dense float64 array (its transpose for trans)."""
    T = np.zeros((n, n))
    T[Gi[:Gp[n]], np.repeat(np.arange(n), np.diff(Gp))] = Gx[:Gp[n]]
    return T.T if trans else T


def dense(n, Gp, Gi, Gx, trans=False):
    """The same in np.longdouble."""
    return dense64(n, Gp, Gi, Gx, trans).astype(np.longdouble)


def substitution_error_ratio(T, x, b):
    """max_i |b - T x|_i / (u (|T||x|)_i) per column, formed in np.longdouble; a row with (|T||x|)_i = 0 must have
    |b - T x|_i = 0 (it counts as ratio 0, anything else as inf).  T dense longdouble [n, n]; x, b [n, k]."""
    x = np.asarray(x, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    E = np.abs(b - T @ x)
    W = np.abs(T) @ np.abs(x)
    u = np.longdouble(2.0) ** -53
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(W > 0, E / (u * W), np.where(E == 0, 0.0, np.inf))
    return ratio.max(axis=0).astype(np.float64)
