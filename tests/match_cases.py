"""Matrices without a strong diagonal for the tests of matching + scaling (tests/test_matching_cpu.py,
tests/test_gpu_matching.py): Jacobians scrambled by a row permutation and row / column scalings over eight decades, and
saddle-point (KKT) systems with a zero diagonal block.  Each case is the smallest that reaches its kernel class.

scramble: A = (D0 J D1)[perm, :].  Where J is strictly row-dominant its diagonal is the unique maximum-product
transversal (around any cycle every off-diagonal entry is smaller than the diagonal of its row; scalings change the product
of every transversal by the same factor), so the expected rowperm is known exactly: rowperm[j] = the position of row j of
J in A.  synth.jacobian_like() is NOT row-dominant (its weakest row has |diagonal| = 0.07 of the rest), its best
transversal leaves the diagonal in 100 columns, and the case has no expected permutation: KNOWN lists the cases that have."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from csparse3_amd import synth

Case = namedtuple("Case", "name n Ap Ai Ax batch expect_rowperm classes")


def _csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def scramble(mat, seed, span=4):
    """-> (n, Ap, Ai, Ax, expected rowperm or None)"""
    m, n, Ap, Ai, Ax = mat
    r = np.random.default_rng(seed)
    d0 = 10 ** r.uniform(-span, span, n)
    d1 = 10 ** r.uniform(-span, span, n)
    perm = r.permutation(n)
    J = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    A = (sp.diags(d0) @ J @ sp.diags(d1)).tocsr()[perm, :]
    absj = abs(J)
    diag = absj.diagonal()
    dominant = bool((diag > np.asarray(absj.sum(axis=1)).ravel() - diag).all())
    # row j of J sits at position argsort(perm)[j] of A
    return _csc(A) + (np.argsort(perm).astype(np.int32) if dominant else None,)


def kkt(nh, ng, seed):
    """[[H, G'], [G, 0]] -> (n, Ap, Ai, Ax, None)"""
    _, _, Hp, Hi, Hx = synth.spd_grid_matrix(nh, *synth.spd_grid_pattern(nh, seed=seed), seed=seed + 1, shift=0.5)
    H = sp.csc_matrix((Hx, Hi, Hp), shape=(nh, nh))
    r = np.random.default_rng(seed)
    cols = r.integers(0, nh, 3 * ng)
    vals = r.uniform(0.5, 1.5, 3 * ng) * r.choice([-1, 1], 3 * ng)
    G = sp.csr_matrix((vals, cols, 3 * np.arange(ng + 1)), shape=(ng, nh))
    G.sum_duplicates()
    return _csc(sp.bmat([[H, G.T], [G, None]], format="csc")) + (None,)


# name -> (builder, batch, the kernel classes (pivot_cases.fronts) the case is there for)
_BUILD = {
    "jac200": (lambda: scramble(synth.jacobian_like(), 3), 1, ("forest_wave",)),
    "grid3000": (lambda: scramble(synth.grid_jacobian(3000, seed=13), 1), 1, ("forest_wave", "forest_shared", "mix_wave")),
    "db100": (lambda: scramble(synth.dense_block_matrix(220, 100, seed=1100), 4), 1, ("block",)),
    "db180": (lambda: scramble(synth.dense_block_matrix(300, 180, seed=1180), 2), 1, ("big_step",)),
    "kkt400": (lambda: kkt(400, 150, 8), 1, ()),
    "kkt2000": (lambda: kkt(2000, 300, 7), 1, ()),
    "db48x20": (lambda: scramble(synth.dense_block_matrix(168, 48, seed=1048), 5), 20, ("wave", "block")),
}
NAMES = list(_BUILD)
KNOWN = ("grid3000", "db100", "db180", "db48x20")      # scrambles of a strictly row-dominant J: rowperm is known exactly
SINGLE = [k for k in NAMES if _BUILD[k][1] == 1]
_CASES = {}


def case(name):
    """The case by name, built once per process."""
    if name not in _CASES:
        build, batch, classes = _BUILD[name]
        n, Ap, Ai, Ax, expect = build()
        _CASES[name] = Case(name, n, Ap, Ai, Ax, batch, expect, classes)
    return _CASES[name]


def batch_values(c, seed=77):
    """[batch, nnz]: the case's values * (1 + 0.05 U(-1, 1)) per entry, one set per matrix of the batch."""
    r = np.random.default_rng(seed)
    return c.Ax[None, :] * (1.0 + 0.05 * r.uniform(-1.0, 1.0, (c.batch, len(c.Ax))))


def scaled(c, Ax, rowperm, dr, dc):
    """B of the header's definition, bit for bit: (n, Ap, rowinv[Ai], (dr[i] * a_ij) * dc[j]) in A's entry order."""
    rowinv = np.argsort(rowperm).astype(np.int32)
    col = np.repeat(np.arange(c.n), np.diff(c.Ap))
    return c.Ap, rowinv[c.Ai], (dr[c.Ai] * Ax) * dc[col]


def weight(c, rowperm):
    """sum_j log |A[rowperm[j], j]| (-inf when the transversal leaves the pattern or meets a stored zero)."""
    A = sp.csc_matrix((c.Ax, c.Ai, c.Ap), shape=(c.n, c.n))
    a = np.abs(np.asarray(A[rowperm, np.arange(c.n)]).ravel())
    with np.errstate(divide="ignore"):
        return float(np.log(a).sum())


def shuffled_columns(c, seed=5):
    """The same matrix with the entries inside each column in random order."""
    r = np.random.default_rng(seed)
    Ai, Ax = c.Ai.copy(), c.Ax.copy()
    for j in range(c.n):
        lo, hi = c.Ap[j], c.Ap[j + 1]
        p = lo + r.permutation(hi - lo)
        Ai[lo:hi], Ax[lo:hi] = c.Ai[p], c.Ax[p]
    return c._replace(Ai=Ai, Ax=Ax)
