"""NumPy / SciPy restatement of the sparse right-hand-side path (cs3_sens_*: csrc/sens.hip and cs3_sens_plan in
csrc/apps.cpp): how a plan groups its solved-for columns into tiles, which side it picks, and Y = C op(A)^-1 B computed
both ways -- from the right, C @ splu(op(A)).solve(B), and from the left, (splu(op(A)').solve(C'))' @ B.

An operand is an Op(ncols, indptr, indices, values): B by columns (n x ncols), C by rows, i.e. the CSC arrays of C'."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

Op = namedtuple("Op", "ncols indptr indices values")

RIGHT, LEFT = 1, 2
SIDES = {"auto": 0, "right": RIGHT, "left": LEFT}


def to_scipy(op, n):
    """The n x ncols matrix of an operand (duplicates add when it is densified)."""
    return sp.csc_matrix((np.asarray(op.values, dtype=np.float64), np.asarray(op.indices), np.asarray(op.indptr)),
                         shape=(n, op.ncols))


def dense(op, n):
    """... densified, duplicates added in storage order as the kernel adds them."""
    D = np.zeros((n, op.ncols))
    cols = np.repeat(np.arange(op.ncols), np.diff(np.asarray(op.indptr)))
    np.add.at(D, (np.asarray(op.indices), cols), np.asarray(op.values, dtype=np.float64))      # unbuffered: one entry at a time
    return D


def choose_side(k, p, side=0, b_ident=False, c_ident=False):
    """The side a plan takes: an identity operand forces the other side, a request is honoured, auto solves for the
    fewer columns and a tie goes right."""
    if b_ident:
        return LEFT
    if c_ident:
        return RIGHT
    if side:
        return side
    return LEFT if p < k else RIGHT


def tiles(ns, limits, tile_env=None):
    """[(first column, columns, solve width)] of ns solved-for columns: tiles of the tile width in order; a tile narrower
    than pad_width is padded to it unless the tile width itself is lower."""
    cap = limits.max_tile if tile_env is None else min(limits.max_tile, max(1, int(tile_env)))
    out = []
    for c0 in range(0, ns, cap):
        t = min(cap, ns - c0)
        w = limits.pad_width if (t < limits.pad_width and cap >= limits.pad_width) else t
        out.append((c0, t, w))
    return out


def info_ref(n, k, p, nnz_b, nnz_c, limits, side=0, trans=False, tile_env=None):
    """What cs3_sens_info must report (nnz_b / nnz_c None: an identity operand)."""
    s = choose_side(k, p, side, nnz_b is None, nnz_c is None)
    tl = tiles(k if s == RIGHT else p, limits, tile_env)
    assert len({w for _, _, w in tl}) <= 2, "at most two solve widths per plan"
    return dict(k=k, p=p, side=s, trans=int(bool(trans)), ntiles=len(tl), max_width=max(w for _, _, w in tl),
                nnz_b=n if nnz_b is None else nnz_b, nnz_c=n if nnz_c is None else nnz_c)


def _lu(A, trans):
    return spla.splu((A.T if trans else A).tocsc())


def y_right(A, B, Ct, trans=False):
    """C @ op(A)^-1 B; B / Ct None = the identity."""
    n = A.shape[0]
    Bd = np.eye(n) if B is None else dense(B, n)
    X = _lu(A, trans).solve(Bd)
    return X if Ct is None else dense(Ct, n).T @ X


def y_left(A, B, Ct, trans=False):
    """(op(A)^-T C')' @ B."""
    n = A.shape[0]
    Cd = np.eye(n) if Ct is None else dense(Ct, n)
    Z = _lu(A, not trans).solve(Cd)
    return Z.T if B is None else Z.T @ dense(B, n)
