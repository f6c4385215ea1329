"""Matrices, Schur sets and the reference of the Schur-complement tests (test_schur_cpu.py, test_gpu_schur.py).

The reference is NumPy float64, dense:  S = A22 - A21 @ solve(A11, A12)  with the blocks taken in the caller's list order.
For grid20k (an interior of 19 700 variables: minutes and 3 GB for the dense solve) that very computation is recorded once
in tests/golden/schur_refs.npz by tests/golden/make_schur_fixtures.py; every other reference is computed here, once per
(matrix, set), and shared."""
import functools
import os

import numpy as np
import scipy.sparse as sp

from csparse3_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _spd(n, seed_shift=1, lower_only=False):
    ei, ej = synth.spd_grid_pattern(n, seed=n)
    return synth.spd_grid_matrix(n, ei, ej, seed=n + seed_shift, lower_only=lower_only)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> (m, n, Ap, Ai, Ax), the matrices of test_gpu_parity.py under their names there."""
    if name == "toy10":
        return synth.toy10()[:5]
    if name == "grid2k":
        return synth.grid_jacobian(n=2000, seed=7)
    if name == "grid20k":
        return synth.grid_jacobian(n=20000, seed=11)
    if name == "denseblock300":
        return synth.dense_block_matrix(n=700, nd=300, seed=1)
    if name == "spd200":
        return _spd(200)
    if name == "spd4000":
        return _spd(4000)
    if name == "spd4000_lower":
        return _spd(4000, lower_only=True)
    raise KeyError(name)


def dense_block_rows():
    """The rows of denseblock300's dense block (synth.dense_block_matrix draws them third from its generator)."""
    rng = np.random.default_rng(1)
    rng.integers(0, 700, size=2100)
    rng.integers(0, 700, size=2100)
    return rng.choice(700, size=300, replace=False)


@functools.lru_cache(maxsize=None)
def _schur_set(name, ns):
    n = matrix(name)[1]
    if name == "toy10":
        assert ns == 3
        return (7, 2, 5)                                   # unsorted
    if name == "denseblock300":
        rows = dense_block_rows()                          # from inside the dense block, in the order they were drawn
        return tuple(int(v) for v in rows[:ns])
    rng = np.random.default_rng(1000 * ns + n)
    return tuple(int(v) for v in rng.choice(n, size=ns, replace=False))      # random buses, unsorted


def schur_set(name, ns):
    return np.asarray(_schur_set(name.replace("_lower", ""), ns), dtype=np.int32)


def to_scipy(n, Ap, Ai, Ax, symmetric_from_lower=False):
    A = sp.csc_matrix((np.asarray(Ax, dtype=np.float64), np.asarray(Ai), np.asarray(Ap)), shape=(n, n))
    if symmetric_from_lower:
        A = (A + sp.tril(A, -1).T).tocsc()
    return A


def split(n, idx):
    """-> (interior ascending, idx)."""
    idx = np.asarray(idx, dtype=np.int64)
    mask = np.ones(n, dtype=bool)
    mask[idx] = False
    return np.flatnonzero(mask), idx


def reference(A, idx):
    """The reference: dense float64 A22 - A21 @ solve(A11, A12), blocks in the order of idx.  A: scipy matrix."""
    n = A.shape[0]
    inter, idx = split(n, idx)
    A = A.tocsr()
    A11 = A[inter][:, inter].toarray()
    A12 = A[inter][:, idx].toarray()
    A21 = A[idx][:, inter].toarray()
    A22 = A[idx][:, idx].toarray()
    return A22 - A21 @ np.linalg.solve(A11, A12)


@functools.lru_cache(maxsize=None)
def reference_of(name, ns):
    """The reference of matrix(name) on schur_set(name, ns), computed once."""
    if name == "grid20k":
        with np.load(os.path.join(GOLDEN, "schur_refs.npz")) as z:
            assert np.array_equal(z["grid20k_idx"], schur_set(name, ns)), "fixture made for another Schur set"
            return z["grid20k_S"].copy()
    m, n, Ap, Ai, Ax = matrix(name)
    return reference(to_scipy(n, Ap, Ai, Ax, symmetric_from_lower=name.endswith("_lower")), schur_set(name, ns))


def condensed_rhs(A, idx, B):
    """b2 - A21 solve(A11, b1), dense float64; B [n] or [n, k]."""
    inter, idx = split(A.shape[0], idx)
    A = A.tocsr()
    return B[idx] - A[idx][:, inter].toarray() @ np.linalg.solve(A[inter][:, inter].toarray(), B[inter])


def interior_pattern(n, Ap, Ai, idx):
    """A11 as the analysis sees it: Schur rows and columns removed, entries in A's order.  -> (interior, n1, Ap11, Ai11)."""
    inter, _ = split(n, idx)
    label = np.full(n, -1, dtype=np.int64)
    label[inter] = np.arange(len(inter))
    Ap11 = np.zeros(len(inter) + 1, dtype=np.int32)
    rows = []
    for k, j in enumerate(inter):
        r = label[np.asarray(Ai[Ap[j]:Ap[j + 1]], dtype=np.int64)]
        r = r[r >= 0]
        rows.append(r)
        Ap11[k + 1] = Ap11[k] + len(r)
    Ai11 = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    return inter.astype(np.int32), len(inter), Ap11, Ai11


def saddle_point(ncon=40, seed=40):
    """[[H, G'], [G, 0]]: H = grid2k, G ncon sparse constraint rows of one to three entries (the first has ONE: a leaf of
    the graph, which a minimum-degree order eliminates first, on its zero diagonal).  No diagonal is stored in the zero
    block.  -> (n, Ap, Ai, Ax, constraint indices, H as scipy, G as dense [ncon, nh])."""
    m, nh, Ap, Ai, Ax = matrix("grid2k")
    H = to_scipy(nh, Ap, Ai, Ax)
    rng = np.random.default_rng(seed)
    G = np.zeros((ncon, nh))
    for i in range(ncon):
        cols = rng.choice(nh, size=1 if i == 0 else int(rng.integers(1, 4)), replace=False)
        G[i, cols] = rng.uniform(0.5, 1.5, size=len(cols)) * rng.choice([-1.0, 1.0], size=len(cols))
    Gs = sp.csc_matrix(G)
    K = sp.bmat([[H, Gs.T], [Gs, None]], format="csc")
    K.sort_indices()
    n = nh + ncon
    return n, K.indptr.astype(np.int32), K.indices.astype(np.int32), K.data.copy(), np.arange(nh, n, dtype=np.int32), H, G


def pendant_zero(ns=33):
    """grid2k plus one variable v = n whose only neighbour is the Schur variable s = schur_set[0] and whose stored diagonal
    is 0.  -> (n + 1, Ap, Ai, Ax, idx, v)."""
    m, n, Ap, Ai, Ax = matrix("grid2k")
    idx = schur_set("grid2k", ns)
    s = int(idx[0])
    A = to_scipy(n, Ap, Ai, Ax).tolil()
    A.resize((n + 1, n + 1))
    A = A.tocoo()
    rows = np.concatenate([A.row, [n, s, n]])
    cols = np.concatenate([A.col, [s, n, n]])
    vals = np.concatenate([A.data, [0.75, -0.6, 0.0]])
    order = np.lexsort((rows, cols))
    Ap2 = np.zeros(n + 2, dtype=np.int64)
    np.add.at(Ap2, cols + 1, 1)
    return (n + 1, np.cumsum(Ap2).astype(np.int32), rows[order].astype(np.int32), vals[order].astype(np.float64), idx, n)


def varied(Ax, t):
    """Values number t of a refactorisation chain / a batch: every entry changed by up to 2 %, t = 0 the matrix itself."""
    if t == 0:
        return np.array(Ax, dtype=np.float64)
    rng = np.random.default_rng(77 + t)
    return Ax * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, size=len(Ax)))


def spd_values(n, t):
    """Values number t of an SPD batch: the pattern of matrix("spd<n>"), another seed."""
    ei, ej = synth.spd_grid_pattern(n, seed=n)
    return synth.spd_grid_matrix(n, ei, ej, seed=n + 1 + t)[4]


# plain handles whose factor schedule is pinned (tests/golden/schur_schedule.npz): (matrix, batch)
SCHEDULE_CASES = (("toy10", 1), ("grid2k", 1), ("grid2k", 130))


def plain_schedule(hip, name, batch):
    """cs3_debug_schedule of a plain LU handle: -> (sched, front_r, front_w)."""
    import ctypes as C
    m, n, Ap, Ai, _ = matrix(name)
    lib = hip.lib()
    i32p = C.POINTER(C.c_int32)
    lib.cs3_debug_schedule.argtypes = [C.c_void_p] + [i32p] * 3
    with hip.Factorization(m, n, Ap, Ai, hip.CS3_LU, hip.ORDER_AMD, batch=batch) as F:
        ns = int(F.info.nsuper)
        out = [np.empty(ns, dtype=np.int32) for _ in range(3)]
        assert lib.cs3_debug_schedule(F._h, *[a.ctypes.data_as(i32p) for a in out]) == 0
    return out
