"""Schur handles at the sizes where k_schur_take, the sweep dispatch and the 256-column chunks change path, for
tests/test_schur_edge_cases_cpu.py and tests/test_gpu_schur_edges.py.

The matrices are sweep_cases.blocks_on_separator(ds, s, fringe): dense diagonal blocks of orders `ds`, each coupled
densely to one dense separator of order s.  The Schur set IS the separator, handed over in a scrambled order (a seeded
permutation), so the analysis keeps exactly one interior front (d + s, d) per block (the chain nodes of `fringe` fold into
their block) below a last supernode (s, s): the Schur front, parentless and alone on the last level.

  case      ds, s                      interior fronts (r, w)           Schur order ns and what it pins
  s5        (1,), 5                    (6, 1)                           5: an interior of ONE variable; SK_SMALL
  s16 s17   (40,) * 4, 16 / 17         (56, 40) / (57, 40)   FC_R64     16 / 17: the order up to which a plain front of a large
                                                                        batch would run lane = matrix; the Schur front never does
  s31-s33   (20,), 31 / 32 / 33        (51..53, 20)          FC_R64     one tile - 1 / one tile / one tile + 1 row; SK_SMALL | SK_WAVE
  s64 s65   (40,) * 4, 64 / 65         (104, 40) / (105, 40) FC_LDS     two tiles / two tiles + 1; SK_WAVE | SK_BLOCK
  s96       (40,) * 4, 96              (136, 40)             FC_LDS     three full tiles (Cholesky mirror without a partial tile)
  s129      (140,) * 2, 129            (269, 140)            FC_BIG     SK_BLOCK Schur front above SK_BIG interior fronts
  s136 s137 (140,) * 2, 136 / 137      (276, 140) / (277, 140) FC_BIG   SK_BLOCK | SK_BIG
  s256 s257 (140,) * 2, 256 / 257      (396, 140) / (397, 140) FC_BIG   one full 256-column chunk / two, the last of one column
  s288mix   (140, 40, 12), 288, fr. 2  (430, 142) (330, 42) (302, 14)   uneven children into one front of 9 tiles per side

The sweep kind of the Schur front follows from ns and the batch alone (r = w = ns: sweep_cases.kind_of); with fewer than
16 right-hand sides an SK_BIG Schur front is a launch group of one front without rows of ancestors, so on the 256-column
path its backward sweep has no init launch (wide_chunk_cases.chunk_width / skips_init).

Reference: schur_cases.reference, dense float64 A22 - A21 @ solve(A11, A12) in the scrambled order.  The bound of the GPU
tests is entry-wise,  |S - S_ref|_ij <= RTOL W_ij  with  W = |A22| + |A21| |A11^-1| |A12|,  the component-wise scale of the
computation: an off-diagonal entry is held to its own size, not to the diagonal's.
"""
import collections

import numpy as np
import scipy.sparse.linalg as spla

import schur_cases as shc
import sweep_cases as sc
import wide_chunk_cases as wc

# name -> (ds, s, fringe)
CASES = {"s5": ((1,), 5, 0), "s16": ((40,) * 4, 16, 0), "s17": ((40,) * 4, 17, 0),
         "s31": ((20,), 31, 0), "s32": ((20,), 32, 0), "s33": ((20,), 33, 0),
         "s64": ((40,) * 4, 64, 0), "s65": ((40,) * 4, 65, 0), "s96": ((40,) * 4, 96, 0),
         "s129": ((140,) * 2, 129, 0), "s136": ((140,) * 2, 136, 0), "s137": ((140,) * 2, 137, 0),
         "s256": ((140,) * 2, 256, 0), "s257": ((140,) * 2, 257, 0), "s288mix": ((140, 40, 12), 288, 2)}
NS = {name: s for name, (_, s, _) in CASES.items()}
ORDER = {name: sum(ds) + s + fringe * len(ds) for name, (ds, s, fringe) in CASES.items()}
# the interior fronts (r, w), one per block, in the order of the blocks
INTERIOR = {name: tuple((d + fringe + s, d + fringe) for d in ds) for name, (ds, s, fringe) in CASES.items()}
# their factor class (symbolic.cpp: front_class) where neither the batch nor the bottom forest changes it
INTERIOR_CLASS = {"s16": "r64", "s17": "r64", "s31": "r64", "s32": "r64", "s33": "r64", "s64": "lds", "s65": "lds", "s96": "lds",
                  "s129": "big", "s136": "big", "s137": "big", "s256": "big", "s257": "big", "s288mix": "big"}
# pivot_cases.fronts names the kernel; the factor class behind it
CLASS_OF_KERNEL = {"forest_wave": "sub", "forest_shared": "sub", "il": "il", "wave": "r32", "mix_wave": "r64", "mix_grid": "r64",
                   "block": "lds", "big_step": "big", "wg": "big", "schur": "schur"}

ST = 32                                        # schur.hip: tile order of k_schur_take
GEMM_MIN = wc.GEMM_MIN                         # right-hand sides from which the GEMM sweeps take the fronts of order > 32
BATCHES_CPU = (1, 2, 7, 16, 130)

# S, entry-wise: every case at batch 1, these beyond
S_BATCHES = {"s33": (2, 7, 16, 130), "s65": (2, 7, 16, 130), "s137": (2, 7, 16, 130), "s257": (2, 7)}
# half-solves: (batch, right-hand sides)
HALF_CASES = ("s5", "s17", "s64", "s65", "s136", "s137", "s257", "s288mix")
HALF_PAIRS = ((1, 1), (1, 7), (1, 8), (1, 16), (1, 70), (2, 3), (2, 4), (7, 1), (15, 1), (16, 1))
HALF_PAIRS_130 = ((130, 1), (130, 3))
HALF_CASES_130 = ("s65", "s137")


def half_pairs(name):
    return HALF_PAIRS + (HALF_PAIRS_130 if name in HALF_CASES_130 else ())


# ------------------------------------------------------------------ construction --

def _seed(name, i, variant=0):
    return 9000 * (1 + list(CASES).index(name)) + 500 * variant + i


def pattern(name, symmetric=False):
    """-> (m, n, Ap, Ai) of case `name`."""
    ds, s, fringe = CASES[name]
    return sc.blocks_on_separator(ds, s, _seed(name, 0), fringe, symmetric)[:4]


_SETS = {}


def schur_set(name):
    """The separator in a scrambled order (int32, read-only)."""
    if name not in _SETS:
        ds, s, _ = CASES[name]
        idx = (sum(ds) + np.random.default_rng(31 * s + len(ds)).permutation(s)).astype(np.int32)
        assert s < 3 or not np.array_equal(idx, np.sort(idx))
        idx.setflags(write=False)
        _SETS[name] = idx
    return _SETS[name]


_VALUES = {}


def values(name, batch, symmetric=False, variant=0):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own; the matrices of a smaller batch
    are the first ones of a larger (built once; read-only).  variant 1: three times the values of other seeds -- what a
    handle is refactorised with."""
    key = (name, symmetric, variant)
    have = _VALUES.get(key)
    if have is None or len(have) < batch:                          # the largest batch asked for so far; smaller ones are views
        ds, s, fringe = CASES[name]
        first = 0 if have is None else len(have)
        more = np.stack([sc.blocks_on_separator(ds, s, _seed(name, i, variant), fringe, symmetric)[4] for i in range(first, batch)])
        if variant:
            more *= 3.0
        have = more if have is None else np.concatenate([have, more])
        have.setflags(write=False)
        _VALUES[key] = have
    return have[:batch]


def scipy_matrix(name, i, symmetric=False, variant=0):
    """Matrix i of the batches of case `name` as a scipy CSC matrix."""
    m, n, Ap, Ai = pattern(name, symmetric)
    have = _VALUES.get((name, symmetric, variant))
    return shc.to_scipy(n, Ap, Ai, (have if have is not None and len(have) > i else values(name, i + 1, symmetric, variant))[i])


# ---------------------------------------------------------------------- reference --

def _blocks(A, idx):
    inter, idx = shc.split(A.shape[0], idx)
    A = A.toarray()
    return A[np.ix_(inter, inter)], A[np.ix_(inter, idx)], A[np.ix_(idx, inter)], A[np.ix_(idx, idx)]


def weight_of(A, idx):
    """W = |A22| + |A21| |A11^-1| |A12|, dense float64, blocks in the order of idx."""
    A11, A12, A21, A22 = _blocks(A, idx)
    return np.abs(A22) + np.abs(A21) @ np.abs(np.linalg.inv(A11)) @ np.abs(A12)


def second_route(A, idx):
    """The Schur complement by another float64 route: a sparse LU of A11 (scipy's SuperLU) applied to A12."""
    inter, idx = shc.split(A.shape[0], idx)
    A = A.tocsc()
    A11 = A[inter][:, inter].tocsc()
    Y = spla.splu(A11).solve(A[inter][:, idx].toarray())
    return A[idx][:, idx].toarray() - A[idx][:, inter].toarray() @ Y


def cond_interior(A, idx):
    """-> (cond_2(A11), cond_2 of A11 with its diagonal scaled to one from both sides).  They differ only where `fringe`
    hangs chain nodes with a diagonal of about 3 beside block rows with one of some hundreds: a scaling, which costs a
    solve with A11 nothing entry-wise."""
    A11 = _blocks(A, idx)[0]
    d = np.sqrt(np.abs(np.diag(A11)))
    return float(np.linalg.cond(A11)), float(np.linalg.cond(A11 / d[:, None] / d[None, :]))


_REFS = {}


def reference(name, i, symmetric=False, variant=0):
    """(S_ref, W) of matrix i of case `name` (computed once; read-only)."""
    key = (name, i, symmetric, variant)
    if key not in _REFS:
        A = scipy_matrix(name, i, symmetric, variant)
        S, W = shc.reference(A, schur_set(name)), weight_of(A, schur_set(name))
        S.setflags(write=False)
        W.setflags(write=False)
        _REFS[key] = (S, W)
    return _REFS[key]


def weight(name, i, symmetric=False, variant=0):
    return reference(name, i, symmetric, variant)[1]


def entrywise_ratio(S, name, i, symmetric=False, variant=0):
    """max_ij |S - S_ref|_ij / W_ij of matrix i (W > 0 everywhere: asserted by the CPU tests)."""
    want, W = reference(name, i, symmetric, variant)
    return float((np.abs(S - want) / W).max())


def transposed_tile_margin(S, W):
    """min over the ST x ST tiles of S of  max_ij-in-the-tile |S - S'|_ij / W_ij  (tiles of one diagonal entry left out):
    what ANY transposed tile of k_schur_take would miss the entry-wise bound by.  The guard of the LU cases; the norm-wise
    form rel_err(S, S') cannot serve, its scale max|S| being a diagonal entry that grows with ns (6.8e-3 at ns = 64)."""
    ns = S.shape[0]
    D = np.abs(S - S.T) / W
    nt = -(-ns // ST)
    tiles = [D[ST * ti:ST * (ti + 1), ST * tj:ST * (tj + 1)] for ti in range(nt) for tj in range(nt)]
    return float(min(t.max() for t in tiles if t.size > 1))


def half_solve_reference(name, i, symmetric, B, variant=0):
    """-> (g, x): the condensed right-hand side b2 - A21 solve(A11, b1) (schur_cases.condensed_rhs) and the solution of
    A x = B formed from x2 = solve(S_ref, g), x1 = solve(A11, b1 - A12 x2); dense float64.  B [n] or [n, k]."""
    A = scipy_matrix(name, i, symmetric, variant)
    idx = schur_set(name)
    g = shc.condensed_rhs(A, idx, B)
    inter, _ = shc.split(A.shape[0], idx)
    A11, A12, _, _ = _blocks(A, idx)
    x = np.empty_like(B)
    x[idx] = np.linalg.solve(reference(name, i, symmetric, variant)[0], g)
    x[inter] = np.linalg.solve(A11, B[inter] - A12 @ x[idx])
    return g, x


# -------------------------------------------------------------------- sweep plans --

Plan = collections.namedtuple("Plan", "kind path cw nchunk no_init")


def schur_kind(ns, batch):
    """The sweep kind of the Schur front (ns, ns): never matrix-interleaved (FC_SCHUR), so ns and the batch decide."""
    return sc.kind_of(ns, ns, batch)


def sweep_plan(ns, batch, k):
    """How the Schur front of order ns is swept with k right-hand sides per matrix (kernels.hip: launch_solve_group,
    big_sweep_plan).  path: 'rhs' (lane = right-hand side), 'gemm', 'wave', 'block' or 'big'; for 'big' the columns per
    chunk launch, the chunks, and whether the backward sweep skips its init launch."""
    kind = schur_kind(ns, batch)
    if k >= GEMM_MIN:
        return Plan(kind, "rhs" if kind == "small" else "gemm", 0, 0, False)
    if kind != "big":
        return Plan(kind, "wave" if kind in ("small", "wave") else "block", 0, 0, False)
    cw = wc.chunk_width(batch, k, ns)
    return Plan(kind, "big", cw, -(-ns // cw), wc.skips_init(batch, k, [(ns, ns)]))
