"""Matrices that put the selected inversion (selinv.hip, selinv.cpp) at the edges of its chunks, slices, tiles and launch
groups, for tests/test_selinv_edge_cases_cpu.py and tests/test_gpu_selinv_edges.py.  Nothing here needs a GPU.

Every matrix is sweep_cases.blocks_on_separator(ds, s, seed, fringe, symmetric): dense blocks of orders ds, each coupled
densely to one dense separator of order s.  The analysis (AMD) keeps some blocks as fronts (d + s, d) under a root that
absorbs the separator and the other blocks, so (r, w) of a front with a contribution block and a parent is chosen by
(d, s).  TABLE states what the analysis makes of every case; the CPU test holds the analysis to it, so a case cannot
leave its edge unnoticed.  Sizes that are meant to sit at a limit of a kernel come from cs3_selinv_limits().

A case is (m, n, Ap, Ai, Ax) as csparse3_amd.synth returns it; Ap / Ai int32, Ax float64.
"""
import collections

import numpy as np

import selinv_cases as sc
import sweep_cases
from csparse3_amd import csc_hip as hip

LIMITS = sc.LIMITS
L, WV = int(LIMITS.lds_max_order), int(LIMITS.wave_max_order)      # largest order of the LDS class and of the wave class
T, D = int(LIMITS.gemm_tile), int(LIMITS.diag_block)               # the MFMA tile, the chunk of tri_slice
S = T                                                              # vectors per slice of tri_slice: 256 threads, 16 per vector
WAVES = 4                                                          # fronts per workgroup of the wave class; tiles per workgroup

# name -> (ds, s, fringe); two_trees: the block diagonal of two of them.  A fringe does not stay below its block: the
# analysis merges the upper nodes of every chain into the block's front (w grows by 4 at fringe 6, by 12 at fringe 12),
# and with a chain of its own below it a big front moves one level up.  So `mixed` (fringe 12) has three big shapes on
# two levels and one small front below a big one, `mixed0` is the same without a fringe: (142, 72) and (170, 100) in one
# group; `l33` has no fringe, and `l33f` takes d = 12 so that d + 4 + s is the first LDS order, with small fronts below.
SPEC = {
    "w40": ((40,) * 4, 110, 0),
    "w64": ((D,) * 4, 5 * T, 0),
    "w65": ((D + 1,) * 4, 5 * T, 0),
    "w128": ((2 * D,) * 4, T, 0),
    "w129": ((2 * D + 1,) * 4, T + 1, 0),
    "c1": ((140,) * 4, 1, 0),
    "c15": ((140,) * 4, T - 1, 0),
    "r137": ((100,) * 4, L + 1 - 100, 0),
    "w8": ((8,) * 4, L, 0),
    "mixed": ((72, 100, 130, 90), 70, 12),
    "mixed0": ((72, 100, 130, 90), 70, 0),
    "w72": ((72,) * 4, 70, 0),
    "l136": ((60,) * 4, L - 60, 0),
    "l70": ((40,) * 4, 30, 0),
    "l33": ((16,) * 4, WV + 1 - 16, 0),
    "l33f": ((12,) * 4, WV + 1 - 16, 6),
    "v32x3": ((20,) * 4, WV - 20, 0),
    "v32x5": ((12,) * 7, WV - 12, 0),
    "v32c1": ((WV - 1,) * 4, 1, 0),
    "v31": ((16,) * 4, WV - 1 - 16, 0),
}
TWO_TREES = ("w72", "r137")
CASES = [name for name in SPEC if name != "w72"] + ["two_trees"]

# What the analysis makes of a case: `fronts`, the (r, w, order of the parent) of every front that is not a root and is
# beyond the wave class, or every such front at all where `rest` is 0; `roots`, the orders of the roots; `rest`, the
# number of further fronts, all of the wave class; `groups`, the launch groups in launch order as (class, fronts);
# `edge`, what the case is there for.
Expect = collections.namedtuple("Expect", "fronts roots rest groups edge")
TABLE = {
    "w40": Expect([(150, 40, 190)] * 2, [190], 0, [("big", 1), ("big", 2)], "one ragged chunk, w < 64"),
    "w64": Expect([(144, 64, 208)] * 2, [208], 0, [("big", 1), ("big", 2)], "one full chunk; c = 5 full slices"),
    "w65": Expect([(145, 65, 210)] * 2, [210], 0, [("big", 1), ("big", 2)], "a last chunk of one pivot"),
    "w128": Expect([(144, 128, 272)] * 2, [272], 0, [("big", 1), ("big", 2)], "two full chunks; c = one full slice and tile"),
    "w129": Expect([(146, 129, 275)] * 2, [275], 0, [("big", 1), ("big", 2)], "three chunks; a second slice of one vector"),
    "c1": Expect([(141, 140, 281)] * 2, [281], 0, [("big", 1), ("big", 2)], "c = 1"),
    "c15": Expect([(155, 140, 295)] * 2, [295], 0, [("big", 1), ("big", 2)], "c = 15"),
    "r137": Expect([(137, 100, 237)] * 2, [237], 0, [("big", 1), ("big", 2)], "the smallest big front, not a root"),
    "w8": Expect([(144, 8, 160)], [160], 0, [("big", 1), ("big", 1)], "w < one tile and slice, c = 136"),
    "mixed": Expect([(166, 96, 212), (154, 84, 212), (182, 112, 212)], [212], 1, [("big", 1), ("big", 1), ("wave", 1), ("big", 2)],
                    "two shapes in one big group; four launch groups; a small front under a big one that has a parent"),
    "mixed0": Expect([(142, 72, 290), (170, 100, 290)], [290], 0, [("big", 1), ("big", 2)], "two shapes in one big group, no fringe"),
    "two_trees": Expect([(142, 72, 214)] * 2 + [(137, 100, 237)] * 2, [214, 237], 0, [("big", 2), ("big", 4)],
                        "two roots in one group; four big fronts of two shapes with two parents in one group"),
    "l136": Expect([(136, 60, 136)] * 3, [136], 0, [("lds", 1), ("lds", 3)], "the largest LDS image with c > 0"),
    "l70": Expect([(70, 40, 70)] * 3, [70], 0, [("lds", 1), ("lds", 3)], "ragged tiles on both sides"),
    "l33": Expect([(33, 16, 49)] * 2, [49], 0, [("lds", 1), ("lds", 2)], "the first LDS order, with c > 0"),
    "l33f": Expect([(33, 16, 35)] * 3, [35], 3, [("lds", 1), ("lds", 3), ("wave", 3)], "the first LDS order, with c > 0 and wave fronts below"),
    "v32x3": Expect([(32, 20, 32)] * 3, [32], 0, [("wave", 1), ("wave", 3)], "three fronts in one workgroup"),
    "v32x5": Expect([(32, 12, 44)] * 5, [44], 0, [("lds", 1), ("wave", 5)], "4 + 1 fronts"),
    "v32c1": Expect([(32, 31, 32)] * 3, [32], 0, [("wave", 1), ("wave", 3)], "c = 1 at ld = 33"),
    "v31": Expect([(31, 16, 47)] * 2, [47], 0, [("lds", 1), ("wave", 2)], "an odd order: ld = r"),
}
assert sorted(TABLE) == sorted(CASES)


def class_of(r):
    """selinv.cpp's class_of."""
    return "wave" if r <= WV else "lds" if r <= L else "big"


def kinds(name):
    """Every case by LU; those with a front beyond the wave class that is not a root also by Cholesky."""
    return ("lu", "chol") if any(class_of(r) != "wave" for r, _, _ in TABLE[name].fronts) else ("lu",)


GPU_CASES = [(name, kind) for name in CASES for kind in kinds(name)]
RESTATED_CHOLESKY = ("w129", "l136")               # the Cholesky cases whose restatement the CPU test holds to the dense inverse


# ------------------------------------------------------------------ construction --

def _seed(name, i):
    return 7000 + 100 * list(SPEC).index(name) + i


def _one(name, i, symmetric):
    ds, s, fringe = SPEC[name]
    return sweep_cases.blocks_on_separator(ds, s, _seed(name, i), fringe, symmetric)


def block_diagonal(a, b):
    """diag(A, B) of two square CSC cases."""
    na, nb = a[1], b[1]
    Ap = np.concatenate([a[2][:na], a[2][na] + b[2][:nb + 1]]).astype(np.int32)
    Ai = np.concatenate([a[3][:a[2][na]], na + b[3][:b[2][nb]]]).astype(np.int32)
    return na + nb, na + nb, Ap, Ai, np.concatenate([a[4][:a[2][na]], b[4][:b[2][nb]]])


_MATRICES = {}


def matrix(name, i=0, symmetric=False):
    """Matrix i of case `name` (the pattern does not depend on i: matrices of one case form a batch); built once, read-only."""
    key = (name, i, symmetric)
    if key not in _MATRICES:
        if name == "two_trees":
            case = block_diagonal(*(_one(part, i, symmetric) for part in TWO_TREES))
        else:
            case = _one(name, i, symmetric)
        case[4].setflags(write=False)
        _MATRICES[key] = case
    return _MATRICES[key]


def tridiagonal(n, i=0):
    """selinv_cases.tridiagonal's pattern with diagonally dominant values that depend on i: nnz = 3 n - 2."""
    k = np.arange(n - 1)
    rows = np.concatenate([np.arange(n), k + 1, k])
    cols = np.concatenate([np.arange(n), k, k + 1])
    vals = np.concatenate([4.0 + 0.5 * np.cos(np.arange(n) + i), -1.0 - 0.3 * np.sin(k + i), -1.5 + 0.3 * np.cos(2 * k + i)])
    return sc._csc(n, rows, cols, vals)


GETTER_ORDERS = (255, 256, 257)                    # k_selinv_gather has 256 threads: n on either side of one workgroup


# ------------------------------------------------------------------------ the plan --

Front = collections.namedtuple("Front", "s r w c parent launch cls")


def plan_fronts(F):
    """The fronts of an analysed handle in the order the selected inversion computes them: supernode, r, w, c = r - w, the
    parent supernode (-1: a root), the index of the group's first launch (F.selinv_plan()), and the class from r."""
    ns = int(F.info.nsuper)
    sched, r, w = (np.empty(ns, dtype=np.int32) for _ in range(3))
    hip._check(hip.lib().cs3_debug_schedule(F._h, hip._pi(sched), hip._pi(r), hip._pi(w)))
    R, W = np.empty(ns, dtype=np.int64), np.empty(ns, dtype=np.int64)
    R[sched], W[sched] = r, w
    parent = F.supernodes()[1]
    front, launch, _, _ = F.selinv_plan()
    return [Front(int(s), int(R[s]), int(W[s]), int(R[s] - W[s]), int(parent[s]), int(launch[t]), class_of(int(R[s])))
            for t, s in enumerate(front)]


def analysed(name, kind="lu", batch=1):
    case = matrix(name, 0, kind == "chol")
    return hip.Factorization(case[0], case[1], case[2], case[3], hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU,
                             hip.ORDER_AMD, batch=batch)


def groups(fronts):
    """The launch groups in launch order: lists of fronts with one launch index."""
    by = collections.OrderedDict()
    for f in fronts:
        by.setdefault(f.launch, []).append(f)
    return list(by.values())


def _ceil(a, b):
    return -(-a // b)


def big_grids(f):
    """(grid_prep, grid_cross, grid_pivot) that a big front asks for alone (selinv.cpp: build_selinv_plan)."""
    gather = max(1, min(256, _ceil(f.c * f.c, 4096)))
    tc, tw = _ceil(f.c, T), _ceil(f.w, T)
    return 2 * _ceil(f.c, S) + _ceil(f.w, S) + gather, max(1, _ceil(2 * tc * tw, WAVES)), _ceil(tw * tw, WAVES)


def _below(fronts, cls):
    """Fronts of a class that have a contribution block (and so a parent)."""
    return [f for f in fronts if f.cls == cls and f.c > 0]


def _big_groups(fronts):
    return [g for g in groups(fronts) if g[0].cls == "big"]


def _surplus(fronts, which):
    """A big front in a group whose grid `which` is larger than the front's own."""
    return any(big_grids(f)[which] < max(big_grids(h)[which] for h in g) for g in _big_groups(fronts) for f in g)


def edges():
    """name -> predicate over a case's plan_fronts(): the edges of selinv.hip / selinv.cpp that the cases are there for.
    An edge is covered when the predicate holds for at least one case."""
    big, lds, wave = (lambda F: _below(F, "big")), (lambda F: _below(F, "lds")), (lambda F: _below(F, "wave"))
    wave_groups = lambda F: [g for g in groups(F) if g[0].cls == "wave" and all(f.c > 0 for f in g)]
    E = collections.OrderedDict()
    # tri_slice with X and Y
    E["one ragged chunk: w < diag_block"] = lambda F: any(f.w < D for f in big(F))
    E["one full chunk: w = diag_block"] = lambda F: any(f.w == D for f in big(F))
    E["two full chunks: w = 2 diag_block"] = lambda F: any(f.w == 2 * D for f in big(F))
    E["a last chunk of one pivot behind one chunk"] = lambda F: any(f.w == D + 1 for f in big(F))
    E["a last chunk of one pivot behind two chunks"] = lambda F: any(f.w == 2 * D + 1 for f in big(F))
    E["X and Y over three chunks or more"] = lambda F: any(f.w > 2 * D for f in big(F))
    E["w < one slice: nsw = 1, nv = w"] = lambda F: any(f.w < S for f in big(F))
    E["c = 1: a slice of one vector"] = lambda F: any(f.c == 1 for f in big(F))
    E["c = slice - 1"] = lambda F: any(f.c == S - 1 for f in big(F))
    E["c = slice: one full slice"] = lambda F: any(f.c == S for f in big(F))
    E["c = slice + 1: a second slice of one vector"] = lambda F: any(f.c == S + 1 for f in big(F))
    E["c a multiple of the slice above one"] = lambda F: any(f.c % S == 0 and f.c > S for f in big(F))
    # grids of a group
    E["a big group with two shapes"] = lambda F: any(len({(f.r, f.w) for f in g}) > 1 for g in _big_groups(F))
    E["surplus workgroups of k_selinv_big_prep"] = lambda F: _surplus(F, 0)
    E["surplus workgroups of k_selinv_big_product<1>"] = lambda F: _surplus(F, 1)
    E["surplus workgroups of k_selinv_big_product<2>"] = lambda F: _surplus(F, 2)
    E["a big group whose fronts have different parents"] = lambda F: any(len({f.parent for f in g if f.parent >= 0}) > 1 for g in _big_groups(F))
    E["a big group with two roots"] = lambda F: any(sum(f.parent < 0 and f.c == 0 for f in g) >= 2 for g in _big_groups(F))
    E["work buffer: big fronts with unequal 2 c w"] = lambda F: len({2 * f.c * f.w for f in big(F)}) > 1
    E["the smallest big front below a root"] = lambda F: any(f.r == L + 1 for f in big(F))
    E["small fronts under big fronts that have a parent"] = lambda F: any(f.cls == "wave" and any(p.s == f.parent and p.cls == "big" and p.parent >= 0 for p in F) for f in F)
    # k_selinv_lds<256>
    E["the largest LDS front with c > 0"] = lambda F: any(f.r == L for f in lds(F))
    E["the smallest LDS front with c > 0"] = lambda F: any(f.r == WV + 1 for f in lds(F))
    E["LDS front with ragged tiles of c and of w"] = lambda F: any(f.c % T and f.w % T and f.c > T and f.w > T for f in lds(F))
    # k_selinv_lds<64>
    E["the largest wave front with c > 0"] = lambda F: any(f.r == WV for f in wave(F))
    E["a wave front of odd order with c > 0"] = lambda F: any(f.r == WV - 1 for f in wave(F))
    E["c = 1 at the largest wave front"] = lambda F: any(f.r == WV and f.c == 1 for f in wave(F))
    E["a wave group of three: the fourth wave returns"] = lambda F: any(len(g) == WAVES - 1 and g[0].r == WV for g in wave_groups(F))
    E["a wave group of five: a second workgroup with one front"] = lambda F: any(len(g) == WAVES + 1 and g[0].r == WV for g in wave_groups(F))
    return E
