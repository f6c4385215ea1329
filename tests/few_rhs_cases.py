"""Matrices with a prescribed assembly tree for the sweeps of 1 to 15 right-hand sides on the level schedule, and a
restatement of what decides the kernel that sweeps a front there and of the forward assembly lists it reads, for
tests/test_few_rhs_cases_cpu.py and tests/test_gpu_few_rhs_edges.py.

The trees are built with the builder of tests/rhs_cases.py (natural order, dense cliques, diagonally dominant values, a
pattern that does not depend on the seed, `symmetric` for Cholesky) and registered there under 'few_<name>'.

What the relaxed amalgamation (symbolic.cpp, step 5b) does to them, and how the trees stand up to it.  A front absorbs
its LAST child -- the one with the tallest column subtree -- when that adds few explicit zeros, one child per pass, four
passes.  It never does when that would push two fronts of order <= 136 past 136 rows, nor (beyond 8 pivots, between 33
and 136 rows) with more than a quarter of zeros: `_guard`, a wide leaf coupled to its parent's first column alone, is
such a child and is put last wherever a front of order <= 136 has to stay as written.  A front of more than 136 rows
has no such protection in the first pass; after it, it absorbs nothing that would start another block of 32 pivots.  So
a front that is to have 64 pivots and more than 136 rows is written down with 63, and its tallest child is one column
(`_sacrifice`, or a single-column leaf) that it absorbs.

With fewer than 16 right-hand sides a front is swept (api.cpp: select_sweep_schedule; schedule.cpp: sweep_groups,
absorb_small_group, launch_solve_group) by
  the bottom forest's own sweeps   one plain right-hand side of a lone matrix, the fronts of the forest ('sub'),
  k_fwd_il / k_bwd_il              order <= 16 in a batch of 128 or more ('il'),
  k_fwd_wave / k_bwd_wave<1 | 8>   order <= 32 ('small') and r <= 128, w <= 64 ('wave'): the two groups of a level are
                                   one launch, four fronts per workgroup; <1> for one right-hand side, <8> beyond,
  k_fwd_blk / k_bwd_blk            everything else that is not 'big' ('block') -- and, for a lone matrix, the wave group of
                                   its level when that holds at most 16 fronts and sits next to it in the schedule,
  the big-front sweeps             w > 64 and r > 136 in a batch of at most 15 ('big': no tree of this module has one).
`dispatch()` restates that, `lists()` the forward assembly list of every front (emit_runs in symbolic.cpp) from the
fronts' row structures: a change of dispatch, of the list layout or of the amalgamation's prices then fails an assertion
of tests/test_few_rhs_cases_cpu.py instead of leaving an edge silently unreached.
"""
import collections

import numpy as np
import scipy.sparse as sp

import pivot_cases as pc
import rhs_cases as rc
import sweep_cases as sc
from rhs_cases import _leaves, _node

FEW_RHS_MAX = rc.RHS_LANES_MIN - 1     # schedule.cpp: sweep_groups regroups below RHS_LANES_MIN
PROMOTE_MAX = 16                       # cs3_device.hpp: PROMOTE_MAX
WAVES_PER_WG = 4                       # kernels.hip: k_fwd_wave / k_bwd_wave, fronts per workgroup
KT = 8                                 # kernels.hip: launch_solve_group, right-hand sides per wave
SOLVE_PF = 8                           # kernels.hip: panel columns prefetched at a time
SOLVE_BW = 64                          # kernels.hip: the triangles of the block kernels
CHUNK = 64                             # symbolic.cpp: emit_runs; kernels.hip: one wave per 64 entries of a list
GATHER_CHUNKS = 16                     # kernels.hip: gather_front, 4 waves x GATHER_UNROLL chunks per pass
BATCHES = (1, 4, 20, 130)


# ------------------------------------------------------------------ construction --

def _guard(w=10):
    """A wide leaf coupled to its parent's first column alone, taller than its siblings: the last child, and too
    expensive to absorb for a parent of order <= 136."""
    return _node(w, (1, 0))


def _row0(count):
    """Single-column leaves coupled to the parent's first column alone: each adds one source to the parent's row 0."""
    return [_node(1, (1, 0)) for _ in range(count)]


def _sacrifice(widths, k=60):
    """One column coupled to k entries of the parent, over a chain of wide leaves (taller than every sibling).  The
    parent absorbs the column; the chain's fronts (w + 1, w) stay: 61 rows + w columns is past 136 for the column, and
    the merged parent would start another block of pivots."""
    c = None
    for w in widths:
        c = _node(w, (1, 0), [c] if c else [])
    return _node(1, (k, 0), [c])


def _wave():
    a = _node(8, (56, 0), _row0(61) + [_guard()])                          # (64, 8): row 0 has 1 + 61 + 1 = 63 sources
    b = _node(9, (56, 1), _row0(62) + [_guard()])                          # (65, 9): 64
    c = _node(13, (33, 2), _row0(63) + [_guard()])                         # (46, 13): 65, a long run
    d = _node(13, (39, 3), _row0(64) + [_guard()])                         # (52, 13): 66
    e = _node(1, (32, 0), _leaves(3, 1, 2) + [_guard()])                   # (33, 1) above the leaves
    f = _node(63, (64, 4))                                                 # (127, 63)
    g = _node(64, (64, 0))                                                 # (128, 64), the tallest child of p: 137 rows with it
    p = _node(60, (13, 0), [a, b, c, d, e, _node(1, (32, 1)), f, g])       # (73, 60): ancestors in rows 60 .. 72
    return _node(64, None, [p])                                            # (64, 64)


def _block():
    # the chain p1 (r = 262), p2 (199), p3 (136) of fronts of 64 pivots under p4 = (136, 129)
    kids = [_node(8, (k, 0)) for k in (200, 255, 256, 257)]                # w = 8 with 255, 256, 257 ancestors
    p1 = _node(63, (198, 0), kids + [_sacrifice([20])])
    p2 = _node(63, (135, 0), [p1, _sacrifice([90])])
    p3 = _node(63, (72, 0), [p2, _sacrifice([81, 81])])
    # q = (136, 64) with 65 leaves on its rows 0 and 62 (a leaf more would be past 136 rows: q absorbs none).  Its list: row 0
    # a long run (two entries), rows 1 .. 61 one entry each, and the long run of row 62 would start at position 63
    q = _node(64, (72, 0), [_node(1, (2, 61)) for _ in range(65)])
    leaves = [_node(64, (65, 0)), _node(64, (73, 0)), _node(65, (35, 1)), _node(31, (100, 0)), _node(32, (100, 1)), _node(33, (100, 2))]
    p4 = _node(129, (7, 0), leaves + [q, p3])
    return _node(20, None, [_node(128, (8, 0)), p4])


def _promote(small):
    """`small` leaves of order <= 32, a leaf (34, 9) and a leaf (138, 8) under a root (130, 130); the extra small leaf of
    promote17 comes last, so that every other column has the same number in both trees.  (The leaf of 9 pivots is the
    tallest child, and 9 + 130 rows are past 136.)"""
    def tree():
        lv = [_node(1 + i % 5, (min(2 + 2 * i, 27), i % 3)) for i in range(15)]      # orders 3 .. 32, seven of them <= 16
        return _node(130, None, lv + [_node(9, (25, 0)), _node(8, (130, 0))] + [_node(3, (9, 1)) for _ in range(small - 15)])
    return tree


TREES = {"wave": _wave, "block": _block, "promote16": _promote(15), "promote17": _promote(16)}
SEEDS = {"wave": 210000, "block": 220000, "promote16": 230000, "promote17": 230000}
for _name in TREES:
    rc.register("few_" + _name, TREES[_name], SEEDS[_name])

REUSED = ("hub", "t16")                # rhs_cases: a row of 66 sources (69 as written) under an order-136 root; orders <= 16 under 17 .. 32
WIDE = "w72"                           # sweep_cases: wide fronts, on the block kernels from a batch of 16 on
CASES = tuple(TREES) + REUSED + (WIDE,)


def _rc_name(name):
    return "few_" + name if name in TREES else name


def case_matrix(name, symmetric=False):
    """(m, n, Ap, Ai, Ax) of case `name` with the values of matrix 0 of its batches."""
    if name == WIDE:
        return sc.case_matrix(name, symmetric=symmetric)
    return rc.case_matrix(_rc_name(name), symmetric)


def case_values(name, batch, symmetric=False):
    """float64 [batch, nnz]: every matrix of the batch with values of its own (read-only)."""
    if name == WIDE:
        return sc.case_values(name, batch, symmetric=symmetric)
    return rc.case_values(_rc_name(name), batch, symmetric)


def handle(hip, name, kind, batch):
    """A handle of case `name` (no device needed before the first numeric call): the trees in the natural order, w72 in
    the library's own, as in the tests it comes from."""
    if name == WIDE:
        m, n, Ap, Ai, _ = case_matrix(name, kind == "chol")
        return hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU, batch=batch)
    return rc.handle(hip, _rc_name(name), kind, batch)


def promote_pair(symmetric=False):
    """-> (Ax16, Ax17, cols): the values of promote17 (matrix 0) and those of promote16 cut out of them -- promote17
    without the columns and rows of its extra leaf -- so that every entry the two matrices share is the same number;
    cols: the columns of promote16 as columns of promote17."""
    m17, n17, Ap17, Ai17, Ax17 = case_matrix("promote17", symmetric)
    m16, n16, Ap16, Ai16, _ = case_matrix("promote16", symmetric)
    extra = n17 - n16
    assert extra == 3
    root0 = n17 - 130 - extra                                              # the extra leaf sits right in front of the root
    cols = np.concatenate([np.arange(root0), np.arange(root0 + extra, n17)])
    A = sp.csc_matrix((Ax17, Ai17, Ap17), shape=(n17, n17))[cols][:, cols].tocsc()
    A.sort_indices()
    assert np.array_equal(A.indptr, Ap16) and np.array_equal(A.indices, Ai16), "promote16 is not promote17 without its extra leaf"
    return A.data.copy(), np.array(Ax17), cols


# ----------------------------------------------------------------------- dispatch --

Launch = collections.namedtuple("Launch", "level kernel fronts promoted merged")
Dispatch = collections.namedtuple("Dispatch", "P FR launches kernel_of forest")


def uses_forest(FR, nrhs, trans):
    """api.cpp, select_sweep_schedule: the forest's own sweeps serve one plain right-hand side only."""
    return nrhs == 1 and not trans and bool(FR.forest.any())


def dispatch(hip, F, nrhs, trans=False):
    """What sweeps every front of the handle F with `nrhs` < 16 right-hand sides.  launches: in the order of a forward
    sweep -- kernel 'sub', 'il', 'wave1', 'wave8', 'blk' or 'big'; promoted: a wave group inside a block launch; merged: a
    small group inside a wave launch.  kernel_of: per supernode."""
    assert 1 <= nrhs <= FEW_RHS_MAX
    P = rc.plan(hip, F)
    FR = pc.fronts(hip, F)
    ns = len(P.w)
    forest = uses_forest(FR, nrhs, trans)
    if forest:
        # symbolic.cpp, step10b_solve_schedule: the factor schedule's levels, the forest as one group in front
        # (level 0; above it level 1 + the height above the forest)
        tl = np.zeros(ns, dtype=np.int64)
        for s in range(ns):
            if P.parent[s] >= 0 and not FR.forest[s]:
                tl[P.parent[s]] = max(tl[P.parent[s]], tl[s] + 1)
        tl = np.where(FR.forest, 0, tl + 1)
        key = lambda s: (tl[s], rc.SK_ORDER[P.kind[s]])                    # noqa: E731
        level = tl
    else:
        key = lambda s: (P.level[s], rc.SK_ORDER[P.kind[s]], not P.r[s] <= 16)          # noqa: E731
        level = P.level
    sched = sorted(range(ns), key=key)
    groups = []                                                            # [level, kind, fronts]
    for s in sched:
        kind = "sub" if forest and FR.forest[s] else P.kind[s]
        if groups and groups[-1][0] == level[s] and groups[-1][1] == kind:
            groups[-1][2].append(s)
        else:
            groups.append([int(level[s]), kind, [s]])
    # sweep_groups: small + wave of one level -> one wave launch
    merged = []
    for lv, kind, fronts in groups:
        if merged and merged[-1][0] == lv and merged[-1][1] == "small" and kind == "wave":
            merged[-1][1] = "wave"
            merged[-1][2] += fronts
            merged[-1][3] = True
        else:
            merged.append([lv, kind, list(fronts), False, False])
    # absorb_small_group: a lone matrix, a wave group of at most 16 fronts right in front of the level's block group
    out = []
    for lv, kind, fronts, mg, _ in merged:
        if F.batch == 1 and out and out[-1][0] == lv and out[-1][1] == "wave" and kind == "block" and len(out[-1][2]) <= PROMOTE_MAX:
            out[-1][1] = "block"
            out[-1][2] += fronts
            out[-1][4] = True
        else:
            out.append([lv, kind, fronts, mg, False])
    wave = "wave1" if nrhs == 1 else "wave%d" % KT
    name = {"sub": "sub", "il": "il", "small": wave, "wave": wave, "block": "blk", "big": "big"}
    launches = [Launch(lv, name[kind], fronts, pr, mg) for lv, kind, fronts, mg, pr in out]
    kernel_of = [None] * ns
    for L in launches:
        for s in L.fronts:
            kernel_of[s] = L.kernel
    assert None not in kernel_of
    return Dispatch(P, FR, launches, kernel_of, forest)


# -------------------------------------------------------------------------- lists --

# per front.  runs: the number of sources of every row that has any (rows ascending); layout: (chunk position, length,
# long) of every run as emit_runs places it; chunks: 64-entry chunks of the list; padded: runs moved to the next chunk
# because they would have straddled a boundary; long_at_63: long runs (more than 64 sources: two entries, the sources
# themselves in a list of their own) moved because the second entry would have; entries: the list up to its last run
Lists = collections.namedtuple("Lists", "runs layout chunks padded long_at_63 entries")


def lists(P, FR):
    """The forward assembly list of every front: row t of front s gets its own entry of X (t < w) and one source from
    every child whose rows below its pivots hold that row."""
    out = []
    for s in range(len(P.w)):
        cnt = np.zeros(int(P.r[s]), dtype=np.int64)
        cnt[:P.w[s]] = 1
        kids = np.zeros(int(P.r[s]), dtype=np.int64)
        for c in P.children[s]:
            pos = np.searchsorted(FR.rows[s], FR.rows[c][P.w[c]:])
            assert np.array_equal(FR.rows[s][pos], FR.rows[c][P.w[c]:])
            kids[pos] += 1
        assert int(kids.max(initial=0)) == P.rounds[s], "the longest run of the children's additions is not rhs_cases' round count"
        cnt += kids
        runs = [int(x) for x in cnt if x]
        pos, layout, padded, long63 = 0, [], 0, 0
        for ln in runs:
            at = pos % CHUNK
            if ln > CHUNK:
                if at + 2 > CHUNK:
                    pos += CHUNK - at
                    long63 += 1
                layout.append((pos % CHUNK, ln, True))
                pos += 2
            else:
                if at + ln > CHUNK:
                    pos += CHUNK - at
                    padded += 1
                layout.append((pos % CHUNK, ln, False))
                pos += ln
        out.append(Lists(runs, layout, -(-pos // CHUNK), padded, long63, pos))
    return out


# ---------------------------------------------------------------------- residuals --

def products(n, Gp, Gi, Gx, X, trans=False):
    """(T x, |T||x|) in np.longdouble, [n, k] each, for the CSC matrix G (T = G' for trans) and X [n, k]: one
    np.longdouble term per entry and column, added up row by row.  What sweep_cases.substitution_error_ratio forms from a
    dense T, without the n^2 zeros (the trees here have up to 1200 columns and batches of 20 matrices to check)."""
    nz = int(Gp[n])
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Gp[:n + 1]))
    rows = np.asarray(Gi[:nz], dtype=np.int64)
    vals = np.asarray(Gx[:nz], dtype=np.longdouble)
    out, src = (cols, rows) if trans else (rows, cols)
    order = np.argsort(out, kind="stable")
    out, src, vals = out[order], src[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], out[1:] != out[:-1]]))
    assert np.array_equal(out[first], np.arange(n)), "a row of T without an entry"
    X = np.asarray(X, dtype=np.longdouble).reshape(n, -1)
    terms = vals[:, None] * X[src]
    return np.add.reduceat(terms, first, axis=0), np.add.reduceat(np.abs(terms), first, axis=0)


def norm1(n, Gp, Gi, Gx, trans=False):
    """The largest absolute column sum of T (G, or G' for trans), as np.abs(T).sum(axis=0).max() of the dense form."""
    G = sp.csc_matrix((np.abs(np.asarray(Gx[:Gp[n]], dtype=np.float64)), Gi[:Gp[n]], Gp[:n + 1]), shape=(n, n))
    return float(G.sum(axis=1 if trans else 0).max())


def error_ratio(n, G, X, B, trans=False):
    """(max_i |b - T x|_i / (u (|T||x|)_i) per column, max_i |b - T x|_i per column, max_i (|T||x|)_i per column); a
    row with (|T||x|)_i = 0 must have |b - T x|_i = 0 (ratio 0, anything else inf)."""
    TX, W = products(n, *G, X, trans)
    E = np.abs(np.asarray(B, dtype=np.longdouble).reshape(n, -1) - TX)
    u = np.longdouble(2.0) ** -53
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(W > 0, E / (u * W), np.where(E == 0, 0.0, np.inf))
    return ratio.max(axis=0).astype(np.float64), E.max(axis=0).astype(np.float64), W.max(axis=0).astype(np.float64)


def describe(D):
    """One line per launch and (r, w): for the messages of failed assertions."""
    out = []
    for L in D.launches:
        cnt = collections.Counter((int(D.P.r[s]), int(D.P.w[s])) for s in L.fronts)
        out.append("level %d %-5s%s%s %s" % (L.level, L.kernel, " promoted" if L.promoted else "", " merged" if L.merged else "",
                                            " ".join("(%d,%d)x%d" % (*k, cnt[k]) for k in sorted(cnt))))
    return "\n".join(out)
