"""Matrices with a prescribed assembly tree for the sweeps of 16 or more right-hand sides, and a restatement of what
decides the kernel instance that sweeps a front there, for tests/test_rhs_cases_cpu.py and
tests/test_gpu_many_rhs_edges.py.

The matrix: every node s of a tree has w_s columns of its own, a dense clique, coupled densely to a chosen subset
anc(s) of its parent's structure (the parent's own columns and anc(parent)); the subset always holds the parent's first
column.  Children are numbered before their parents and the library gets the natural order (q = 0 .. n - 1), so no
fill-reducing ordering reshuffles the tree (the analysis still postorders it: ordering()["q"] is what the factors are
in): node s becomes a front of w_s pivots and w_s + |anc(s)| rows, up to what the relaxed amalgamation merges (a front
absorbs its LAST child, one per pass, four passes: the trees below carry the children that this costs them).  Values as in
sweep_cases.blocks_on_separator: off-diagonal -U(0.1, 1), diagonal = the column's absolute sum + 1, `symmetric` for
Cholesky, and a pattern that does not depend on the seed, so matrices of different seeds form a batch.

With 16 or more right-hand sides a front is swept (symbolic.cpp: solve_kind, the solve schedule; kernels.hip:
launch_solve_group) by
  k_fwd_il / k_bwd_il              order <= 16 in a batch of 128 or more ('il'),
  k_fwd_rhs / k_bwd_rhs<RMAX>      order <= 32 ('small'): ONE instance per (level, kind) group, by the group's largest
                                   order -- RMAX 16, 24 or 32,
  the GEMM sweeps                  beyond ('wave', 'block', 'big'): k_gemm_gather, k_gemm_fwd, k_gemm_bwd_init, k_gemm_bwd.
What the children add to a front's vector is laid out in SLOT ROUNDS: round j holds the j-th source of every row.
k_fwd_rhs keeps 4 rounds of indices in registers and k_gemm_gather 64; beyond that they reload.  `plan()` restates the
levels, the kinds, the groups with their instance and the round count of every front, so that a change of dispatch or of
the amalgamation's prices makes the tests' assertions fail instead of leaving an instance silently untested.
"""
import collections
import ctypes as C

import numpy as np

import pivot_cases as pc
import sweep_cases as sc

RHS_LANES_MIN = 16             # kernels.hip: from this many right-hand sides on the kernels above sweep
SLOT_ROUNDS_RHS = 4            # kernels.hip, k_fwd_rhs: SR
SLOT_ROUNDS_GATHER = 64        # kernels.hip, k_gemm_gather: rounds per pass
IL_MIN_BATCH = 128             # symbolic.cpp: il_min_batch
BATCHES = (1, 4, 20, 50, 130)


# ------------------------------------------------------------------ construction --

def _node(w, anc=None, children=()):
    """A node of the tree: w own columns; anc = (k, skip): coupled to k entries of the parent's structure -- its first
    and the k - 1 from position 1 + skip on (None: the root)."""
    return (w, anc, tuple(children))


def _leaves(count, w, k, skips=3):
    return [_node(w, (k, c % skips)) for c in range(count)]


def _t16():
    mids = [_node(2, (5, 0), _leaves(14, 1, 2)), _node(3, (6, 1), _leaves(9, 2, 2)), _node(2, (4, 2), _leaves(6, 1, 1, 1))]
    return _node(20, None, mids)


def _t24():
    mids = [_node(6, (10, 0), _leaves(14, 2, 2)), _node(5, (8, 1), _leaves(9, 2, 3)), _node(7, (12, 2), _leaves(13, 1, 2))]
    return _node(22, None, mids)


def _t32():
    mids = [_node(1, (28, 0), [_node(8, (1, 0))]), _node(8, (16, 0), _leaves(18, 2, 3)), _node(6, (7, 1), _leaves(9, 1, 2)),
            _node(12, (1, 0), _leaves(8, 2, 2)), _node(5, (12, 3), _leaves(8, 1, 1, 1))]
    return _node(30, None, mids)


def _hub():
    a = _node(20, (24, 0), _leaves(12, 2, 2) + _leaves(56, 1, 1, 1))
    b = _node(40, (50, 1), _leaves(13, 2, 3) + _leaves(56, 1, 1, 1))
    m = _node(6, (14, 2), _leaves(12, 2, 2))
    return _node(136, None, [a, b, m] + _leaves(12, 2, 2))


TREES = {"t16": _t16, "t24": _t24, "t32": _t32, "hub": _hub}
SEEDS = {"t16": 16000, "t24": 24000, "t32": 32000, "hub": 64000}

_REGISTERED = {}               # trees of other case modules (tests/forest_cases.py): not among the cases of this one


def register(name, tree, seed):
    """Makes `tree` (a function -> _node) known to _pattern / tree_matrix / case_matrix / handle under `name`."""
    assert name not in TREES and _REGISTERED.get(name, tree) is tree
    _REGISTERED[name] = tree
    SEEDS[name] = seed


Pattern = collections.namedtuple("Pattern", "n Ap Ai ei ej order")
_PATTERNS = {}


def _pattern(name):
    if name in _PATTERNS:
        return _PATTERNS[name]
    # postorder: the children of a node, each with its whole subtree, then the node
    flat = []                                                              # (w, anc, parent's index in flat or -1)

    def walk(node):
        w, anc, children = node
        mine = []
        for c in children:
            mine.append(walk(c))
        flat.append([w, anc, -1])
        for c in mine:
            flat[c][2] = len(flat) - 1
        return len(flat) - 1

    walk((TREES[name] if name in TREES else _REGISTERED[name])())
    c0 = np.concatenate([[0], np.cumsum([f[0] for f in flat])]).astype(np.int64)
    n = int(c0[-1])
    struct = [None] * len(flat)
    for s in range(len(flat) - 1, -1, -1):                                 # parents first
        w, anc, p = flat[s]
        own = np.arange(c0[s], c0[s] + w)
        if p < 0:
            up = np.zeros(0, dtype=np.int64)
        else:
            k, skip = anc
            cand = struct[p]
            up = np.unique(np.concatenate([cand[:1], cand[1 + skip:skip + k]]))
            assert len(up) == k, "node %d: its parent's structure has no %d entries from %d on" % (s, k - 1, 1 + skip)
        struct[s] = np.concatenate([own, up])
    ei, ej = [], []
    for s, (w, anc, p) in enumerate(flat):
        own, up = struct[s][:w], struct[s][w:]
        i, j = np.triu_indices(w, 1)
        ei.append(own[i]); ej.append(own[j])
        i, j = np.meshgrid(own, up, indexing="ij")
        ei.append(i.ravel()); ej.append(j.ravel())
    ei, ej = np.concatenate(ei).astype(np.int64), np.concatenate(ej).astype(np.int64)
    assert (ei < ej).all() and len(np.unique(ei * n + ej)) == len(ei)
    rows = np.concatenate([ej, ei, np.arange(n)])                          # lower triangle, upper triangle, diagonal
    cols = np.concatenate([ei, ej, np.arange(n)])
    order = np.lexsort((rows, cols))
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    _PATTERNS[name] = Pattern(n, Ap.astype(np.int32), rows[order].astype(np.int32), ei, ej, order)
    return _PATTERNS[name]


def tree_matrix(name, seed, symmetric=False):
    """-> (m, n, Ap, Ai, Ax) of case `name` with the values of `seed`."""
    P = _pattern(name)
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.1, 1.0, size=len(P.ei))                             # entry (ej, ei), column ei
    up = lo if symmetric else rng.uniform(0.1, 1.0, size=len(P.ei))        # entry (ei, ej), column ej
    diag = 1.0 + np.bincount(P.ei, weights=lo, minlength=P.n) + np.bincount(P.ej, weights=up, minlength=P.n)
    Ax = np.concatenate([-lo, -up, diag])[P.order]
    return P.n, P.n, P.Ap, P.Ai, Ax


def case_matrix(name, symmetric=False):
    """The pattern of case `name` with the values of matrix 0 of its batches."""
    return tree_matrix(name, SEEDS[name], symmetric)


_VALUES = {}


def case_values(name, batch, symmetric=False, other=False):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own (built once; read-only).
    other: a second set of values on the same pattern (the tests of state that outlives a factorisation)."""
    key = (name, batch, symmetric, other)
    if key not in _VALUES:
        AX = np.stack([tree_matrix(name, SEEDS[name] + (500 if other else 0) + i, symmetric)[4] for i in range(batch)])
        AX.setflags(write=False)
        _VALUES[key] = AX
    return _VALUES[key]


def handle(hip, name, kind, batch):
    """A handle of case `name` in the natural order (no device needed before the first numeric call)."""
    m, n, Ap, Ai, _ = case_matrix(name, symmetric=kind == "chol")
    return hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU,
                             q=np.arange(n, dtype=np.int32), batch=batch)


# ----------------------------------------------------------------------- dispatch --

SK_ORDER = {"small": 0, "wave": 1, "block": 2, "big": 3, "il": 4}         # cs3_internal.hpp: the solve schedule's second key

Group = collections.namedtuple("Group", "level kind fronts max_r rmax")
Plan = collections.namedtuple("Plan", "r w parent kind level rounds children schedule groups")


def rmax_of(max_r):
    """kernels.hip, launch_solve_group: the register-size instance of k_fwd_rhs / k_bwd_rhs for a group of 'small' fronts."""
    assert max_r <= 32
    return 16 if max_r <= 16 else 24 if max_r <= 24 else 32


def plan(hip, F):
    """What sweeps every front of the handle F with 16 or more right-hand sides.  level: height above the leaves
    (symbolic.cpp: sn_level); kind: sweep_cases.solve_kinds; rounds: the largest number of children whose rows below their
    pivots contain one row of the front (symbolic.cpp: sl_rounds); schedule: the fronts by (level, kind, order <= 16
    first), stable; groups: the runs of one (level, kind) in it, with the largest order and, for 'small', RMAX."""
    K = sc.solve_kinds(hip, F)
    FR = pc.fronts(hip, F)
    ns = len(K.w)
    sched = np.zeros(ns, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    assert hip.lib().cs3_debug_schedule(F._h, sched.ctypes.data_as(i32p), None, None) == 0
    parent = np.asarray(K.parent)
    level = np.zeros(ns, dtype=np.int64)
    children = [[] for _ in range(ns)]
    for s in range(ns):                                                    # children precede their parents
        if parent[s] >= 0:
            assert parent[s] > s
            level[parent[s]] = max(level[parent[s]], level[s] + 1)
            children[parent[s]].append(s)
    # the library's own levels; and its factor schedule runs level by level wherever no bottom forest goes first
    assert np.array_equal(F.supernodes()[2], level), "the levels of the solve schedule are not the heights above the leaves"
    assert FR.forest.any() or (np.diff(level[sched]) >= 0).all(), "the factor schedule does not run level by level"
    rounds = np.zeros(ns, dtype=np.int64)
    for s in range(ns):
        below = [FR.rows[c][K.w[c]:] for c in children[s]]
        if below and sum(len(b) for b in below):
            allrows = np.concatenate(below)
            assert np.isin(allrows, FR.rows[s]).all()
            rounds[s] = np.unique(allrows, return_counts=True)[1].max()
    schedule = sorted(range(ns), key=lambda s: (level[s], SK_ORDER[K.kind[s]], not K.r[s] <= 16))
    groups = []
    for s in schedule:
        if groups and (groups[-1].level, groups[-1].kind) == (int(level[s]), K.kind[s]):
            groups[-1].fronts.append(s)
        else:
            groups.append(Group(int(level[s]), K.kind[s], [s], 0, 0))
    for i, g in enumerate(groups):
        max_r = int(max(K.r[s] for s in g.fronts))
        groups[i] = g._replace(max_r=max_r, rmax=rmax_of(max_r) if g.kind == "small" else 0)
    return Plan(np.asarray(K.r), np.asarray(K.w), parent, K.kind, level, rounds, children, schedule, groups)


def group_of(P, s):
    return next(g for g in P.groups if s in g.fronts)


def describe(P):
    """One line per (level, kind, r, w, rounds): for the messages of failed assertions."""
    cnt = collections.Counter((int(P.level[s]), P.kind[s], int(P.r[s]), int(P.w[s]), int(P.rounds[s])) for s in range(len(P.w)))
    return "\n".join("level %d %-5s r=%3d w=%3d rounds=%3d  x%d" % (*k, cnt[k]) for k in sorted(cnt))


# ---------------------------------------------------------------- right-hand sides --

def right_hand_sides(batch, n, nrhs, seed):
    """[batch, n, nrhs] standard normal; of the batch * nrhs columns (matrix-major) the last is scaled by 2^200, the
    second by 2^-200 (three columns or more) and the third is zero (four or more)."""
    B = np.random.default_rng(seed).standard_normal((batch, n, nrhs))
    cols = B.transpose(0, 2, 1).reshape(batch * nrhs, n)                   # a copy: column c = (matrix c // nrhs, column c % nrhs)
    if len(cols) >= 2:
        cols[-1] *= 2.0 ** 200
    if len(cols) >= 3:
        cols[1] *= 2.0 ** -200
    if len(cols) >= 4:
        cols[2] = 0.0
    return np.ascontiguousarray(cols.reshape(batch, nrhs, n).transpose(0, 2, 1))
