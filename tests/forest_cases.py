"""Matrices whose bottom forest (csrc/forest.hip; chosen by build_forest / fill_forest in csrc/symbolic.cpp) has a
prescribed shape, and a restatement of what decides that shape, for tests/test_forest_cases_cpu.py and
tests/test_gpu_forest_edges.py.

The matrices are the assembly trees of tests/rhs_cases.py (same builder, same values: off-diagonal -U(0.1, 1), diagonal =
the column's absolute sum + 1, the natural order handed to the library), registered there under names of their own, and
block-diagonal matrices of several such trees ('islands'), every island with values from a seed of its own.

What the forest does with a front (forest.hip): a TASK (one workgroup) holds whole subtrees -- at most 64 fronts, 5 000
doubles of contribution blocks, height 4 -- and works them local level by local level.  The block of a front whose parent
is in the task stays in the task's LDS ARENA, at an offset that accumulates nb (nb + 1) doubles per such front in task
order (nb = r - w), and its part of the right-hand side in a VECTOR ARENA that accumulates nb per front; with more than
256 subtree roots a task holds several roots, one behind the other in both arenas.  A front of 6 pivots or more on a
local level of at most two fronts is SHARED by four waves in column slices of 8: ceil(r / 8) slices, of which the first
ceil(w / 8) own pivots; the last slice carries the right-hand side.  `shape()` restates all of it from the handle, so
that a change of the limits or of the amalgamation's prices makes the tests' assertions fail instead of leaving a path
silently untested.

The relaxed amalgamation (symbolic.cpp, step 5b) lets a front absorb its LAST child, one per pass, four passes, and the
library's own postorder puts the child with the tallest column subtree last.  So a node all of whose children are
single-column leaves ends with 4 more pivots and rows than written down and 4 leaves fewer, and where subtrees are to
survive the last child is either too expensive to absorb (the chains: w_child + r_parent > 32 with more than a quarter
of explicit zeros) or a wide leaf put there for that purpose (`_guard`).
"""
import collections
import ctypes as C

import numpy as np
import scipy.sparse as sp

import pivot_cases as pc
import rhs_cases as rc
from rhs_cases import _leaves, _node

# symbolic.cpp: ForestLimits, and forest.hip: the slice width of a shared front
FRONTS_MAX = 64
ARENA_MAX = 5000
BINS = 256
HEIGHT_MAX = 4
COOP_W = 6
COOP_LEVEL = 2
SLICE = 8
SUB_RMAX = 32                  # cs3_internal.hpp: the largest order of a forest front
SUB_NW = 8                     # forest.hip: fronts of a full local level in flight at once (one per wave)


def slices(x):
    return -(-int(x) // SLICE)


# ------------------------------------------------------------------ construction --

def _guard(w=10):
    """A wide leaf that is the tallest child of its parent (w columns are a chain of w in the column tree) and too
    expensive to absorb: with it the amalgamation leaves the parent and its other children as written."""
    return _node(w, (1, 0))


def _one():
    return _node(4, None, _leaves(9, 1, 1, 1))


def _oneb():
    return _node(4, None, _leaves(10, 1, 1, 1))


def _two():
    return _node(8, None, [_node(3, (2, 0), _leaves(9, 1, 1, 1))] + _leaves(6, 1, 1, 1))


def _three():
    return _node(20, None, [_node(8, (4, 0), _leaves(10, 1, 2, 1)), _node(9, (2, 0), _leaves(10, 1, 1, 1))])


def _pair33():
    return _node(24, None, [_node(16, (2, 0), _leaves(10, 1, 2, 1)), _node(16, (3, 0), _leaves(10, 1, 1, 1))])


def _pair44():
    return _node(24, None, [_node(24, (2, 0), _leaves(10, 1, 2, 1)), _node(24, (3, 0), _leaves(10, 1, 1, 1))])


def _w89():
    return _node(26, None, [_node(4, (3, 0), _leaves(6, 1, 1, 1)), _node(5, (2, 0), _leaves(6, 1, 1, 1)), _guard()])


def _full64():
    return _node(10, None, _leaves(67, 1, 1, 1))


def _over64():
    return _node(10, None, _leaves(68, 1, 1, 1))


def _chain(top):
    """A chain of wide fronts, none of which the amalgamation merges (w_child + r_parent > 32 and too many zeros): one
    shared front per local level, from a leaf of one slice up."""
    c = _node(6, (2, 0))                                                   # (8, 6)
    for w, k in ((24, 6), (25, 4), (17, 6), (16, 4))[:top]:                # (30, 24) (29, 25) (23, 17) (20, 16)
        c = _node(w, (k, 0), [c])
    return _node(26, None, [c])


def _chain6():
    return _chain(4)


def _tri():
    return _chain(1)


def _ea():
    """Child blocks of order 15 and 16, under a one-wave front (5 pivots) and under a shared one; theirs of order 17 and
    10 under the shared root."""
    return _node(28, None, [_node(1, (17, 0), [_node(1, (15, 0)), _node(1, (16, 1))] + _leaves(4, 1, 1, 1)),
                            _node(12, (10, 0), [_node(1, (15, 5)), _node(1, (16, 5))] + _leaves(4, 1, 1, 1))])


def _big():
    return _node(1, (31, 0), [_node(1, (31, 0)), _guard()])                # a block of order 31 into a front of one pivot


def _arena4904():
    return _node(32, None, [_big(), _big(), _node(1, (30, 0)), _guard(12)])


def _arena5014():
    return _node(32, None, [_big(), _big(), _node(1, (30, 0)), _node(1, (10, 0)), _guard(12)])


def _fan(k):
    return lambda: _node(4, None, _leaves(k + 4, 1, 1, 1))


TREES = {}
SEEDS = {}


def _register(name, tree, seed):
    TREES[name] = tree
    SEEDS[name] = seed
    rc.register("forest_" + name, tree, seed)


# islands: name -> [(tree name, copies)]; island i gets the values of seed SEEDS[name] + i
ISLANDS = {}

Matrix = collections.namedtuple("Matrix", "m n Ap Ai Ax starts")
_MATRICES = {}


def case_matrix(name, symmetric=False, other=False):
    """-> Matrix of case `name` (built once); starts: the first column of every island and n (one island for a tree).
    other: a second set of values on the same pattern."""
    key = (name, symmetric, other)
    if key in _MATRICES:
        return _MATRICES[key]
    shift = 500000 if other else 0
    if name in TREES:
        m, n, Ap, Ai, Ax = rc.tree_matrix("forest_" + name, SEEDS[name] + shift, symmetric)
        M = Matrix(m, n, Ap, Ai, Ax, np.array([0, n]))
    else:
        blocks, i = [], 0
        for tree, copies in ISLANDS[name]:
            for _ in range(copies):
                _, nb, Ap, Ai, Ax = rc.tree_matrix("forest_" + tree, SEEDS[name] + shift + i, symmetric)
                blocks.append(sp.csc_matrix((Ax, Ai, Ap), shape=(nb, nb)))
                i += 1
        A = sp.block_diag(blocks, format="csc")
        A.sort_indices()
        n = A.shape[0]
        starts = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])])
        M = Matrix(n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), starts)
    M.Ax.setflags(write=False)
    _MATRICES[key] = M
    return M


def handle(hip, name, kind):
    """A handle of case `name` at batch 1 in the natural order (no device needed before the first numeric call)."""
    M = case_matrix(name, symmetric=kind == "chol")
    return hip.Factorization(M.m, M.n, M.Ap, M.Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU,
                             q=np.arange(M.n, dtype=np.int32), batch=1)


# -------------------------------------------------------------------------- shape --

# per forest front, in task order.  s: the supernode; cls: (slices of its order, slices that own pivots); in_arena: its
# block stays in the task's LDS; arena / varena: where (arena: -1 when the block goes to the pool or there is none);
# child_nb: the orders of its children's blocks; span: the slices of this front that each child's block touches
Front = collections.namedtuple("Front", "s task level shared r w cls in_arena arena varena children child_nb span")
# per task.  levels: per local level (fronts, of them shared)
Task = collections.namedtuple("Task", "fronts roots arena varena levels members")
Shape = collections.namedtuple("Shape", "FR fronts tasks by_sn")


def shape(hip, F):
    """The forest of the handle F as the kernels see it (no device needed)."""
    FR = pc.fronts(hip, F)
    ns = len(FR.w)
    lib = hip.lib()
    i32p = C.POINTER(C.c_int32)
    sn = np.full(ns, -1, dtype=np.int32)
    nf = int(lib.cs3_debug_forest(F._h, sn.ctypes.data_as(i32p), None, None, None))
    order = [int(s) for s in sn[:nf]]                                      # the fronts in task order
    assert sorted(order) == [int(s) for s in np.flatnonzero(FR.forest)]
    children = [[] for _ in range(ns)]
    for s in range(ns):
        if FR.parent[s] >= 0:
            children[FR.parent[s]].append(s)
    fronts, tasks, by_sn = [], [], {}
    arena = varena = 0
    task = -1
    for s in order:
        if FR.task[s] != task:
            assert FR.task[s] == task + 1, "tasks are numbered in the order of their fronts"
            task, arena, varena = task + 1, 0, 0
            tasks.append(dict(fronts=0, roots=0, arena=0, varena=0, levels=[], members=[]))
        T = tasks[-1]
        r, w = int(FR.r[s]), int(FR.w[s])
        nb = r - w
        p = int(FR.parent[s])
        inside = p >= 0 and bool(FR.forest[p])
        assert not inside or FR.task[p] == task
        assert all(FR.forest[c] and FR.task[c] == task for c in children[s]), "a forest front has a child outside its task"
        span = []
        for c in children[s]:
            below = FR.rows[c][FR.w[c]:]
            pos = np.searchsorted(FR.rows[s], below)
            assert np.array_equal(FR.rows[s][pos], below)
            span.append(len(np.unique(pos // SLICE)))
        f = Front(s, task, int(FR.level[s]), bool(FR.shared[s]), r, w, (slices(r), slices(w)), inside,
                  arena if inside else -1, varena, list(children[s]), [int(FR.r[c] - FR.w[c]) for c in children[s]], span)
        if inside:
            arena += nb * (nb + 1)
        varena += nb
        by_sn[s] = len(fronts)
        fronts.append(f)
        T["fronts"] += 1
        T["roots"] += not inside
        T["arena"], T["varena"] = arena, varena
        T["members"].append(len(fronts) - 1)
        while len(T["levels"]) <= f.level:
            T["levels"].append([0, 0])
        assert f.level == len(T["levels"]) - 1, "a task's fronts come local level by local level"
        T["levels"][f.level][0] += 1
        T["levels"][f.level][1] += f.shared
    tasks = [Task(T["fronts"], T["roots"], T["arena"], T["varena"], [tuple(l) for l in T["levels"]], T["members"]) for T in tasks]
    for T in tasks:
        assert T.fronts <= FRONTS_MAX and T.arena <= ARENA_MAX and len(T.levels) <= HEIGHT_MAX + 1
        assert all(sh == 0 or cnt <= COOP_LEVEL for cnt, sh in T.levels)
    return Shape(FR, fronts, tasks, by_sn)


def describe(S):
    """The forest and what lies above it, one line per task and per kind of front: for the messages of failed assertions."""
    out = []
    for t, T in enumerate(S.tasks):
        out.append("task %d: %d fronts, %d roots, arena %d, vector arena %d, levels %s" % (t, T.fronts, T.roots, T.arena, T.varena, T.levels))
        if t >= 6:
            out.append("... %d tasks in all" % len(S.tasks))
            break
    cnt = collections.Counter((f.level, f.shared, f.r, f.w, f.in_arena, tuple(sorted(f.child_nb))) for f in S.fronts)
    for k in sorted(cnt):
        out.append("level %d %s r=%2d w=%2d %s children %s  x%d" % (k[0], "shared" if k[1] else "wave  ", k[2], k[3],
                                                                  "arena" if k[4] else "pool ", list(k[5]), cnt[k]))
    FR = S.FR
    above = collections.Counter((int(FR.r[s]), int(FR.w[s]), FR.cls[s]) for s in range(len(FR.w)) if not FR.forest[s])
    for k in sorted(above):
        out.append("above the forest r=%3d w=%3d %s  x%d" % (*k, above[k]))
    return "\n".join(out)


for _name, _tree, _seed in (("one", _one, 101000), ("oneb", _oneb, 101500), ("two", _two, 102000), ("three", _three, 103000),
                            ("pair33", _pair33, 104000), ("pair44", _pair44, 104500),
                            ("full64", _full64, 105000), ("over64", _over64, 106000),
                            ("chain6", _chain6, 107000), ("tri", _tri, 107500), ("w89", _w89, 108000), ("ea", _ea, 109000),
                            ("arena4904", _arena4904, 110000), ("arena5014", _arena5014, 111000),
                            ("fan8", _fan(8), 112000), ("fan9", _fan(9), 112100), ("fan16", _fan(16), 112200),
                            ("fan17", _fan(17), 112300)):
    _register(_name, _tree, _seed)

# full local levels of exactly 8, 9, 16 and 17 fronts, a task each
ISLANDS["fans"] = [("fan8", 1), ("fan9", 1), ("fan16", 1), ("fan17", 1)]
SEEDS["fans"] = 120000
# 276 roots for 256 tasks: the 20 smallest subtrees (3 fronts on 3 local levels each) go behind the roots of other tasks
ISLANDS["isl"] = [("oneb", 118), ("tri", 10), ("two", 20), ("oneb", 118), ("tri", 10)]
SEEDS["isl"] = 130000

# the cases of the tests: what each is there for is asserted in tests/test_forest_cases_cpu.py
CASES = ("one", "two", "three", "pair33", "pair44", "w89", "chain6", "ea", "full64", "over64", "arena4904", "arena5014", "fans", "isl")
