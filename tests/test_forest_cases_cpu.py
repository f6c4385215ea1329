"""The matrices of tests/forest_cases.py against the host analysis and the CPU oracle alone (no GPU): between them the
cases deliver every shape of the bottom forest that tests/test_gpu_forest_edges.py is written for -- shared fronts of
one to four slices whose LAST slice owns pivots, pivots that end at a slice edge, local levels of every mix, child
blocks at and beyond 16, tasks at the limits of ForestLimits and tasks of several roots -- for LU and Cholesky alike;
the oracle keeps the diagonal on them, and the high-precision substitution that the GPU tests use as their reference
agrees with the oracle's sweeps."""
import numpy as np
import pytest

import forest_cases as fc
import pivot_cases as pc
import sweep_cases as sc

KINDS = ("lu", "chol")
LU_TOL = 1e-3

_SHAPES = {}


def _shape(hip, name, kind):
    if (name, kind) not in _SHAPES:
        with fc.handle(hip, name, kind) as F:
            _SHAPES[name, kind] = fc.shape(hip, F)
    return _SHAPES[name, kind]


def _what(S, name, kind):
    return "%s %s\n%s" % (name, kind, fc.describe(S))


def _shared(S, cond=lambda f: True):
    return [f for f in S.fronts if f.shared and cond(f)]


@pytest.mark.parametrize("kind", KINDS)
def test_restated_limits_and_the_sharing_rule(hip, kind):
    """shape() restates who is shared; the library's own count of shared fronts per level is not exported, so the rule
    (6 pivots or more, a local level of at most two fronts) is pinned through the limits it asserts and through the
    classes below."""
    for name in fc.CASES:
        S = _shape(hip, name, kind)
        for f in S.fronts:
            assert f.r <= fc.SUB_RMAX
            assert f.shared == (f.w >= fc.COOP_W and S.tasks[f.task].levels[f.level][0] <= fc.COOP_LEVEL), _what(S, name, kind)
            assert f.cls == (fc.slices(f.r), fc.slices(f.w)) and (f.arena >= 0) == f.in_arena
            assert S.FR.cls[f.s] == ("forest_shared" if f.shared else "forest_wave")
        assert len(S.tasks) <= fc.BINS


@pytest.mark.parametrize("kind", KINDS)
def test_a_one_slice_shared_front(hip, kind):
    """(a)  r <= 8: one slice, which is the last, owns every pivot and carries the right-hand side."""
    S = _shape(hip, "one", kind)
    assert S.FR.n == 13 and [(f.r, f.w) for f in _shared(S)] == [(8, 8)], _what(S, "one", kind)
    S = _shape(hip, "chain6", kind)
    got = _shared(S, lambda f: f.r <= 8 and f.w < f.r and f.in_arena)
    assert [(f.r, f.w) for f in got] == [(8, 6)], _what(S, "chain6", kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_last_slice_owns_pivots(hip, kind):
    """(b)  classes (1,1) (2,2) (3,3) (4,4), with and without contribution columns behind the pivots in the last slice."""
    seen = {}
    for name in fc.CASES:
        S = _shape(hip, name, kind)
        for f in _shared(S):
            seen.setdefault((f.cls, f.w < f.r), set()).add(name)
    for c in (1, 2, 3, 4):
        assert ((c, c), True) in seen and ((c, c), False) in seen, (c, seen)
    S = _shape(hip, "pair33", kind)
    both = [f for f in _shared(S, lambda f: f.cls == (3, 3) and f.w < f.r)]
    assert len(both) == 2 and both[0].task == both[1].task and both[0].level == both[1].level, _what(S, "pair33", kind)
    assert [(f.r, f.w) for f in _shared(S, lambda f: f.w == f.r)] == [(24, 24)]
    # ... and a last slice of four slices with several pivots and contribution columns behind them
    S = _shape(hip, "pair44", kind)
    assert sorted((f.r, f.w) for f in _shared(S)) == [(24, 24), (30, 28), (31, 28)], _what(S, "pair44", kind)
    S = _shape(hip, "three", kind)
    assert sorted((f.r, f.w) for f in _shared(S)) == [(16, 12), (32, 32)], _what(S, "three", kind)
    S = _shape(hip, "two", kind)
    assert [(f.r, f.w) for f in _shared(S)] == [(15, 15)], _what(S, "two", kind)


@pytest.mark.parametrize("kind", KINDS)
def test_pivots_that_end_at_a_slice_edge(hip, kind):
    """(c)"""
    widths = set()
    for name in ("w89", "chain6"):
        S = _shape(hip, name, kind)
        widths |= {f.w for f in _shared(S, lambda f: f.w < f.r)}
    assert {8, 9, 16, 17, 24, 25} <= widths, widths


@pytest.mark.parametrize("kind", KINDS)
def test_local_levels(hip, kind):
    """(d)"""
    levels = {name: [lv for T in _shape(hip, name, kind).tasks for lv in T.levels] for name in fc.CASES}
    assert (2, 1) in levels["ea"], "one shared and one one-wave front on a level"
    assert (1, 1) in levels["three"] and (2, 2) in levels["pair33"] and (2, 2) in levels["w89"]
    assert sorted(levels["fans"]) == [(1, 1)] * 4 + [(8, 0), (9, 0), (16, 0), (17, 0)], levels["fans"]
    assert fc.SUB_NW == 8                                   # (8 | 9 and 16 | 17: one and two full rounds of the waves, and one front more)
    S = _shape(hip, "chain6", kind)
    assert len(S.tasks) == 1 and S.tasks[0].levels == [(1, 1)] * 5, _what(S, "chain6", kind)
    # the counter that the hand-overs are numbered with grows by 64 per round of (up to) two shared fronts and is never
    # reset: the fifth level starts at 256 and counts on from there
    rounds = sum(-(-sh // 2) for _, sh in S.tasks[0].levels)
    assert 64 * (rounds - 1) >= 256 and _shared(S)[-1].w > 8


@pytest.mark.parametrize("kind", KINDS)
def test_extend_add(hip, kind):
    """(e)"""
    S = _shape(hip, "ea", kind)
    what = _what(S, "ea", kind)
    eaters = [f for f in S.fronts if sorted(f.child_nb)[-2:] == [15, 16]]
    assert sorted(f.shared for f in eaters) == [False, True], what
    for f in eaters:
        kids = [S.fronts[S.by_sn[c]] for c in f.children]
        assert all(k.in_arena for k in kids), what
        if f.shared:
            assert all(sp >= 3 for sp, nb in zip(f.span, f.child_nb) if nb >= 15), what
    root = S.fronts[-1]
    assert root.shared and sorted(root.child_nb) == [10, 17] and max(root.span) >= 3, what
    # the largest block there can be: order 31, from a front of order 32 with one pivot into another such front, and
    # from that into a shared root of four slices
    S = _shape(hip, "arena4904", kind)
    what = _what(S, "arena4904", kind)
    big = [f for f in S.fronts if 31 in f.child_nb]
    assert sorted((f.shared, f.r, f.w) for f in big) == [(False, 32, 1), (False, 32, 1), (True, 32, 32)], what
    assert all(S.fronts[S.by_sn[c]].in_arena for f in big for c in f.children), what
    S = _shape(hip, "full64", kind)
    assert len(S.fronts[-1].children) == 63 >= 12, _what(S, "full64", kind)


@pytest.mark.parametrize("kind", KINDS)
def test_limits_from_both_sides(hip, kind):
    """(f)"""
    S = _shape(hip, "full64", kind)
    assert S.FR.n == 77 and [T.fronts for T in S.tasks] == [fc.FRONTS_MAX] and S.FR.forest.all(), _what(S, "full64", kind)
    S = _shape(hip, "over64", kind)
    assert S.FR.n == 78 and len(S.FR.w) == fc.FRONTS_MAX + 1 and not S.FR.forest.any(), _what(S, "over64", kind)
    S = _shape(hip, "arena4904", kind)
    assert [T.arena for T in S.tasks] == [4904] and S.FR.forest.all(), _what(S, "arena4904", kind)
    assert 4900 <= 4904 <= fc.ARENA_MAX
    S = _shape(hip, "arena5014", kind)
    what = _what(S, "arena5014", kind)
    out = np.flatnonzero(~S.FR.forest)
    assert list(out) == [len(S.FR.w) - 1] and S.FR.parent[out[0]] == -1, what
    assert sum(T.arena for T in S.tasks) + 2 * 1 + 30 * 31 + 10 * 11 + 2 * 31 * 32 == 5014 > fc.ARENA_MAX, what
    assert sorted(len(T.levels) for T in S.tasks) == [1, 1, 1, 2, 2], what
    S = _shape(hip, "chain6", kind)
    what = _what(S, "chain6", kind)
    out = np.flatnonzero(~S.FR.forest)
    assert list(out) == [len(S.FR.w) - 1] and S.FR.r[out[0]] <= fc.SUB_RMAX, what      # outside for its height alone
    assert [len(T.levels) for T in S.tasks] == [fc.HEIGHT_MAX + 1], what
    top = S.fronts[-1]
    assert not top.in_arena and S.FR.parent[top.s] == out[0] and top.r > top.w, what     # its block goes to the pool


@pytest.mark.parametrize("kind", KINDS)
def test_several_roots_per_task(hip, kind):
    """(g)"""
    S = _shape(hip, "isl", kind)
    what = _what(S, "isl", kind)
    M = fc.case_matrix("isl", symmetric=kind == "chol")
    roots = sum(T.roots for T in S.tasks)
    assert roots == len(M.starts) - 1 == 276 >= fc.BINS + 1 and len(S.tasks) == fc.BINS and S.FR.forest.all(), what
    assert sorted(set(T.roots for T in S.tasks)) == [1, 2], what
    island = np.searchsorted(M.starts, S.FR.c0, side="right") - 1
    behind = 0
    for T in S.tasks:
        if T.roots < 2:
            continue
        mine = [S.fronts[i] for i in T.members]
        isl = [int(island[f.s]) for f in mine]
        assert len(set(isl)) == 2, what
        # roots join a task largest subtree first: the second root is the one of fewer fronts
        a, b = sorted(set(isl), key=lambda i: -isl.count(i))
        second = [f for f, i in zip(mine, isl) if i == b]
        # its subtree: three local levels, two of its blocks in the arena, the upper one behind blocks of the first root
        assert sorted(f.level for f in second) == [0, 1, 2] and isl.count(a) > 3, what
        if any(f.in_arena and f.arena > 0 and f.varena > 0 and f.level > 0 for f in second):
            behind += 1
        # the two islands are different trees
        assert M.starts[a + 1] - M.starts[a] != M.starts[b + 1] - M.starts[b], what
    assert behind == 20, what
    sizes = set(np.diff(M.starts))
    assert len(sizes) >= 2
    # every island has values of its own
    diag = [M.Ax[M.Ap[c]:M.Ap[c + 1]][:2].tobytes() for c in M.starts[:-1]]
    assert len(set(diag)) == len(diag)


# ---------------------------------------------------------------------- reference --

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", fc.CASES)
def test_the_library_keeps_the_natural_order_up_to_a_postorder(hip, name, kind):
    S = _shape(hip, name, kind)
    M = fc.case_matrix(name, symmetric=kind == "chol")
    assert sorted(S.FR.q) == list(range(M.n))
    island = np.searchsorted(M.starts, S.FR.q, side="right") - 1
    assert (np.diff(island) >= 0).all(), "the islands stay in their order"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", fc.CASES)
def test_oracle_keeps_the_diagonal_and_substitute_agrees_with_its_sweeps(orc, hip, name, kind):
    """(h)  in the order the library factors in."""
    S = _shape(hip, name, kind)
    M = fc.case_matrix(name, symmetric=kind == "chol")
    n, q = M.n, S.FR.q
    if kind == "chol":
        L, U = pc.oracle_chol(orc, n, M.Ap, M.Ai, M.Ax, q), None
    else:
        Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, M.Ap, M.Ai, M.Ax, q, LU_TOL)
        assert np.array_equal(pinv[q], np.arange(n)), "the oracle left the diagonal"
        L, U = (Lp, Li, Lx), (Up, Ui, Ux)
    b = np.random.default_rng(3).standard_normal(n)
    sweeps = [(L, True, False, orc.csc_lsolve_f), (L, True, True, orc.csc_ltsolve_f)]
    if U is not None:
        sweeps += [(U, False, False, orc.csc_usolve_f)]
    for G, lower, trans, fn in sweeps:
        x = sc.substitute(n, *G, b, lower, trans)
        want = b.copy()
        fn(n, *G, want)
        assert np.abs(x - want).max() <= 1e-13 * np.abs(want).max(), (lower, trans)
