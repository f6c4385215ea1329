"""The matrices of tests/few_rhs_cases.py against the host analysis and the CPU oracle alone (no GPU): every case
delivers the fronts, levels, launch groups, assembly-list layouts and kernels that tests/test_gpu_few_rhs_edges.py is
written for, in every batch it runs; the oracle keeps the diagonal on them, the high-precision substitution that the GPU
tests use as their reference agrees with the oracle's four sweeps, and the componentwise bound asserted there holds for
the oracle's own float64 sweeps without being vacuous (a relative error of 1e-9 in one entry of x, or in the smallest
entry of the factor, breaks it)."""
import numpy as np
import pytest

import few_rhs_cases as fc
import pivot_cases as pc
import rhs_cases as rc
import sweep_cases as sc
from helpers import RTOL

KINDS = ("lu", "chol")
LU_TOL = 1e-3
CALLS = [(nrhs, trans) for nrhs in (1, 2, 15) for trans in (False, True)]

_ANALYSED = {}


def _analysed(hip, name, kind, batch):
    """{(nrhs, trans): Dispatch} and the lists of every front, once per (case, kind, batch)."""
    key = (name, kind, batch)
    if key not in _ANALYSED:
        with fc.handle(hip, name, kind, batch) as F:
            D = {(nrhs, trans): fc.dispatch(hip, F, nrhs, trans) for nrhs, trans in CALLS if not (trans and kind == "chol")}
            _ANALYSED[key] = (D, fc.lists(D[2, False].P, D[2, False].FR))
    return _ANALYSED[key]


def _rw(P):
    return {(int(r), int(w)) for r, w in zip(P.r, P.w)}


def _check_kernels(D, batch, promoted, what):
    """The kernel of every front in every call, stated front by front (not through the launch groups): the forest's
    sweeps for its fronts at one plain right-hand side, lane = matrix for order <= 16 in a batch of 128 or more, the block
    kernels for 'block' fronts and for the promoted wave group, one wave per front otherwise."""
    for (nrhs, trans), d in D.items():
        P, FR = d.P, d.FR
        assert d.forest == (nrhs == 1 and not trans and bool(FR.forest.any())), what
        assert "big" not in P.kind or batch > sc.BIG_BATCH_MAX or what.startswith(fc.WIDE), what
        for s in range(len(P.w)):
            if d.forest and FR.forest[s]:
                want = "sub"
            elif P.r[s] <= 16 and batch >= rc.IL_MIN_BATCH:
                want = "il"
            elif P.r[s] <= 128 and P.w[s] <= 64:
                want = "blk" if s in promoted else "wave1" if nrhs == 1 else "wave8"
            else:
                want = "big" if P.kind[s] == "big" else "blk"
            assert d.kernel_of[s] == want, "%s nrhs %d trans %s front %d (%d, %d): %s, not %s\n%s" % (
                what, nrhs, trans, s, P.r[s], P.w[s], d.kernel_of[s], want, fc.describe(d))
        assert sorted(s for L in d.launches if L.promoted for s in L.fronts if s in promoted) == sorted(promoted), what
        assert all(L.kernel == "blk" for L in d.launches if L.promoted), what
        assert bool(promoted) == any(L.promoted for L in d.launches), what


@pytest.mark.parametrize("batch", fc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_wave(hip, kind, batch):
    D, LS = _analysed(hip, "wave", kind, batch)
    d = D[2, False]
    P, FR = d.P, d.FR
    what = "wave %s batch %d\n%s" % (kind, batch, fc.describe(d))
    ns = len(P.w)
    assert not FR.forest.any(), what                                       # one plain right-hand side takes the level schedule too
    _check_kernels(D, batch, (), what)
    assert set(P.kind) <= {"small", "wave", "il"} and (P.r <= 128).all() and (P.w <= 64).all(), what
    # the fronts: the first order past the small ones; 64 against 65 rows (the second row of a lane); w = 64, every lane a
    # pivot row, with two full rows per lane; one row and one pivot less
    for rw in ((sc.SMALL_RMAX + 1, 1), (64, 8), (65, 9), (128, 64), (127, 63)):
        assert rw in _rw(P), what
    # the prefetch steps of 8: w no multiple, and the ancestors r - w one past and one short of a multiple
    assert {(P.r[s] - P.w[s]) % fc.SOLVE_PF for s in range(ns) if P.w[s] % fc.SOLVE_PF and P.kind[s] == "wave"} >= {1, 7}, what
    # ancestors in rows >= 64 behind fewer than 64 pivots: the backward sweep broadcasts from the second row of a lane
    assert any(P.w[s] < 64 < P.r[s] and P.r[s] - P.w[s] > 8 for s in range(ns)), what
    assert (73, 60) in _rw(P), what                                        # ... starting inside a prefetch step (rows 60 .. 72)
    root = ns - 1
    assert P.parent[root] == -1 and P.r[root] == P.w[root] == 64 and (P.parent[:root] >= 0).all(), what
    # four fronts per workgroup: a launch whose count leaves one front for the last workgroup
    waves = [L for L in d.launches if L.kernel == "wave8"]
    assert any(len(L.fronts) > fc.WAVES_PER_WG and len(L.fronts) % fc.WAVES_PER_WG == 1 for L in waves), what
    if batch < rc.IL_MIN_BATCH:                                            # the small group of a level inside its wave launch
        assert any(L.merged and {"small", "wave"} <= {P.kind[s] for s in L.fronts} for L in waves), what
    else:
        assert any(L.kernel == "il" for L in d.launches) and not any(L.merged for L in d.launches), what
    # pivot row 0 with 63, 64, 65, 66 sources in wave fronts: the last two as long runs (one lane adds them up)
    row0 = {LS[s].runs[0]: LS[s].layout[0] for s in range(ns) if P.kind[s] == "wave" and P.children[s]}
    assert {63, 64, 65, 66} <= set(row0), what
    assert [row0[k][2] for k in (63, 64, 65, 66)] == [False, False, True, True], what
    assert all(row0[k][0] == 0 for k in (63, 64, 65, 66)), what


@pytest.mark.parametrize("batch", fc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_block(hip, kind, batch):
    D, LS = _analysed(hip, "block", kind, batch)
    d = D[2, False]
    P, FR = d.P, d.FR
    what = "block %s batch %d\n%s" % (kind, batch, fc.describe(d))
    ns = len(P.w)
    assert not FR.forest.any() and "big" not in P.kind, what
    _check_kernels(D, batch, (), what)
    blk = [s for s in range(ns) if P.kind[s] == "block"]
    # 64 pivots just past the wave kernels and past the LDS-resident fronts; 255, 256, 257 ancestors (the U12 pass takes
    # 256 at a time); triangles of 64: w = 64, 65, 128, 129; the last triangle no multiple of 16 (81 - 64); w around 32
    for rw in ((129, 64), (137, 64), (263, 8), (264, 8), (265, 8), (100, 65), (136, 128), (136, 129), (82, 81), (131, 31), (132, 32), (133, 33)):
        assert rw in _rw(P) and all(P.kind[s] == "block" for s in range(ns) if (P.r[s], P.w[s]) == rw), what
    assert {P.r[s] - P.w[s] for s in blk} >= {255, 256, 257} and {P.w[s] for s in blk} >= {64, 65, 128, 129}, what
    assert any(P.w[s] > fc.SOLVE_BW and (P.w[s] % fc.SOLVE_BW) % 16 for s in blk), what
    assert any(P.r[s] > 256 and P.w[s] == 64 and P.children[s] for s in blk), what       # the 256-thread strides over the rows
    assert any(P.w[s] > 64 and P.parent[s] >= 0 and not P.children[s] for s in blk), what
    # the lists: more chunks than one pass of gather_front takes; exactly one chunk without padding; 64 + 1 entries; a
    # long run that would start at position 63; a run moved to the next chunk because it would straddle a boundary
    assert any(LS[s].chunks > fc.GATHER_CHUNKS for s in blk), what
    assert any(LS[s].chunks == 1 and LS[s].entries == fc.CHUNK for s in blk), what
    assert any(LS[s].entries == fc.CHUNK + 1 and LS[s].chunks == 2 for s in blk), what
    assert any(LS[s].long_at_63 for s in blk), what
    assert any(LS[s].padded for s in blk), what
    long_front = next(s for s in blk if LS[s].long_at_63)
    assert [ly for ly in LS[long_front].layout if ly[2]] == [(0, 66, True), (0, 66, True)], what      # (the second one: moved to position 0)
    assert LS[long_front].layout[62] == (0, 66, True) and LS[long_front].entries == 64 + 3, what
    root = ns - 1
    assert P.parent[root] == -1 and P.kind[root] == "small", what


@pytest.mark.parametrize("batch", fc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_promote(hip, kind, batch):
    """The wave group of a level -- 15 fronts of order <= 32 and the front of order 34 that makes it a wave group -- joins
    the level's block group for a lone matrix; with one front more it does not, and in a batch never."""
    for name, count in (("promote16", 16), ("promote17", 17)):
        D, LS = _analysed(hip, name, kind, batch)
        d = D[2, False]
        P, FR = d.P, d.FR
        what = "%s %s batch %d\n%s" % (name, kind, batch, fc.describe(d))
        assert not FR.forest.any(), what
        group = [s for s in range(len(P.w)) if P.level[s] == 0 and P.r[s] <= 128]
        assert len(group) == count and sum(1 for s in group if P.r[s] <= 32) == count - 1, what
        assert sorted(P.kind[s] for s in range(len(P.w)) if P.level[s] == 0 and s not in group) == ["block"], what
        assert any(P.r[s] <= 16 for s in group) and any(16 < P.r[s] <= 32 for s in group), what
        promoted = group if batch == 1 and count <= fc.PROMOTE_MAX else ()
        _check_kernels(D, batch, promoted, what)
        if batch == 1 and not promoted:                                    # next to the block group all the same
            at = next(i for i, L in enumerate(d.launches) if L.level == 0)
            assert [L.kernel for L in d.launches[at:at + 2]] == ["wave8", "blk"] and d.launches[at + 1].level == 0, what
    assert fc.PROMOTE_MAX == 16


def test_promote16_is_promote17_without_its_extra_leaf(hip):
    for sym in (False, True):
        Ax16, Ax17, cols = fc.promote_pair(sym)
        n16 = fc.case_matrix("promote16")[1]
        assert len(cols) == n16 and len(Ax16) < len(Ax17)


@pytest.mark.parametrize("batch", fc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_reused_cases(hip, kind, batch):
    # hub: a pivot row with more than 65 sources in a wave front -- the long run of the sweeps' own gather -- and the order-136 root
    D, LS = _analysed(hip, "hub", kind, batch)
    d = D[2, False]
    P = d.P
    what = "hub %s batch %d\n%s" % (kind, batch, fc.describe(d))
    _check_kernels(D, batch, (), what)
    longs = [s for s in range(len(P.w)) if any(ly[2] for ly in LS[s].layout)]
    assert longs and all(P.kind[s] == "wave" for s in longs) and max(max(LS[s].runs) for s in longs) > fc.CHUNK + 1, what
    assert P.kind[len(P.w) - 1] == "block" and P.r[len(P.w) - 1] == 136, what
    # t16: fronts of order <= 16 under fronts of 17 .. 32 (lane = matrix under lane = row from 128 matrices on)
    D, LS = _analysed(hip, "t16", kind, batch)
    d = D[2, False]
    what = "t16 %s batch %d\n%s" % (kind, batch, fc.describe(d))
    _check_kernels(D, batch, (), what)
    il = [L for L in d.launches if L.kernel == "il"]
    assert bool(il) == (batch >= rc.IL_MIN_BATCH), what
    if il:
        assert any(d.P.children[s] for L in il for s in L.fronts) and d.launches[-1].kernel == "wave8", what
    # the forest takes every front of order <= 32 whose subtree fits a task, at one plain right-hand side of a lone matrix
    for name in ("hub", "t16"):
        dd = _analysed(hip, name, kind, batch)[0]
        FR = dd[1, False].FR
        assert bool(FR.forest.any()) == (batch == 1), name
        if batch == 1:
            assert all(FR.forest[s] == (FR.r[s] <= 32) for s in range(len(FR.w))), name
            assert "sub" in dd[1, False].kernel_of and "sub" not in dd[2, False].kernel_of, name
            assert kind == "chol" or "sub" not in dd[1, True].kernel_of, name
    # w72: wide fronts with a parent, on the block kernels from 16 matrices on
    D, LS = _analysed(hip, fc.WIDE, kind, batch)
    d = D[2, False]
    what = "w72 %s batch %d\n%s" % (kind, batch, fc.describe(d))
    _check_kernels(D, batch, (), what)
    wide = sc.wide_fronts(d.P)
    assert len(wide) == 3 and {d.kernel_of[s] for s in wide} == {"blk" if batch > sc.BIG_BATCH_MAX else "big"}, what


# ---------------------------------------------------------------------- reference --

NAMES = tuple(fc.TREES)


def _oracle_factors(orc, hip, name, kind):
    m, n, Ap, Ai, _ = fc.case_matrix(name, symmetric=kind == "chol")
    Ax = fc.case_values(name, 1, symmetric=kind == "chol")[0]
    with fc.handle(hip, name, kind, 1) as F:
        q = F.ordering()["q"]
    if kind == "chol":
        return n, q, pc.oracle_chol(orc, n, Ap, Ai, Ax, q), None
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, LU_TOL)
    assert np.array_equal(pinv[q], np.arange(n)), "the oracle left the diagonal"
    return n, q, (Lp, Li, Lx), (Up, Ui, Ux)


def _sweeps(orc, L, U):
    sweeps = [(L, True, False, orc.csc_lsolve_f), (L, True, True, orc.csc_ltsolve_f)]
    if U is not None:
        sweeps += [(U, False, False, orc.csc_usolve_f), (U, False, True, orc.csc_utsolve_f)]
    return sweeps


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_substitute_agrees_with_the_oracles_sweeps_and_the_bound_holds_for_them(orc, hip, name, kind):
    n, q, L, U = _oracle_factors(orc, hip, name, kind)
    B = rc.right_hand_sides(1, n, 15, seed=3)[0]
    for G, lower, trans, fn in _sweeps(orc, L, U):
        X = sc.substitute(n, *G, B, lower, trans)
        X64 = np.empty_like(B)
        for j in range(B.shape[1]):
            want = B[:, j].copy()
            fn(n, *G, want)
            X64[:, j] = want
            scale = np.abs(want).max()
            assert np.abs(X[:, j] - want).max() <= RTOL * scale, (lower, trans, j)
            if j == 2:
                assert scale == 0.0 and not X[:, j].any()
        assert (fc.error_ratio(n, G, X, B, trans)[0] <= 1.0).all(), (lower, trans)
        # the sparse form of the ratio is the dense one of sweep_cases
        ratio = fc.error_ratio(n, G, X64, B, trans)[0]
        if name == "wave":
            dense = sc.substitution_error_ratio(sc.dense(n, *G, trans=trans), X64, B)
            assert np.abs(ratio - dense).max() <= 2 * n * 2.0 ** -11, (lower, trans)        # (n np.longdouble terms per row, 2^-11 u each)
        # a float64 substitution stays inside 2 n u |T||x|, and the bound is no more than three orders above what it reaches
        print("%s %s lower %s trans %s: oracle max |b - T x| / (u |T||x|) = %.2f (2 n = %d)" % (name, kind, lower, trans, ratio.max(), 2 * n))
        assert 2 * n / 1000 <= ratio.max() <= 2 * n, (lower, trans, ratio)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_the_bound_sees_one_slightly_wrong_entry(orc, hip, name, kind):
    """A relative error of 1e-9 in one entry of x, and one in the smallest entry of the factor, is beyond 2 n u |T||x|."""
    n, q, L, U = _oracle_factors(orc, hip, name, kind)
    B = np.random.default_rng(5).standard_normal((n, 1))
    for G, lower, trans, fn in _sweeps(orc, L, U):
        X = B[:, 0].copy()
        fn(n, *G, X)
        X = X[:, None]
        assert fc.error_ratio(n, G, X, B, trans)[0][0] <= 2 * n
        # the entry that the sweep computes LAST feeds no other row: its row of the residual is its own error alone
        last = n - 1 if lower != trans else 0
        X2 = X.copy()
        X2[last] *= 1 + 1e-9
        assert fc.error_ratio(n, G, X2, B, trans)[0][0] > 2 * n, (lower, trans)
        # the smallest entry of the factor, T(i, j), under the right-hand side that isolates it: x = e_j solves T x = T e_j
        # exactly, and no longer once that entry is off by 1e-9 (on a random x the entry's share of its row is too small to see)
        p = int(np.argmin(np.abs(G[2][:G[0][n]])))
        j = int(G[1][p]) if trans else int(np.searchsorted(G[0], p, side="right") - 1)
        E = np.zeros((n, 1))
        E[j] = 1.0
        Bj = fc.products(n, *G, E, trans)[0].astype(np.float64)
        assert fc.error_ratio(n, G, E, Bj, trans)[0][0] == 0.0
        Gx = np.array(G[2], dtype=np.float64, copy=True)
        Gx[p] *= 1 + 1e-9
        assert fc.error_ratio(n, (G[0], G[1], Gx), E, Bj, trans)[0][0] > 2 * n, (lower, trans)
