"""The matrices of tests/rhs_cases.py against the host analysis and the CPU oracle alone (no GPU): every case delivers
the fronts, the slot-round counts, the level groups and the register-size instances that
tests/test_gpu_many_rhs_edges.py is written for, in every batch it runs; the oracle keeps the diagonal on them, the
high-precision substitution that the GPU tests use as their reference agrees with the oracle's four sweeps, and the
componentwise bound asserted there holds for the oracle's own float64 sweeps without being vacuous."""
import numpy as np
import pytest

import pivot_cases as pc
import rhs_cases as rc
import sweep_cases as sc
from helpers import RTOL

KINDS = ("lu", "chol")
LU_TOL = 1e-3

_PLANS = {}


def _plan(hip, name, kind, batch):
    if (name, kind, batch) not in _PLANS:
        with rc.handle(hip, name, kind, batch) as F:
            _PLANS[name, kind, batch] = rc.plan(hip, F)
    return _PLANS[name, kind, batch]


def _with_children(P, g):
    return any(P.children[s] for s in g.fronts)


def _small_group(P, lo, hi):
    """The (level, 'small') groups above the leaves whose largest order is in lo .. hi and that hold a front with children."""
    return [g for g in P.groups if g.kind == "small" and g.level > 0 and lo <= g.max_r <= hi and _with_children(P, g)]


def _check_common(P, batch, what):
    ns = len(P.w)
    il = batch >= rc.IL_MIN_BATCH
    for s in range(ns):
        want = "il" if il and P.r[s] <= 16 else "small" if P.r[s] <= 32 else "wave" if P.r[s] <= 128 and P.w[s] <= 64 else \
            "big" if P.w[s] > 64 and P.r[s] > 136 and batch <= sc.BIG_BATCH_MAX else "block"
        assert P.kind[s] == want, what
    assert sorted(P.schedule) == list(range(ns))
    assert all(g.rmax == rc.rmax_of(g.max_r) for g in P.groups if g.kind == "small")
    if il:
        # the fronts of order <= 16 sweep lane = matrix, and a lane = right-hand-side front reads what they hand up
        assert any(P.kind[s] == "small" and 17 <= P.r[s] <= 32 and any(P.kind[c] == "il" for c in P.children[s]) for s in range(ns)), what
        assert all(P.kind[s] == "il" for s in range(ns) if P.r[s] <= 16), what
    else:
        assert "il" not in P.kind, what


@pytest.mark.parametrize("batch", rc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_t16(hip, kind, batch):
    P = _plan(hip, "t16", kind, batch)
    what = "t16 %s batch %d\n%s" % (kind, batch, rc.describe(P))
    _check_common(P, batch, what)
    root = len(P.w) - 1
    assert P.parent[root] == -1 and P.r[root] == P.w[root] and 17 <= P.r[root] <= 32, what
    assert (P.parent[:root] >= 0).all(), what
    # a level above the leaves whose fronts all have order <= 16, one of them with 9 slot rounds or more
    lv = [l for l in range(1, int(P.level.max()) + 1) if all(P.r[s] <= 16 for s in range(len(P.w)) if P.level[s] == l)]
    assert lv, what
    on = [s for s in range(len(P.w)) if P.level[s] in lv]
    assert any(P.rounds[s] >= 9 for s in on) and all(P.children[s] for s in on), what
    if batch < rc.IL_MIN_BATCH:
        gs = _small_group(P, 1, 16)
        assert gs and all(g.rmax == 16 for g in gs), what
        assert any(P.rounds[s] >= 9 for g in gs for s in g.fronts), what
    else:
        assert all(P.kind[s] == "il" for s in on), what


@pytest.mark.parametrize("batch", rc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_t24(hip, kind, batch):
    P = _plan(hip, "t24", kind, batch)
    what = "t24 %s batch %d\n%s" % (kind, batch, rc.describe(P))
    _check_common(P, batch, what)
    gs = _small_group(P, 17, 24)
    assert gs and all(g.rmax == 24 for g in gs), what
    fronts = [s for g in gs for s in g.fronts]
    assert any(P.r[s] % 8 for s in fronts), what
    assert any(P.rounds[s] >= 9 for s in fronts), what
    assert any(P.rounds[s] == rc.SLOT_ROUNDS_RHS + 1 for s in fronts), what
    root = len(P.w) - 1
    assert P.parent[root] == -1 and P.r[root] == P.w[root] <= 32, what


@pytest.mark.parametrize("batch", rc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_t32(hip, kind, batch):
    P = _plan(hip, "t32", kind, batch)
    what = "t32 %s batch %d\n%s" % (kind, batch, rc.describe(P))
    _check_common(P, batch, what)
    gs = [g for g in _small_group(P, 25, 32) if P.parent[g.fronts[0]] >= 0]        # (the root is a group of its own)
    assert len(gs) == 1 and gs[0].rmax == 32, what
    fronts = gs[0].fronts
    assert any(P.r[s] == 32 for s in fronts) and any(P.r[s] == 17 for s in fronts), what
    assert any(P.rounds[s] >= 3 * rc.SLOT_ROUNDS_RHS + 1 for s in fronts), what         # a fourth pass: three reloads
    assert any(P.w[s] == 1 and P.children[s] for s in fronts), what
    assert any(P.r[s] - P.w[s] == 1 and P.children[s] for s in fronts), what
    root = len(P.w) - 1
    assert P.parent[root] == -1 and P.r[root] == P.w[root] <= 32, what


@pytest.mark.parametrize("batch", rc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_hub(hip, kind, batch):
    P = _plan(hip, "hub", kind, batch)
    what = "hub %s batch %d\n%s" % (kind, batch, rc.describe(P))
    _check_common(P, batch, what)
    ns = len(P.w)
    gemm = [s for s in range(ns) if P.kind[s] in ("wave", "block")]
    assert "big" not in P.kind, what
    assert any(P.kind[s] == "wave" and 33 <= P.r[s] <= 64 for s in gemm), what
    assert any(P.kind[s] == "wave" and 65 <= P.r[s] <= 128 for s in gemm), what
    assert any(P.kind[s] == "block" and P.r[s] == 136 for s in gemm), what
    small_or_il = ("small", "il")
    for s in gemm:                                                         # small fronts hang under each of them
        kids = [c for c in P.children[s] if P.kind[c] in small_or_il and P.r[c] - P.w[c] >= 2]
        assert 10 <= len(kids) <= 13, what
    # k_gemm_gather: exactly one full pass of 64 rounds, and one round past it, on two fronts; the rounds beyond the small
    # children's come from single-column leaves that all add to one row
    assert sorted(int(P.rounds[s]) for s in gemm if P.kind[s] == "wave") == [rc.SLOT_ROUNDS_GATHER, rc.SLOT_ROUNDS_GATHER + 1], what
    for s in gemm:
        if P.kind[s] == "wave":
            assert sum(1 for c in P.children[s] if P.w[c] == 1 and P.r[c] == 2) >= 50, what
    # two GEMM fronts in one launch group
    assert [len(g.fronts) for g in P.groups if g.kind == "wave"] == [2], what
    root = ns - 1
    assert P.parent[root] == -1 and P.r[root] == P.w[root] == 136, what


def test_every_register_size_instance_has_a_group_with_children(hip):
    seen = {}
    for name in rc.TREES:
        for kind in KINDS:
            for batch in rc.BATCHES:
                if batch >= rc.IL_MIN_BATCH:
                    continue
                P = _plan(hip, name, kind, batch)
                for g in P.groups:
                    if g.kind == "small" and _with_children(P, g):
                        seen.setdefault((kind, g.rmax), set()).add(name)
    assert set(seen) == {(kind, rmax) for kind in KINDS for rmax in (16, 24, 32)}, seen


# ---------------------------------------------------------------------- reference --

def _oracle_factors(orc, hip, name, kind, other=False):
    m, n, Ap, Ai, _ = rc.case_matrix(name, symmetric=kind == "chol")
    Ax = rc.case_values(name, 1, symmetric=kind == "chol", other=other)[0]
    with rc.handle(hip, name, kind, 1) as F:
        q = F.ordering()["q"]
    if kind == "chol":
        return n, q, pc.oracle_chol(orc, n, Ap, Ai, Ax, q), None
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, LU_TOL)
    assert np.array_equal(pinv[q], np.arange(n)), "the oracle left the diagonal"
    return n, q, (Lp, Li, Lx), (Up, Ui, Ux)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(rc.TREES))
def test_substitute_agrees_with_the_oracles_sweeps_and_the_bound_is_neither_vacuous_nor_too_tight(orc, hip, name, kind):
    n, q, L, U = _oracle_factors(orc, hip, name, kind)
    B = rc.right_hand_sides(1, n, 17, seed=3)[0]
    sweeps = [(L, True, False, orc.csc_lsolve_f), (L, True, True, orc.csc_ltsolve_f)]
    if U is not None:
        sweeps += [(U, False, False, orc.csc_usolve_f), (U, False, True, orc.csc_utsolve_f)]
    for G, lower, trans, fn in sweeps:
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
        T = sc.dense(n, *G, trans=trans)
        assert (sc.substitution_error_ratio(T, X, B) <= 1.0).all(), (lower, trans)
        # a float64 substitution stays inside 2 n u |T||x| and uses more than a thousandth of it: the bound that the GPU
        # tests assert holds for a correct sweep, and it is no more than three orders above what a correct sweep reaches
        ratio = sc.substitution_error_ratio(T, X64, B).max()
        assert 2 * n / 1000 <= ratio <= 2 * n, (lower, trans, ratio)


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_value_sets_of_the_state_tests_have_different_solutions(orc, hip, kind):
    """Column by column the solutions of A1 x = b and A2 x = b differ by more than 1e-3 relative: a sweep with the
    inverted diagonal blocks of the other factorisation cannot pass for the right one under 1e-10."""
    m, n, Ap, Ai, _ = rc.case_matrix("hub", symmetric=kind == "chol")
    B = np.random.default_rng(11).standard_normal((n, 16))
    X = []
    for other in (False, True):
        Ax = rc.case_values("hub", 1, symmetric=kind == "chol", other=other)[0]
        A = sc.dense64(n, Ap, Ai, Ax)
        X.append(np.linalg.solve(A, B))
    diff = np.abs(X[0] - X[1]).max(axis=0) / np.abs(X[0]).max(axis=0)
    assert (diff > 1e-3).all(), diff
    # ... and so do the inverses of the diagonal blocks themselves: the factors' diagonals differ
    which = 2 if kind == "chol" else 3                                     # (LU: L has a unit diagonal, the pivots are U's)
    d = [np.abs(np.diag(sc.dense64(n, *_oracle_factors(orc, hip, "hub", kind, other=o)[which]))) for o in (False, True)]
    assert (np.abs(d[0] - d[1]) > 1e-3 * d[0]).mean() > 0.5
