"""The bottom forest (csrc/forest.hip: k_sub_factor, k_sub_fwd, k_sub_bwd) at its part, task and arena edges.

tests/forest_cases.py builds matrices whose forest has a prescribed shape (asserted without a device in
tests/test_forest_cases_cpu.py): shared fronts of one to four slices whose last slice owns pivots, with and without
contribution columns behind them; pivots that end at a slice edge; local levels of one shared front, two, one beside a
one-wave front, and full levels of 8, 9, 16 and 17 fronts; child blocks of order 15, 16, 17 and 31 into one-wave and
into shared fronts; a task of exactly 64 fronts, one of 4 904 of 5 000 doubles of arena, their neighbours beyond the
limit; five local levels under a front that is outside for its height; 276 islands in 256 tasks.  One handle per
(case, kind); LU and Cholesky.

Every case: factors against the CPU oracle entry by entry and to the componentwise bound 2 n u; the one-right-hand-side
sweeps against a substitution in extended precision on the handle's own factors, per island, norm-wise to 1e-10 and
componentwise to 2 n u |T||x| per half sweep (n: the island's order -- no row of an island sums more terms); the fused
step bit for bit against factor + solve; all of it unchanged bit for bit by a poisoned LDS.  The pivot check at its
threshold in the slices that no other matrix of the suite reaches: the first and the last pivot of a LAST slice that
owns pivots, the last pivot of slice 0.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import forest_cases as fc
import pivot_cases as pc
import sweep_cases as sc
from helpers import (RTOL, assert_backward_error, assert_factor_equal, backward_error_ratio, backward_error_ratio_dense,
                     csc_to_scipy, lower_transposed, permuted)

pytestmark = pytest.mark.gpu

KINDS = ("lu", "chol")
LU_TOL = 1e-3
BOTH = [(name, kind) for name in fc.CASES for kind in KINDS]
IDS = ["%s-%s" % nk for nk in BOTH]


def _tol(kind):
    return LU_TOL if kind == "lu" else 0.0


class _Case:
    """One handle, its shape, the split factorisation's factors and the oracle's, built on first use."""

    def __init__(self, gpu, orc, name, kind):
        self.name, self.kind = name, kind
        self.M = fc.case_matrix(name, symmetric=kind == "chol")
        self.F = fc.handle(gpu, name, kind)
        self.S = fc.shape(gpu, self.F)
        self.q = self.S.FR.q
        self.n = self.M.n
        self.F.factor(self.M.Ax, _tol(kind))
        self.factors = self.F.factors()
        M, n = self.M, self.n
        if kind == "chol":
            self.oracle = pc.oracle_chol(orc, n, M.Ap, M.Ai, M.Ax, self.q) + (None, None, None)
        else:
            o = orc.csc_lu_f(n, n, M.Ap, M.Ai, M.Ax, self.q, LU_TOL)
            assert np.array_equal(o[6][self.q], np.arange(n)), "the oracle left the diagonal"
            self.oracle = o[:6]
        # the islands in pivot order (the analysis keeps them in their order: test_forest_cases_cpu.py)
        isl = np.searchsorted(M.starts, self.q, side="right") - 1
        assert (np.diff(isl) >= 0).all()
        self.blocks = [(int(M.starts[i]), int(M.starts[i + 1])) for i in range(len(M.starts) - 1)]
        self.b = np.random.default_rng(fc.SEEDS[name] + 7).standard_normal(n)

    def refactor(self):
        self.F.factor(self.M.Ax, _tol(self.kind))

    def L(self, f=None):
        return (f or self.factors)[0:3]

    def U(self, f=None):
        return (f or self.factors)[3:6]


@pytest.fixture(scope="module")
def cases(gpu, orc):
    held = {}

    def get(name, kind):
        if (name, kind) not in held:
            held[name, kind] = _Case(gpu, orc, name, kind)
        return held[name, kind]

    yield get
    for c in held.values():
        c.F.close()


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------ factors --

@pytest.mark.parametrize("name,kind", BOTH, ids=IDS)
def test_factors_against_the_oracle(gpu, orc, cases, name, kind):
    c = cases(name, kind)
    M, n = c.M, c.n
    what = "%s %s" % (name, kind)
    assert_factor_equal(n, c.L(), c.oracle[0:3], what + " L")
    A = permuted(n, M.Ap, M.Ai, M.Ax, c.q)
    dense = n <= 2048
    ratio = backward_error_ratio_dense if dense else backward_error_ratio
    if kind == "lu":
        assert_factor_equal(n, c.U(), c.oracle[3:6], what + " U")
        o_ratio, _ = ratio(n, A, c.oracle[0:3], c.oracle[3:6])
        g_ratio = assert_backward_error(n, A, c.L(), c.U(), what, oracle_ratio=o_ratio, dense=dense)
    else:
        o_ratio, _ = ratio(n, A, c.oracle[0:3], lower_transposed(n, c.oracle[0:3]))
        g_ratio = assert_backward_error(n, A, c.L(), lower_transposed(n, c.L()), what, oracle_ratio=o_ratio, dense=dense)
    print("%s: max |PAQ - LU| / (u |L||U|): forest %.2f, oracle %.2f (bound %d)" % (what, g_ratio, o_ratio, 2 * n))
    # again on the same handle, and on a fresh one: bit for bit
    c.refactor()
    assert _same(c.F.factors(), c.factors), what + ": a second factorisation differs"
    with fc.handle(gpu, name, kind) as G:
        G.factor(M.Ax, _tol(kind))
        assert _same(G.factors(), c.factors), what + ": a fresh handle's factors differ"


# ------------------------------------------------------------- one right-hand side --

def _block(G, n, lo, hi, trans):
    """Rows and columns lo .. hi of the triangular factor G (its transpose for trans), dense, np.longdouble."""
    T = sp.csc_matrix((G[2], G[1], G[0]), shape=(n, n))[lo:hi, lo:hi].toarray()
    return (T.T if trans else T).astype(np.longdouble)


def _check_sweep(c, G, lower, trans, got, rhs, what, orc_fn=None):
    """One half sweep `got` = T \\ rhs of the handle against substitute() on the same factor, island by island; -> the
    largest componentwise ratio of the handle's sweep and of the oracle's float64 substitution on the same factor."""
    n = c.n
    want = sc.substitute(n, *G, rhs, lower, trans)
    ref64 = None
    if orc_fn is not None:
        ref64 = np.array(rhs, dtype=np.float64, copy=True)
        orc_fn(n, *G, ref64)
    worst = [0.0, 0.0]
    for i, (lo, hi) in enumerate(c.blocks):
        w = want[lo:hi]
        scale = float(np.abs(w).max())
        err = float(np.abs(got[lo:hi] - w).max())
        assert err <= RTOL * scale, "%s island %d: %.3e of %.3e" % (what, i, err, scale)
        T = _block(G, n, lo, hi, trans)
        ratio = sc.substitution_error_ratio(T, got[lo:hi, None], rhs[lo:hi, None])[0]
        assert ratio <= 2 * (hi - lo), "%s island %d: |b - T x| / (u |T||x|) = %.2f > %d" % (what, i, ratio, 2 * (hi - lo))
        worst[0] = max(worst[0], ratio)
        if ref64 is not None:
            worst[1] = max(worst[1], sc.substitution_error_ratio(T, ref64[lo:hi, None], rhs[lo:hi, None])[0])
    return worst


def _residual_ok(M, x, b):
    A = csc_to_scipy(M.m, M.n, M.Ap, M.Ai, M.Ax)
    return np.abs(A @ x - b).max() <= 1e-12 * (abs(A).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max())


def _split_sweeps(c):
    """-> (x, y, z [, z'])  of solve, lsolve, usolve and, for Cholesky, ltsolve on the case's right-hand side."""
    F, b, q = c.F, c.b, c.q
    y = F.lsolve(b[q])
    out = [F.solve(b), y, F.usolve(y)]
    if c.kind == "chol":
        out.append(F.ltsolve(y))
    return out


@pytest.mark.parametrize("name,kind", BOTH, ids=IDS)
def test_split_sweeps_with_one_right_hand_side(gpu, orc, cases, name, kind):
    c = cases(name, kind)
    c.refactor()
    M, n, q, b, F = c.M, c.n, c.q, c.b, c.F
    what = "%s %s" % (name, kind)
    x, y, z = _split_sweeps(c)[:3]
    assert np.isfinite(x).all() and _residual_ok(M, x, b), what
    L = c.L()
    fwd = _check_sweep(c, L, True, False, y, b[q], what + " lsolve", orc.csc_lsolve_f)
    if kind == "lu":
        bwd = _check_sweep(c, c.U(), False, False, z, y, what + " usolve", orc.csc_usolve_f)
    else:
        bwd = _check_sweep(c, L, True, True, z, y, what + " usolve", orc.csc_ltsolve_f)
        assert np.array_equal(F.ltsolve(y), z), what + ": ltsolve is not usolve"
    print("%s: |b - T x| / (u |T||x|): forward forest %.2f, oracle %.2f; backward forest %.2f, oracle %.2f (n %d)"
          % (what, fwd[0], fwd[1], bwd[0], bwd[1], max(hi - lo for lo, hi in c.blocks)))
    # the full solve is the two half sweeps between the permutations, island by island
    ref = sc.substitute(n, *L, b[q], True, False)
    ref = sc.substitute(n, *(c.U() if kind == "lu" else L), ref, kind != "lu", kind != "lu")
    for i, (lo, hi) in enumerate(c.blocks):
        assert np.abs(x[q][lo:hi] - ref[lo:hi]).max() <= RTOL * float(np.abs(ref[lo:hi]).max()), "%s solve island %d" % (what, i)
    # exactly: a power of two scales through, zero stays zero, a repeat is the same
    assert np.array_equal(F.solve(b * 2.0 ** 40), x * 2.0 ** 40), what
    assert not F.solve(np.zeros(n)).any() and not F.lsolve(np.zeros(n)).any() and not F.usolve(np.zeros(n)).any(), what
    assert _same(_split_sweeps(c), [x, y, z] + ([z] if kind == "chol" else [])), what + ": a repeat differs"


# --------------------------------------------------------------------- fused step --

def _fused(c, times=1, poison=None):
    import torch
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    ax = torch.from_numpy(np.array(c.M.Ax)).to(dev)                    # (a copy: the case's values are read-only)
    out = []
    for _ in range(times):
        xd = torch.from_numpy(c.b.copy()).to(dev)
        if poison:
            poison()
        c.F.factor_solve_dev(ax.data_ptr(), xd.data_ptr(), 1, _tol(c.kind), sh)
        c.F.factor_status(sh)
        out.append(xd.cpu().numpy())
    return out


@pytest.mark.parametrize("name,kind", BOTH, ids=IDS)
def test_fused_step_is_factor_then_solve(gpu, cases, name, kind):
    c = cases(name, kind)
    what = "%s %s" % (name, kind)
    c.refactor()
    x = c.F.solve(c.b)
    c.F.factor(fc.case_matrix(name, symmetric=kind == "chol", other=True).Ax, _tol(kind))     # (other factors in between)
    xs = _fused(c, times=3)                                              # the third call replays the graph
    assert np.array_equal(xs[0], x), what + ": fused x differs from factor + solve"
    assert _same(c.F.factors(), c.factors), what + ": the fused step's factors differ"
    assert np.array_equal(xs[1], x) and np.array_equal(xs[2], x), what + ": a repeat differs"
    assert _same(c.F.factors(), c.factors), what


# ---------------------------------------------------------------------- stale LDS --

@pytest.mark.parametrize("name,kind", BOTH, ids=IDS)
def test_poisoned_lds_changes_nothing(gpu, cases, name, kind):
    c = cases(name, kind)
    what = "%s %s" % (name, kind)
    c.refactor()
    want = _split_sweeps(c)
    c.F.factor(fc.case_matrix(name, symmetric=kind == "chol", other=True).Ax, _tol(kind))
    x = _fused(c, poison=lambda: _poison(gpu))[0]
    assert np.array_equal(x, want[0]), what + ": fused step"
    assert _same(c.F.factors(), c.factors), what + ": fused step's factors"
    F, b, q = c.F, c.b, c.q
    _poison(gpu)
    y = F.lsolve(b[q])
    _poison(gpu)
    z = F.usolve(y)
    _poison(gpu)
    got = [F.solve(b), y, z]
    if kind == "chol":
        _poison(gpu)
        got.append(F.ltsolve(y))
    assert _same(got, want), what + ": split sweeps"
    _poison(gpu)
    c.refactor()
    assert _same(c.F.factors(), c.factors), what + ": factorisation"


# -------------------------------------------------------------------- pivot check --

PIVOT_CASES = ("chain6", "w89", "pair33", "pair44")
WANTED = {"chain6": {(1, 1), (3, 3), (4, 4)}, "w89": {(2, 2)}, "pair33": {(3, 3)}, "pair44": {(4, 4)}}


def _pivot_fronts(S):
    """The shared fronts with rows below their pivots whose last slice owns pivots."""
    return [f for f in S.fronts if f.shared and f.w < f.r and f.cls[0] == f.cls[1]]


def _positions(f):
    """-> {position: label}: the first and the last pivot of the last slice, the last pivot of slice 0."""
    first = fc.SLICE * (f.cls[0] - 1)
    pos = {first: "last slice first", f.w - 1: "last slice last"}
    if f.cls[0] > 1:
        pos[fc.SLICE - 1] = "slice 0 last"
    return pos


def _contrib(FR, s):
    return {"contrib": lambda below, k, e=int(FR.c0[s] + FR.w[s]): below[below >= e][::-1]}


@pytest.mark.parametrize("name", PIVOT_CASES)
def test_lu_threshold_in_the_slices_that_own_the_last_pivots(gpu, orc, cases, name):
    c = cases(name, "lu")
    M, n, F, FR = c.M, c.n, c.F, c.S.FR
    fronts = _pivot_fronts(c.S)
    assert {f.cls for f in fronts} >= WANTED[name], fc.describe(c.S)
    compared = 0
    for f in fronts:
        if f.cls not in WANTED[name]:
            continue
        pos = _positions(f)
        targets = pc.front_targets(FR, M.Ap, M.Ai, f.s, sorted(pos), _contrib(FR, f.s), "%s %s" % (name, f.cls))
        assert len(targets) == len(pos) and all(t.where == "contrib" and t.i >= FR.c0[f.s] + f.w for t in targets)
        for t in targets:
            p = pc.prepare(orc, n, M.Ap, M.Ai, M.Ax, c.q, t)
            what = "%s (%s)" % (t.label, pos[t.k - int(FR.c0[f.s])])
            assert p.i_max == t.i, what
            if p.weight < pc.DECISION_WEIGHT:                          # the engineered pivot is what a cancellation leaves
                continue
            rho = pc.reject_rho(p)
            if p.rho is not None:
                F.factor(p.Ax, rho * (1 - pc.MARGIN))
                if p.weight >= pc.MIN_WEIGHT:
                    got = F.factors()
                    o = orc.csc_lu_f(n, n, M.Ap, M.Ai, p.Ax, c.q, rho * (1 - pc.MARGIN))
                    assert np.array_equal(o[6][c.q], np.arange(n)), what
                    assert_factor_equal(n, got[0:3], o[0:3], what + " L")
                    assert_factor_equal(n, got[3:6], o[3:6], what + " U")
                    assert_backward_error(n, permuted(n, M.Ap, M.Ai, p.Ax, c.q), got[0:3], got[3:6], what, dense=True)
                    compared += 1
            with pytest.raises(gpu.SingularMatrix):
                F.factor(p.Ax, rho * (1 + pc.MARGIN))
            assert F.info.fail_col == t.k == pc.first_off_diagonal(orc, n, M.Ap, M.Ai, p.Ax, c.q, rho * (1 + pc.MARGIN)), what
        # two failing columns in two different slices of one front: the smaller one is reported
        if f.cls[0] > 1:
            t1, t2 = [t for t in targets if t.k - FR.c0[f.s] in (fc.SLICE - 1, fc.SLICE * (f.cls[0] - 1))]
            assert t1.k < t2.k and (t1.k - FR.c0[f.s]) // fc.SLICE != (t2.k - FR.c0[f.s]) // fc.SLICE
            Ax2, tol = pc.prepare_two(orc, n, M.Ap, M.Ai, M.Ax, c.q, t1, t2)
            assert pc.first_off_diagonal(orc, n, M.Ap, M.Ai, Ax2, c.q, tol) == t1.k
            with pytest.raises(gpu.SingularMatrix):
                F.factor(Ax2, tol)
            assert F.info.fail_col == t1.k, "%s: fail_col %d, the engineered columns are %d < %d" % (name, F.info.fail_col, t1.k, t2.k)
    assert compared >= 2 * len(WANTED[name]), compared
    c.refactor()                                                         # the handle recovers
    assert F.info.fail_col == -1 and _same(F.factors(), c.factors)


@pytest.mark.parametrize("name", PIVOT_CASES)
def test_cholesky_pivot_just_below_and_just_above_zero_in_those_slices(gpu, orc, cases, name):
    c = cases(name, "chol")
    M, n, F, FR = c.M, c.n, c.F, c.S.FR
    fronts = _pivot_fronts(c.S)
    assert {f.cls for f in fronts} >= WANTED[name], fc.describe(c.S)
    for f in fronts:
        for j, label in sorted(_positions(f).items()):
            k = int(FR.c0[f.s]) + j
            what = "%s %s p%d (%s)" % (name, f.cls, j, label)
            neg = pc.engineer_chol(orc, n, M.Ap, M.Ai, M.Ax, c.q, k, -1.0)
            assert pc.chol_fail_step(orc, n, M.Ap, M.Ai, neg, c.q) == k
            with pytest.raises(gpu.NotPositiveDefinite):
                F.factor(neg)
            assert F.info.fail_col == k, what
            pos = pc.engineer_chol(orc, n, M.Ap, M.Ai, M.Ax, c.q, k, +1.0)
            later = pc.chol_fail_step(orc, n, M.Ap, M.Ai, pos, c.q)
            assert later is not None and later > k, what                 # (every one of these pivots has rows below it)
            with pytest.raises(gpu.NotPositiveDefinite):
                F.factor(pos)
            assert F.info.fail_col == later, what
    c.refactor()
    assert F.info.fail_col == -1 and _same(F.factors(), c.factors)
