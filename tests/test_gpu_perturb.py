"""Static pivot perturbation on the GPU (cs3_set_pivot_perturbation / cs3_get_perturbed / cs3_refine): a pivot with
|p| < delta is replaced by +delta, in every factor kernel, in the STORED U_kk; the factors are those of A(q, q) + diag(E).

The matrices are those of tests/pivot_cases.py with a pivot of a chosen size at a chosen place (tests/perturb_cases.py);
what the CPU can say about them is asserted in tests/test_perturb_cpu.py.  Componentwise bound of test 2:
|L U - A(q, q) - diag(E_ref)|_ij <= 4 k u (|L||U|)_ij, k the largest column count of L; the largest ratio (in units of
k u) per class is printed and recorded in DESIGN.md section 7."""
import ctypes as C

import numpy as np
import pytest

import perturb_cases as pp
import pivot_cases as pc
from helpers import canon, csc_to_scipy, rel_err

pytestmark = pytest.mark.gpu


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def handles(gpu):
    """One handle per (matrix, batch), shared by every test of this module; the LDS is poisoned before the first."""
    _poison(gpu)
    held = {}

    def get(name, batch):
        if (name, batch) not in held:
            m, n, Ap, Ai, _ = pc.matrix(name)
            held[name, batch] = gpu.Factorization(m, n, Ap, Ai, batch=batch)
        return held[name, batch]

    yield get
    for F in held.values():
        F.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _diag_u(n, fac):
    """U_kk of cs3_get_factors' arrays, for every k."""
    Up, Ui, Ux = canon(n, *fac[3:6])
    last = Up[1:n + 1] - 1
    assert np.array_equal(Ui[last], np.arange(n))
    return Ux[last]


def _slot(batch, t):
    return pp.BATCH_SLOTS[batch][t % len(pp.BATCH_SLOTS[batch])] if batch > 1 else 0


def _expect_count(batch, slot, count):
    want = np.zeros(batch, dtype=np.int64)
    want[slot] = count
    return want


# 1. the threshold, per kernel class
@pytest.mark.parametrize("name,cls", pp.CLASSES, ids=pp.IDS)
def test_threshold_leaves_a_pivot_above_delta_alone_and_replaces_one_below(gpu, orc, handles, name, cls):
    case = pc.lu_case(gpu, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    batch = name[1]
    F = handles(*name)
    AX0 = pp.batch_values(Ax, batch, seed=batch)
    got = pp.picked(gpu, orc, name, cls)
    assert got
    for t, (lo, _, _) in enumerate(got):
        k, slot = lo.target.k, _slot(batch, t)
        what = "%s b%d %s" % (name[0], batch, lo.target.label)
        assert case["FR"].cls[lo.target.front] == cls and lo.weight >= pc.DECISION_WEIGHT
        AX = pp.with_slot(AX0, slot, lo.Ax)
        F.set_perturbation(0.0).factor(AX, 0.0)
        assert not F.perturbed().any(), what
        plain = F.factors(b=slot)
        # just below |u|: nothing is touched, bit for bit
        F.set_perturbation(abs(lo.u) * (1 - pc.MARGIN)).factor(AX, 0.0)
        assert not F.perturbed().any(), what
        same = F.factors(b=slot)
        assert _same_bits(same[2], plain[2]) and _same_bits(same[5], plain[5]), what
        # just above: that pivot alone, in that matrix alone, and delta is what is stored
        delta = abs(lo.u) * (1 + pc.MARGIN)
        F.set_perturbation(delta).factor(AX, 0.0)
        assert np.array_equal(F.perturbed(), _expect_count(batch, slot, 1)), what
        d = _diag_u(n, F.factors(b=slot))
        assert _same_bits(d[k], delta), "%s: U_kk = %r, delta = %r" % (what, d[k], delta)
        assert list(np.flatnonzero(_bits(d) == _bits(delta))) == [k], what
    F.set_perturbation(0.0)


# 2. a real perturbation, per kernel class
@pytest.mark.parametrize("name,cls", pp.CLASSES, ids=pp.IDS)
def test_factors_are_those_of_the_reference_perturbed_matrix(gpu, orc, handles, name, cls):
    case = pc.lu_case(gpu, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    batch = name[1]
    F = handles(*name)
    AX0 = pp.batch_values(Ax, batch, seed=batch)
    worst = 0.0
    for t, (_, hi, ref) in enumerate(pp.picked(gpu, orc, name, cls)):
        slot = _slot(batch, t)
        what = "%s b%d %s" % (name[0], batch, hi.target.label)
        delta = pp.DELTA_OF_M * hi.M
        F.set_perturbation(delta).factor(pp.with_slot(AX0, slot, hi.Ax), 0.0)
        assert F.info.fail_col == -1
        assert np.array_equal(F.perturbed(), _expect_count(batch, slot, len(ref.perturbed))), what
        fac = F.factors(b=slot)
        d = _diag_u(n, fac)
        assert np.array_equal(np.flatnonzero(_bits(d) == _bits(delta)), ref.perturbed), what
        for g, w in ((fac[0:3], ref.factors[0:3]), (fac[3:6], ref.factors[3:6])):         # the oracle's pattern
            gp, gi, _ = canon(n, *g)
            wp, wi, _ = canon(n, *w)
            assert np.array_equal(gp, wp) and np.array_equal(gi, wi), what
        ratio, nz_bad = pp.bound_ratio(n, Ap, Ai, ref.Ax, q, fac[0:3], fac[3:6])
        print("%s: |LU - A - E_ref| / (k u |L||U|) = %.3f" % (what, ratio))
        assert nz_bad == 0 and ratio <= pp.C_BOUND, "%s: ratio %.3f" % (what, ratio)
        worst = max(worst, ratio)
    print("%s b%d %s: max ratio %.3f (bound %.1f)" % (name[0], batch, cls, worst, pp.C_BOUND))
    F.set_perturbation(0.0)


def _first_pivot(case, cls, leaf):
    FR = case["FR"]
    if leaf:
        s = next(s for s in range(len(FR.w)) if FR.cls[s] == cls and FR.level[s] == 0 and FR.r[s] > FR.w[s])
    else:
        s = next(s for s in range(len(FR.w)) if FR.cls[s] == cls and FR.w[s] > 136)
    return int(FR.c0[s])


# 3. an exact zero, 4. a NaN
@pytest.mark.parametrize("name,cls,leaf", [(("grid4000", 1), "forest_wave", True), (("db180", 1), "big_step", False)],
                         ids=["leaf", "big_front"])
def test_exact_zero_is_replaced_and_nan_is_not(gpu, orc, handles, name, cls, leaf):
    case = pc.lu_case(gpu, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    F = handles(*name)
    k = _first_pivot(case, cls, leaf)
    p = pc._entry(Ap, Ai, q[k], q[k])
    zero = Ax.copy()
    zero[p] = 0.0                                            # (nothing updates this entry before its turn: the pivot IS 0.0)
    F.set_perturbation(0.0)
    with pytest.raises(gpu.SingularMatrix):
        F.factor(zero, 0.0)
    assert F.info.fail_col == k
    delta = gpu.perturbation_delta(True, Ax, False)
    F.set_perturbation(delta).factor(zero, 0.0)
    assert F.info.fail_col == -1 and list(F.perturbed()) == [1]
    assert _same_bits(_diag_u(n, F.factors())[k], delta)
    nan = Ax.copy()
    nan[p] = np.nan
    with pytest.raises(gpu.SingularMatrix):
        F.factor(nan, 0.0)
    assert F.info.fail_col == k
    F.set_perturbation(0.0).factor(Ax, 1e-3)                 # the handle recovers
    assert F.info.fail_col == -1 and list(F.perturbed()) == [0]


def _tiny_for(gpu, orc, name, cls):
    _, hi, ref = pp.picked(gpu, orc, name, cls)[-1]
    return hi, ref


# 5. fused = split
@pytest.mark.parametrize("name,cls", [(("grid4000", 1), "forest_wave"), (("db180", 1), "big_step")], ids=["forest", "big_step"])
@pytest.mark.parametrize("nrhs", [1, 5])
def test_fused_step_equals_factor_then_solve(gpu, orc, handles, name, cls, nrhs):
    import torch
    case = pc.lu_case(gpu, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    F = handles(*name)
    hi, ref = _tiny_for(gpu, orc, name, cls)
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    b = np.random.default_rng(nrhs).standard_normal((n, nrhs) if nrhs > 1 else n)
    ax, bt = torch.from_numpy(hi.Ax).to(dev), torch.from_numpy(b).to(dev)
    F.set_perturbation(pp.DELTA_OF_M * hi.M)
    x_split = bt.clone()
    F.factor_dev(ax.data_ptr(), 0.0, sh)
    F.solve_dev(x_split.data_ptr(), nrhs, sh)
    F.factor_status(sh)
    count = F.perturbed(sh)
    assert list(count) == [len(ref.perturbed)]
    x_fused = bt.clone()
    F.factor_solve_dev(ax.data_ptr(), x_fused.data_ptr(), nrhs, 0.0, sh)
    F.factor_status(sh)
    assert np.array_equal(F.perturbed(sh), count) and torch.equal(x_fused, x_split)
    x_bx = torch.zeros_like(bt)
    F.factor_solve_bx_dev(ax.data_ptr(), bt.data_ptr(), x_bx.data_ptr(), nrhs, 0.0, sh)
    F.factor_status(sh)
    assert np.array_equal(F.perturbed(sh), count) and torch.equal(x_bx, x_split)
    assert torch.isfinite(x_split).all()
    F.set_perturbation(0.0)


# 6. switching delta on one handle
def test_switching_delta_drops_the_graphs(gpu, orc, handles):
    import torch
    name, cls = ("grid4000", 1), "forest_wave"
    case = pc.lu_case(gpu, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    F = handles(*name)
    hi, ref = _tiny_for(gpu, orc, name, cls)
    d1 = pp.DELTA_OF_M * hi.M
    F.set_perturbation(d1).factor(hi.Ax, 0.0)
    assert list(F.perturbed()) == [1]
    F.set_perturbation(0.0).factor(hi.Ax, 0.0)
    assert list(F.perturbed()) == [0]
    got = F.factors()
    with gpu.Factorization(m, n, Ap, Ai) as G:
        want = G.factor(hi.Ax, 0.0).factors()
        assert list(G.perturbed()) == [0]
    assert _same_bits(got[2], want[2]) and _same_bits(got[5], want[5])
    # fused calls with one X: the fourth replays a graph of its own; a new delta must not replay it
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    b = np.random.default_rng(6).standard_normal(n)
    ax, bt = torch.from_numpy(hi.Ax).to(dev), torch.from_numpy(b).to(dev)
    x = torch.zeros_like(bt)
    F.set_perturbation(d1)
    for _ in range(4):
        F.factor_solve_bx_dev(ax.data_ptr(), bt.data_ptr(), x.data_ptr(), 1, 0.0, sh)
    F.factor_status(sh)
    x1 = x.clone()
    d2 = 16.0 * d1
    F.set_perturbation(d2)
    F.factor_solve_bx_dev(ax.data_ptr(), bt.data_ptr(), x.data_ptr(), 1, 0.0, sh)
    F.factor_status(sh)
    assert list(F.perturbed(sh)) == [1]
    x2 = x.clone()
    assert not torch.equal(x1, x2)
    xs = bt.clone()
    F.factor_dev(ax.data_ptr(), 0.0, sh)
    F.solve_dev(xs.data_ptr(), 1, sh)
    F.factor_status(sh)
    assert torch.equal(x2, xs)
    assert _same_bits(_diag_u(n, F.factors())[hi.target.k], d2)
    F.set_perturbation(0.0)


# 7. end to end
@pytest.mark.parametrize("match", [False, True], ids=["plain", "matched"])
def test_lusol_with_perturbation_agrees_with_partial_pivoting(gpu, orc, match):
    from csparse3_amd import csc
    _poison(gpu)
    (m, n, Ap, Ai, Ax), b, x_ref, k = pp.end_to_end(gpu, orc)
    A = csc.CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    x = csc.lusol(A, b, perturb=True, match=match)
    assert rel_err(x, x_ref) <= 1e-10, rel_err(x, x_ref)
    assert _same_bits(csc.csc_lusol_f(1, m, n, Ap, Ai, Ax, b, perturb=True, match=match), x)
    F = A.lu(match=match, perturb=True)
    count = int(F.perturbed()[0])
    # the rounds lusol ran, one at a time
    xs, corr, prev = F.solve(b), [], np.inf
    for _ in range(10 if count else 0):
        x_new, c = F.refine(Ax, b, xs, 1)
        corr.append(c)
        if not c <= prev:
            break
        xs = x_new
        if not c < 0.5 * prev:
            break
        prev = c
    print("%s: %d perturbed, corrections %s" % ("matched" if match else "plain", count, ["%.1e" % c for c in corr]))
    assert len(corr) < 10 and _same_bits(xs, x)
    # cs3_refine is cs3_refine_dev on staged copies: the same bits, the last correction included
    import torch
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    x0 = F.solve(b)
    ax_d, b_d, x_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (Ax, b, x0))
    c_dev = F.refine_dev(ax_d.data_ptr(), b_d.data_ptr(), x_d.data_ptr(), 1, 2, sh)
    x_host, c_host = F.refine(Ax, b, x0, 2)
    assert _same_bits(x_d.cpu().numpy(), x_host) and _same_bits(c_dev, c_host)
    if match:
        # the matching moves the engineered row off the diagonal: the CPU reference on B replaces nothing, and neither
        # may the handle (test 8 covers a matched handle that does replace pivots)
        import match_cases as mc
        rowperm, dr, dc = F.matching()
        Bp, Bi, Bx = mc.scaled(mc.Case("e2e", n, Ap, Ai, Ax, 1, None, ()), Ax, rowperm, dr, dc)
        ref_b = pp.reference(orc, (n, n, Bp, Bi, Bx), F.ordering()["q"], gpu.perturbation_delta(True, Ax, True))
        assert count == len(ref_b.perturbed) == 0 and corr == []
        return
    assert count >= 1
    with pytest.raises(gpu.SingularMatrix):
        csc.lusol(A, b, tol=1e-3)
    # slogdet describes the perturbed matrix: the reference's sum of log |U_kk|
    q = F.ordering()["q"]
    ref = pp.reference(orc, (m, n, Ap, Ai, Ax), q, gpu.perturbation_delta(True, Ax, False))
    assert count == len(ref.perturbed) and k in ref.perturbed
    d = pp.diag_of_u(n, ref.factors[3], ref.factors[5])
    sign, logabs = F.slogdet()
    want = float(np.log(np.abs(d)).sum())
    assert sign[0] == np.prod(np.sign(d)) and abs(logabs[0] - want) <= 1e-12 * abs(want), (logabs[0], want)


# 8. a matched handle: delta refers to B
def test_matched_handle_perturbs_b(gpu, orc):
    _poison(gpu)
    R = pp.matched_case(gpu, orc)
    c, ref, q = R["c"], R["ref"], R["q"]
    Bp, Bi, _ = R["B"]
    with gpu.Factorization(c.n, c.n, c.Ap, c.Ai, match_values=c.Ax) as F:
        assert np.array_equal(F.ordering()["q"], q)
        F.set_perturbation(R["delta"]).factor(c.Ax, 0.0)
        assert list(F.perturbed()) == [len(ref.perturbed)]
        fac = F.factors()
        d = _diag_u(c.n, fac)
        assert np.array_equal(np.flatnonzero(_bits(d) == _bits(R["delta"])), ref.perturbed)
        kept = []                                            # (B + B' is analysed: drop what the elimination never fills)
        for Gp, Gi, Gx in (fac[0:3], fac[3:6]):
            G = csc_to_scipy(c.n, c.n, Gp, Gi, Gx).copy()
            G.eliminate_zeros()
            kept.append((G.indptr, G.indices, G.data))
        ratio, nz_bad = pp.bound_ratio(c.n, Bp, Bi, ref.Ax, q, kept[0], kept[1])
        print("matched %s: %d perturbed, ratio %.3f" % (c.name, len(ref.perturbed), ratio))
        assert nz_bad == 0 and ratio <= pp.C_BOUND
        F.set_perturbation(0.0).factor(c.Ax, 0.0)
        assert list(F.perturbed()) == [0]
