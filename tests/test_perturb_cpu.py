"""Static pivot perturbation on the CPU alone (no GPU): the ground tests/test_gpu_perturb.py stands on.  The reference of
tests/perturb_cases.py gives, for every engineered case, factors whose product differs from A(q, q) on the diagonal only,
at its perturbed set only, by what makes the pivot delta; it meets the componentwise bound the kernels are held to; and
refinement against A with a solver for A + E converges within the cap of lusol()."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import perturb_cases as pp
import pivot_cases as pc
from helpers import U_ROUND, csc_to_scipy, rel_err


@pytest.mark.parametrize("name,cls", pp.CLASSES, ids=pp.IDS)
def test_reference_perturbs_the_engineered_pivot_alone(hip, orc, name, cls):
    case = pc.lu_case(hip, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    got = pp.picked(hip, orc, name, cls)
    assert 1 <= len(got) <= 2, "%s: %d targets" % (cls, len(got))
    kinds = set(t.where for t in (p.target for p in case["targets"]) if t.cls == cls)
    if kinds & set(pp._NEAR) and kinds & set(pp._FAR):
        assert len(got) == 2 and len(set(hi.target.where in pp._NEAR for _, hi, _ in got)) == 2, cls
    worst = 0.0
    for lo, hi, ref in got:
        t = hi.target
        what = "%s %s" % (name[0], t.label)
        assert case["FR"].cls[t.front] == cls and lo.weight >= pc.DECISION_WEIGHT
        delta = pp.DELTA_OF_M * hi.M
        assert abs(hi.u) < delta and ref.rounds <= pp.MAX_ROUNDS
        # the threshold test's matrix: no other pivot anywhere near the engineered one
        d_lo = pp.diag_of_u(n, *[orc.csc_lu_f(n, n, Ap, Ai, lo.Ax, q, 0.0)[i] for i in (3, 5)])
        assert d_lo[t.k] == lo.u and np.abs(np.delete(d_lo, t.k)).min() >= 10 * abs(lo.u), what
        L, U = ref.factors[0:3], ref.factors[3:6]
        d = pp.diag_of_u(n, U[0], U[2])
        # L U - A(q, q) is diag(E): E is nonzero at the perturbed set alone, L U equals A(q, q) + diag(E) to the bound
        assert list(ref.perturbed) == [t.k] and list(np.flatnonzero(ref.E)) == [t.k], what
        ratio, nz_bad = pp.bound_ratio(n, Ap, Ai, ref.Ax, q, L, U)
        assert nz_bad == 0 and ratio <= pp.C_BOUND, "%s: ratio %.2f" % (what, ratio)
        worst = max(worst, ratio)
        # U_kk is delta there (to the rounding of the corrected entry: perturb_cases), E_kk is what was missing
        w = pp.abs_product_diagonal(n, L, U)
        assert delta <= d[t.k] <= delta + pp.PIVOT_SLACK * U_ROUND * w[t.k], what
        assert abs(ref.E[t.k] - (delta - hi.u)) <= pp.PIVOT_SLACK * U_ROUND * w[t.k], what
        # every other pivot is ten times delta or more: only the engineered pivot decides
        assert np.abs(np.delete(d, t.k)).min() >= 10 * delta, what
    print("%s b%d %s: reference max |LU - A - E| / (k u |L||U|) = %.3f" % (name[0], name[1], cls, worst))


def test_reference_on_a_matched_handle_perturbs_a_few_pivots_of_b(hip, orc):
    R = pp.matched_case(hip, orc)
    c, ref = R["c"], R["ref"]
    assert 1 <= len(ref.perturbed) <= 8
    Bp, Bi, _ = R["B"]
    ratio, nz_bad = pp.bound_ratio(c.n, Bp, Bi, ref.Ax, R["q"], ref.factors[0:3], ref.factors[3:6])
    assert nz_bad == 0 and ratio <= pp.C_BOUND


def _corrected(n, Ap, Ai, ref, q):
    """A + E in A's own rows and columns: E_kk sits at (q[k], q[k])."""
    return csc_to_scipy(n, n, Ap, Ai, ref.Ax)


def test_refinement_converges_within_the_cap_plain(hip, orc):
    """lusol(perturb=True) on the end-to-end case, emulated: SciPy's splu of A + E solves, A forms the residual."""
    (m, n, Ap, Ai, Ax), b, x_ref, k = pp.end_to_end(hip, orc)
    case = pc.lu_case(hip, orc, ("grid4000", 1))
    q = case["FR"].q
    delta = hip.perturbation_delta(True, Ax, False)
    ref = pp.reference(orc, (m, n, Ap, Ai, Ax), q, delta)
    assert k in ref.perturbed
    lu = spla.splu(_corrected(n, Ap, Ai, ref, q).tocsc())
    x, corr = pp.refine_loop(lu.solve, csc_to_scipy(n, n, Ap, Ai, Ax), b)
    assert len(corr) < 10 and rel_err(x, x_ref) <= 1e-10, (corr, rel_err(x, x_ref))
    print("plain: %d perturbed, corrections %s" % (len(ref.perturbed), ["%.1e" % c for c in corr]))


def test_refinement_converges_within_the_cap_matched(hip, orc):
    """The same with the matching in front: delta = sqrt(eps) refers to B; x = Dc (B + E)^-1 (Dr P b)."""
    (m, n, Ap, Ai, Ax), b, x_ref, _ = pp.end_to_end(hip, orc)
    import match_cases as mc
    with hip.Factorization(n, n, Ap, Ai, match_values=Ax) as F:
        rowperm, dr, dc = F.matching()
        q = F.ordering()["q"]
    c = mc.Case("e2e", n, Ap, Ai, Ax, 1, None, ())
    Bp, Bi, Bx = mc.scaled(c, Ax, rowperm, dr, dc)
    delta = hip.perturbation_delta(True, Ax, True)
    ref = pp.reference(orc, (n, n, Bp, Bi, Bx), q, delta)      # (the matching may leave nothing to perturb: that is its job)
    lu = spla.splu(csc_to_scipy(n, n, Bp, Bi, ref.Ax).tocsc())
    solve = lambda r: dc * lu.solve((dr * r)[rowperm])                   # noqa: E731
    x, corr = pp.refine_loop(solve, csc_to_scipy(n, n, Ap, Ai, Ax), b)
    assert len(corr) < 10 and rel_err(x, x_ref) <= 1e-10, (corr, rel_err(x, x_ref))
    print("matched: %d perturbed, corrections %s" % (len(ref.perturbed), ["%.1e" % c for c in corr]))


def test_argument_checks_need_no_gpu(hip):
    """cs3_set_pivot_perturbation and cs3_get_perturbed refuse bad arguments before they touch a device."""
    import ctypes as C
    lib = hip.lib()
    m, n, Ap, Ai, Ax = pc.matrix("db48")
    assert lib.cs3_set_pivot_perturbation(None, 1e-8) == hip.CS3_ERR_ARG
    count = (C.c_int64 * 1)()
    assert lib.cs3_get_perturbed(None, count, None) == hip.CS3_ERR_ARG
    with hip.Factorization(m, n, Ap, Ai) as F:
        for bad in (-1.0, np.nan, np.inf, -np.inf):
            assert lib.cs3_set_pivot_perturbation(F._h, bad) == hip.CS3_ERR_ARG, bad
        assert lib.cs3_set_pivot_perturbation(F._h, 0.0) == 0 and lib.cs3_set_pivot_perturbation(F._h, 1e-8) == 0
        assert F.set_perturbation(2e-8).perturbation == 2e-8
        assert lib.cs3_get_perturbed(F._h, None, None) == hip.CS3_ERR_ARG
        assert lib.cs3_get_perturbed(F._h, count, None) == hip.CS3_ERR_STATE          # nothing factorised yet
        with pytest.raises(hip.Cs3Error):
            F.perturbed()
        b = np.zeros(n)
        assert lib.cs3_refine(F._h, None, hip._pf(b), hip._pf(b), 1, 1, None) == hip.CS3_ERR_ARG
        assert lib.cs3_refine(F._h, hip._pf(Ax), hip._pf(b), hip._pf(b), 0, 1, None) == hip.CS3_ERR_ARG
        assert lib.cs3_refine(F._h, hip._pf(Ax), hip._pf(b), hip._pf(b), 1, 1, None) == hip.CS3_ERR_STATE
    S = sp.csc_matrix(sp.eye(4) * 2.0)
    with hip.Factorization(4, 4, S.indptr, S.indices, kind=hip.CS3_CHOLESKY) as F:
        assert lib.cs3_set_pivot_perturbation(F._h, 1e-8) == hip.CS3_ERR_ARG             # LU only
    assert hip.perturbation_delta(0.0, Ax, False) == 0.0 and hip.perturbation_delta(False, Ax, True) == 0.0
    eps = np.finfo(np.float64).eps
    assert hip.perturbation_delta(True, Ax, True) == np.sqrt(eps)
    assert hip.perturbation_delta(True, Ax, False) == np.sqrt(eps) * np.abs(Ax).max()
    assert hip.perturbation_delta(3e-7, Ax, False) == 3e-7
