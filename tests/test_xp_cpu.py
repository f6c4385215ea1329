"""Extra-precise refinement, what the CPU can say: the NumPy restatement (tests/xp_ref.py) with SuperLU as the inner solver
on the cases of tests/xp_cases.py against the 80-digit solutions of tests/golden/xp_refs.npz, and the argument checks of
the C ABI, which need no device.

Measured with this file (printed by the tests): cond_1 of the chains 1.3e7, 8.4e9, 6.7e11, 5.3e13, 4.3e15, 2.7e17; the
restatement needs 2, 2, 3, 4, 8 corrections on the first five and returns the correctly rounded solution (forward error 0
against the fixture's head); ten plain rounds leave 6e-9 .. 2e-3 on the five with cond >= 1e9; (2, 20) is still iterating
after 10 (rate 0.40, true error 4.1e-5, ferr 2.4e-4)."""
import ctypes as C
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest

import xp_cases as xc
import xp_ref
from csparse3_amd import csc, csc_hip

EPS = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xp_refs.npz")


@pytest.fixture(scope="module")
def refs():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return xc.refinement_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """The restatement from x0 = solve(b) with SuperLU, once per case."""
    out = {}
    for name, case in cases.items():
        solve = xc.superlu_solver(case)
        out[name] = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, case.b, solve(case.b), 10, case.trans)
    return out


def _ferr_true(x, xh):
    return float(np.abs(x - xh).max() / np.abs(xh).max())


def test_product_error_is_exact():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(200) * 2.0 ** rng.integers(-30, 30, 200)
    x = rng.standard_normal(200) * 2.0 ** rng.integers(-30, 30, 200)
    p, e = xp_ref.two_prod(a, x)
    for ai, xi, pi, ei in zip(a, x, p, e):
        assert Fraction(float(ai)) * Fraction(float(xi)) - Fraction(float(pi)) == Fraction(float(ei))
    s, e = xp_ref.two_sum(a, x)
    for ai, xi, si, ei in zip(a, x, s, e):
        assert Fraction(float(ai)) + Fraction(float(xi)) - Fraction(float(si)) == Fraction(float(ei))


def test_doubled_residual_against_exact_arithmetic():
    """r of the restatement is within one rounding of the exact residual of x + xt where plain summation is not."""
    case = xc.chain(3, 15)
    rng = np.random.default_rng(1)
    x = np.linalg.solve(xc.dense(case), case.b)
    xt = x * 2.0 ** -54 * rng.standard_normal(case.n)
    r, s = xp_ref.resid_xp(case.n, case.Ap, case.Ai, case.Ax, case.b, x, xt)
    A = xc.dense(case)
    for i in range(case.n):
        exact = Fraction(float(case.b[i])) - sum(Fraction(float(A[i, j])) * (Fraction(float(x[j])) + Fraction(float(xt[j])))
                                                 for j in range(case.n) if A[i, j] != 0.0)
        # doubled accumulation: an error of a few eps^2 relative to s_i, and one final rounding
        assert abs(Fraction(float(r[i])) - exact) <= abs(exact) * Fraction(EPS) + Fraction(float(s[i])) * Fraction(EPS) ** 2 * 16
        assert abs(s[i] - (abs(case.b[i]) + np.abs(A[i]) @ np.abs(x))) <= 8 * EPS * s[i]


def test_converged_cases(cases, refs, restated):
    for name, case in cases.items():
        cond = float(refs[name + "_cond"])
        if name == "hopeless" or cond >= 2.0 ** 52:
            continue
        res = restated[name]
        err = _ferr_true(res["x"], refs[name + "_xh"])
        print("%-13s cond %.1e iters %d flag %d rate %.2e ferr %.2e true %.2e" % (name, cond, res["iters"], res["flag"],
                                                                                  res["rate"], res["ferr"], err))
        assert res["flag"] == 1 and res["iters"] <= 10
        assert err <= EPS
        assert res["ferr"] >= err and res["ferr"] == EPS


@pytest.mark.parametrize("name", ["chain_4_11", "chain_3_13", "chain_3_15", "chain_3_17", "chain_4_11_t"])
def test_plain_rounds_do_not_get_there(cases, refs, name):
    case = cases[name]
    assert float(refs[name + "_cond"]) >= 1e9
    solve = xc.superlu_solver(case)
    x = xp_ref.plain_rounds(solve, case.n, case.Ap, case.Ai, case.Ax, case.b, solve(case.b), 10, case.trans)
    err = _ferr_true(x, refs[name + "_xh"])
    print("%s: ten plain rounds leave %.2e" % (name, err))
    assert err > 2.0 ** 10 * EPS


def test_beyond_one_over_eps_still_iterating_with_a_bound_that_holds(refs, restated):
    res = restated["chain_2_20"]
    err = _ferr_true(res["x"], refs["chain_2_20_xh"])
    print("chain_2_20: cond %.1e iters %d flag %d rate %.2e ferr %.2e true %.2e" % (float(refs["chain_2_20_cond"]), res["iters"],
                                                                                 res["flag"], res["rate"], res["ferr"], err))
    assert float(refs["chain_2_20_cond"]) >= 2.0 ** 52
    assert res["flag"] == 0 and res["iters"] == 10
    assert np.isfinite(res["ferr"]) and res["ferr"] >= err


def test_edge_shapes_do_not_depend_on_the_inner_solvers_rounding(cases):
    """(3, 17) and (2, 20) sit at 1 / eps: their seeds were chosen so that five arithmetics of the inner solver agree."""
    for name, want_flag in (("chain_3_17", 1), ("chain_2_20", 0)):
        case = cases[name]
        solvers = [xc.superlu_solver(case)] + [xc.tridiagonal_solver(case, recip, fma) for recip in (False, True)
                                               for fma in (False, True)]
        got = [xp_ref.refine_xp(s, case.n, case.Ap, case.Ai, case.Ax, case.b, s(case.b), 10) for s in solvers]
        print(name, [(r["iters"], r["flag"], "%.1e" % r["rate"]) for r in got])
        assert [r["flag"] for r in got] == [want_flag] * 5
        if want_flag == 1:
            assert max(r["iters"] for r in got) <= 8
        else:
            assert all(0.05 <= r["rate"] <= 0.45 for r in got)


def test_hopeless_pair_stalls(restated):
    res = restated["hopeless"]
    assert res["flag"] == 2 and res["ferr"] == np.inf and res["rate"] >= 1.0


def test_special_cases_of_the_restatement():
    case = xc.chain(4, 8)
    solve = xc.superlu_solver(case)
    x0 = solve(case.b)
    none = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, case.b, x0, 0)
    assert none["iters"] == 0 and none["flag"] == 0 and none["ferr"] == np.inf and np.array_equal(none["x"], x0)
    zero = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, np.zeros(case.n), np.zeros(case.n))
    assert (zero["iters"], zero["flag"], zero["ferr"], zero["berr"]) == (1, 1, 0.0, 0.0) and not zero["x"].any()
    b = case.b.copy()
    b[3] = np.nan
    bad = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, b, x0)
    assert bad["flag"] == 3 and bad["iters"] == 0 and np.array_equal(bad["x"], x0)


def test_fixture_inputs_regenerate_bit_for_bit(cases, refs):
    for name, case in cases.items():
        for key in ("Ap", "Ai", "Ax", "Ax0", "b"):
            want, got = refs["%s_%s" % (name, key)], getattr(case, key)
            assert want.dtype == got.dtype and want.tobytes() == got.tobytes(), (name, key)
        head, tail = refs[name + "_xh"], refs[name + "_xt"]
        assert (np.abs(tail) <= EPS * np.abs(head)).all()
    assert len(cases) == 13


# ---- the C ABI without a device ---------------------------------------------------------------------------------------

def test_limits():
    lim = csc_hip.refine_xp_limits()
    assert lim.eps == EPS and lim.stall_ratio == 0.5 and lim.max_iters_default == 10
    assert lim.block >= 64 and lim.block % 64 == 0 and lim.grid_cap >= 1 and lim.maxima_grid_cap >= 1
    assert csc_hip.lib().cs3_refine_xp_limits(None) == csc_hip.CS3_ERR_ARG


def _p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _refine(h, Ax, B, X, k=1, max_iters=10, trans=0):
    return csc_hip.lib().cs3_refine_xp(h, _p(Ax), _p(B), _p(X), None, k, max_iters, trans, None, None, None, None, None)


def _residual(h, Ax, B, X, R, k=1):
    return csc_hip.lib().cs3_residual_xp(h, _p(Ax), _p(B), _p(X), None, _p(R), None, k, 0)


def test_argument_checks_need_no_device():
    case = xc.chain(4, 8)
    n, Ap, Ai, Ax = case.n, case.Ap, case.Ai, case.Ax
    b, x, r = case.b.copy(), np.zeros(n), np.zeros(n)
    ARG, STATE = csc_hip.CS3_ERR_ARG, csc_hip.CS3_ERR_STATE
    with csc_hip.Factorization(n, n, Ap, Ai, order=csc_hip.ORDER_NATURAL) as F:
        h = F._h
        assert _refine(None, Ax, b, x) == ARG
        assert _refine(h, None, b, x) == ARG
        assert _refine(h, Ax, None, x) == ARG
        assert _refine(h, Ax, b, None) == ARG
        assert _refine(h, Ax, b, x, k=0) == ARG
        assert _refine(h, Ax, b, x, max_iters=-1) == ARG
        # the order: a bad argument is reported before the missing factorisation
        assert _refine(h, Ax, b, x, k=0, max_iters=0) == ARG
        assert _refine(h, Ax, b, x) == STATE
        assert _refine(h, Ax, b, x, max_iters=0, trans=1) == STATE
        assert "factorisation" in csc_hip.lib().cs3_last_error().decode()
        dev = csc_hip.lib().cs3_refine_xp_dev
        assert dev(h, None, None, None, None, 1, 10, 0, None, None, None, None, None, None) == ARG
        assert dev(h, 8, 8, 8, None, 1, -1, 0, None, None, None, None, None, None) == ARG
        assert dev(h, 8, 8, 8, None, 1, 10, 0, None, None, None, None, None, None) == STATE
        assert _residual(None, Ax, b, x, r) == ARG
        assert _residual(h, None, b, x, r) == ARG
        assert _residual(h, Ax, None, x, r) == ARG
        assert _residual(h, Ax, b, None, r) == ARG
        assert _residual(h, Ax, b, x, None) == ARG
        assert _residual(h, Ax, b, x, r, k=0) == ARG
        rdev = csc_hip.lib().cs3_residual_xp_dev
        assert rdev(h, None, None, None, None, None, None, 1, 0, None) == ARG
    with csc_hip.Factorization(n, n, Ap, Ai, schur=[0, 1]) as S:
        assert _refine(S._h, Ax, b, x) == ARG
        assert "Schur" in csc_hip.lib().cs3_last_error().decode()
        assert _residual(S._h, Ax, b, x, r) == ARG


def test_extra_is_a_third_value_and_the_default_stays():
    for fn in (csc_hip.Factorization.solve_refined, csc_hip.csc_lusol_f, csc.CscMat.solve, csc.lusol):
        assert inspect.signature(fn).parameters["refine"].default == "stationary", fn
    with pytest.raises(AssertionError):
        csc_hip.Factorization.solve_refined(None, None, None, refine="more")
