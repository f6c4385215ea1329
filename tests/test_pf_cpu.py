"""The AC power flow without a GPU: the NumPy restatement against central differences, the convergence facts of the
shared cases that the GPU tests rely on, and plan creation through the C ABI (host work only) -- the Jacobian's pattern and
the maps against the restatement, element for element, and every refusal in its documented order."""
import ctypes as C

import numpy as np
import pytest

import pf_cases as pc
import pf_ref as R


@pytest.fixture(scope="module")
def limits(hip):
    return hip.pf_limits()


def all_cases(limits):
    return pc.newton_cases(int(limits.wave_row))


def test_limits(limits):
    assert limits.block == 256                                    # the launch shape the header documents
    assert limits.grid_cap >= 1 and limits.wave_row >= 1


@pytest.mark.parametrize("key", ["planted0", "planted1", "one_sided", "n2", "n3", "two_refs", "star62"])
def test_restated_jacobian_against_central_differences(limits, key):
    case = dict(all_cases(limits))[key]
    P = pc.reference(key, case)["P"]
    vm, va = case["vm0"] + 0.01 * np.cos(np.arange(case["n"])), case["va0"] + 0.1 * np.sin(np.arange(case["n"]))
    J = R.dense_jacobian(P, R.jacobian_ref(P, case["Yz"], vm, va)[0])
    h, npvpq = 1e-6, P["npvpq"]
    for c in range(P["nj"]):
        vp, ap, vn, an = vm.copy(), va.copy(), vm.copy(), va.copy()
        tgt_p, tgt_n = (ap, an) if c < npvpq else (vp, vn)
        tgt_p[P["ubus"][c]] += h
        tgt_n[P["ubus"][c]] -= h
        # F of the restatement is MINUS the mismatch
        col = -(R.mismatch_ref(P, case["Yz"], case["S"], vp, ap)["F"] - R.mismatch_ref(P, case["Yz"], case["S"], vn, an)["F"]) / (2 * h)
        assert np.abs(col - J[:, c]).max() <= 1e-6 * np.abs(J).max(), (key, c)     # truncation h^2 + rounding eps / h, with room


def test_two_bus_jacobian_by_hand(limits):
    case = pc.shape("n2")                                         # bus 0 the reference, bus 1 PQ
    P = pc.reference("n2", case)["P"]
    assert P["nj"] == 2 and list(P["Jp"]) == [0, 2, 4] and list(P["Ji"]) == [0, 1, 0, 1]
    vm, va = np.array([1.01, 0.98]), np.array([0.0, -0.07])
    V = vm * np.exp(1j * va)
    Yd = np.zeros((2, 2), dtype=complex)
    Yd[case["Yi"], np.repeat(np.arange(2), np.diff(case["Yp"]))] = case["Yz"]
    I = Yd @ V
    ds_dth = 1j * V[1] * np.conj(I[1] - Yd[1, 1] * V[1])
    ds_dvm = V[1] * np.conj(Yd[1, 1] * V[1] / vm[1]) + np.conj(I[1]) * V[1] / vm[1]
    want = np.array([[ds_dth.real, ds_dvm.real], [ds_dth.imag, ds_dvm.imag]])
    got = R.dense_jacobian(P, R.jacobian_ref(P, case["Yz"], vm, va)[0])
    assert np.abs(got - want).max() <= 64 * R.EPS * np.abs(want).max()


def test_planted_cases_converge_as_recorded():
    for k, want in enumerate(pc.PLANTED_ITERS):
        case = pc.planted(k)
        ref = pc.reference("planted%d" % k, case)
        assert ref["iters"] == want, (k, ref["run"]["norms"])
        # two more steps reach the floor: the planted voltages to 1e-14 (the fifth case, all PV, by the same reasoning:
        # the error is ||J^-1|| times a mismatch floor of some 1e-14 relative to injections of order 10, on angles below 1)
        run = R.newton_ref(ref["P"], case["Yz"], case["S"], case["vm0"], case["va0"], 0.0, want + 2)
        assert max(np.abs(run["vm"] - case["vm"]).max(), np.abs(run["va"] - case["va"]).max()) <= 1e-14, k


def test_every_newton_case_separates_its_last_two_norms(limits):
    for key, case in all_cases(limits):
        ref = pc.reference(key, case)
        run, k = ref["run"], ref["iters"]
        assert run["flag"] == 0 and k >= 1, key
        assert run["norms"][k - 1] >= 1e3 * run["norms"][k], (key, run["norms"])
        assert run["norms"][k] < ref["tol"] < run["norms"][k - 1]
        if key.startswith("star"):
            assert 4 <= k <= 5, (key, k)
        # pivot_tol = 1e-3 is safe: at EVERY iterate the diagonal stays above 0.9 of its column, but for the all-PQ case,
        # which passes through a norm of 67 and falls to a few hundredths
        again, ratios = pc.newton_with_ratios(ref["P"], case)
        assert again["iters"] == k and len(ratios) == k
        if key == "planted3":
            assert 0.02 <= min(ratios) < 0.9, ratios
        else:
            assert min(ratios) > 0.9, (key, ratios)


def test_the_member_that_does_not_converge():
    case = pc.planted(2)
    P = pc.reference("planted2", case)["P"]
    S = case["S"].copy()
    S[1:] *= 1.3
    run, ratios = pc.newton_with_ratios(P, case, S=S, max_iters=11)
    assert run["flag"] == 1 and run["iters"] == 11
    assert np.isfinite(run["norms"]).all() and min(run["norms"]) > 0.5 and max(run["norms"]) < 100     # it wanders, it does not blow up
    assert min(ratios) >= 0.1, ratios                             # and its pivots stay far above pivot_tol = 1e-3
    S = case["S"].copy()
    S[1:] *= 0.5
    run = R.newton_ref(P, case["Yz"], S, case["vm0"], case["va0"], pc.NOMINAL_TOL, 11)
    assert run["flag"] == 0 and run["iters"] < 11 and run["norms"][-2] >= 1e3 * run["norms"][-1]


def test_the_trio_is_separated_by_one_tolerance():
    t = pc.trio()
    assert all(r["flag"] == 0 for r in t["runs"]) and len({r["iters"] for r in t["runs"]}) >= 2
    assert t["above"] >= 1e3 * t["below"] and t["below"] < t["tol"] < t["above"]
    for b, r in enumerate(t["runs"]):                             # the tolerance of the batch gives every member the count of the nominal one
        again, ratios = pc.newton_with_ratios(t["P"], t["case"], S=t["S"][b], tol=t["tol"], max_iters=20)
        assert again["iters"] == r["iters"] and min(ratios) > 0.9, (b, ratios)


def test_the_late_rejection_case_passes_its_first_factorisation_only():
    case = pc.planted(3)
    run, ratios = pc.newton_with_ratios(pc.reference("planted3", case)["P"], case)
    assert ratios[0] >= 1.8 * pc.LATE_PIVOT_TOL and ratios[1] <= pc.LATE_PIVOT_TOL / 1.8, ratios


def test_a_closed_borrower_is_lent_again(hip):
    case = pc.shape("n3")
    with hip.PowerFlowPlan(case["n"], case["Yp"], case["Yi"], case["pv"], case["pq"]) as plan:
        with plan.factorization as f:
            assert f.info.n == plan.nj
        with pytest.raises(hip.Cs3Error):
            f.info                                                # closing the borrower ended THAT loan and freed nothing ...
        assert plan.factorization is not f and plan.factorization.info.n == plan.nj      # ... and the plan lends its handle again


def test_plan_pattern_and_maps_match_the_restatement(hip, limits):
    for key, case in all_cases(limits):
        P = pc.reference(key, case)["P"]
        with hip.PowerFlowPlan(case["n"], case["Yp"], case["Yi"], case["pv"], case["pq"], batch=3, y_batch=3) as plan:
            Jp, Ji = plan.pattern()
            maps = plan.maps()
            inf = plan.info
        assert np.array_equal(Jp, P["Jp"]) and np.array_equal(Ji, P["Ji"]), key
        for name in ("jpos", "Rp", "Rj", "Rpos", "upos_a", "upos_m"):
            assert np.array_equal(maps[name], P[name]), (key, name)
        rows = np.diff(P["Rp"])[P["upos_a"] >= 0]
        assert (inf.n, inf.nnz_y, inf.npv, inf.npq, inf.nj, inf.nnz_j) == (case["n"], P["nnz"], len(case["pv"]), len(case["pq"]), P["nj"], len(P["Ji"]))
        assert (inf.nref, inf.batch, inf.y_batch) == (case["n"] - len(case["pv"]) - len(case["pq"]), 3, 3)
        assert (inf.rows_lane, inf.rows_wave, inf.max_row) == ((rows <= limits.wave_row).sum(), (rows > limits.wave_row).sum(), rows.max())
    hub = dict(all_cases(limits))["star%d" % limits.wave_row]       # a hub row of wave_row + 1 entries is a wave's
    with hip.PowerFlowPlan(hub["n"], hub["Yp"], hub["Yi"], hub["pv"], hub["pq"]) as plan:
        assert plan.info.rows_wave == 1 and plan.info.max_row == limits.wave_row + 1


def _create(hip, n, Yp, Yi, pv, pq, batch=1, y_batch=1, order=1, out=True):
    L = hip.lib()
    a = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32)
    Yp, Yi, pv, pq = a(Yp), a(Yi), a(pv), a(pq)
    p = C.c_void_p()
    rc = L.cs3_pf_plan_create(n, hip._pi(Yp), hip._pi(Yi), 0 if pv is None else len(pv), hip._pi(pv), 0 if pq is None else len(pq),
                              hip._pi(pq), batch, y_batch, order, C.byref(p) if out else None)
    msg = L.cs3_last_error().decode()
    if rc == 0:
        L.cs3_pf_plan_free(p)
    return rc, msg


def test_refusals_and_their_order(hip):
    # a good 3-bus chain: 0 - 1 - 2
    Yp, Yi = [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2]
    assert _create(hip, 3, Yp, Yi, [1], [2])[0] == 0
    twice = ([0, 3, 6, 8], [0, 1, 1, 0, 1, 2, 1, 2])             # row 1 twice in column 0
    nodiag = ([0, 2, 4, 6], [0, 1, 0, 2, 1, 2])                   # bus 1 without a diagonal
    # every refusal alone, in the documented order; then each with a LATER fault added: the earlier one is reported
    ladder = [
        (dict(Yp=None, Yi=Yi, pv=[1], pq=[2]), "null column pointers"),
        (dict(Yp=[0, 2, 1, 7], Yi=Yi, pv=[1], pq=[2]), "Yp decreases at column 1"),
        (dict(Yp=Yp, Yi=[0, 1, 0, 3, 2, 1, 2], pv=[1], pq=[2]), "row index out of range at entry 3"),
        (dict(Yp=Yp, Yi=Yi, pv=[1], pq=[2], batch=0), "batch must be >= 1"),
        (dict(Yp=Yp, Yi=Yi, pv=[1], pq=[2], batch=4, y_batch=2), "y_batch must be 1 or batch"),
        (dict(Yp=Yp, Yi=Yi, pv=[3], pq=[2]), "pv[0] out of range"),
        (dict(Yp=Yp, Yi=Yi, pv=[1, 1], pq=[2]), "pv[1] repeats an earlier entry"),
        (dict(Yp=Yp, Yi=Yi, pv=[1], pq=[2, 1]), "pq[1] is also in pv"),
        (dict(Yp=Yp, Yi=Yi, pv=[], pq=[]), "npv + npq = 0"),
        (dict(Yp=twice[0], Yi=twice[1], pv=[1], pq=[2]), "row 1 is stored twice in column 0"),
        (dict(Yp=nodiag[0], Yi=nodiag[1], pv=[1], pq=[2]), "pv bus 1 has no stored diagonal entry"),
    ]
    for kw, text in ladder:
        rc, msg = _create(hip, 3, **kw)
        assert rc == hip.CS3_ERR_ARG and msg.startswith("cs3_pf_plan_create: ") and text in msg, (kw, rc, msg)
    assert _create(hip, 3, Yp, Yi, [1], [2], out=False)[0] == hip.CS3_ERR_ARG
    assert _create(hip, 3, [1, 2, 5, 7], Yi, [1], [2])[1].endswith("Yp[0] != 0")
    assert _create(hip, 3, Yp, None, [1], [2])[1].endswith("null row indices")
    assert _create(hip, 3, Yp, Yi, [1], [2], order=2)[1].endswith("order must be 0 (natural) or 1 (AMD)")
    pairs = [
        (dict(Yp=[0, 2, 1, 7], Yi=Yi, pv=[1], pq=[2], batch=0), "Yp decreases"),                  # pattern before batch
        (dict(Yp=Yp, Yi=Yi, pv=[7], pq=[2], batch=0), "batch must be"),                           # batch before bus lists
        (dict(Yp=twice[0], Yi=twice[1], pv=[1], pq=[1]), "pq[0] is also in pv"),                 # bus lists before duplicates
        (dict(Yp=twice[0], Yi=twice[1], pv=[], pq=[]), "npv + npq = 0"),                          # nothing to solve before duplicates
        (dict(Yp=[0, 3, 5, 7], Yi=[0, 1, 1, 0, 2, 1, 2], pv=[1], pq=[2]), "stored twice"),        # duplicates before the diagonal
    ]
    for kw, text in pairs:
        rc, msg = _create(hip, 3, **kw)
        assert rc == hip.CS3_ERR_ARG and text in msg, (kw, rc, msg)


def test_driver_argument_checks_need_no_device(hip):
    case = pc.shape("n3")
    L = hip.lib()
    one = np.ones(8)
    bad = C.c_void_p(0x10000)                                     # never followed: every check comes before device work
    with hip.PowerFlowPlan(case["n"], case["Yp"], case["Yi"], case["pv"], case["pq"]) as plan:
        call = lambda p, y, tol, mi, re: L.cs3_pf_solve_dev(p, y, bad, bad, bad, C.c_double(tol), mi, re, C.c_double(1e-3), None, None, None, None)
        ladder = [((None, bad, 1e-8, 5, 1), "null argument"), ((plan._p, None, 1e-8, 5, 1), "null argument"),
                  ((plan._p, bad, -1.0, -1, 0), "tol must be finite and >= 0"), ((plan._p, bad, float("nan"), 5, 1), "tol must be finite and >= 0"),
                  ((plan._p, bad, float("inf"), 5, 1), "tol must be finite and >= 0"),
                  ((plan._p, bad, 1e-8, -1, 0), "max_iters must be >= 0"), ((plan._p, bad, 1e-8, 0, 0), "refactor_every must be >= 1")]
        for args, text in ladder:
            assert call(*args) == hip.CS3_ERR_ARG and L.cs3_last_error().decode() == "cs3_pf_solve_dev: " + text, args
        assert L.cs3_pf_solve(plan._p, hip._pf(one), hip._pf(one), hip._pf(one), hip._pf(one), C.c_double(1e-8), 5, 0, C.c_double(1e-3),
                              None, None, None) == hip.CS3_ERR_ARG
        h = C.c_void_p()
        assert L.cs3_pf_handle(plan._p, C.byref(h)) == 0 and h.value
        assert plan.factorization.info.n == plan.nj and plan.factorization.info.batch == 1
        f = plan.factorization
    with pytest.raises(hip.Cs3Error):
        f.info                                                    # the plan is closed: the borrower is empty
