"""The AC state estimation on the device (include/csparse3_amd.h, "AC state estimation") against the NumPy restatement
(se_ref.py) on the shared cases (se_cases.py, whose conditioning and convergence facts test_se_cpu.py asserts).

Kernels: per entry |dev - ref| <= (d + 16) eps sum |terms| (+ eps |z_i| for a residual), derived in se_ref.py.  Device and
NumPy sincos differ in the last bits: no bit test against the restatement there.  The exact invariants compare the device
with itself, bit for bit: the three copies of H, the tree behind J, the gradient's order of summation, the driver against
a hand-driven loop, one run against the next and the host forms against the device forms."""
import gc

import numpy as np
import pytest

import quad_ref
import se_cases as sc
import se_ref as R

pytestmark = pytest.mark.gpu


def _plan(hip, case):
    return hip.StateEstPlan(case["n"], case["Yp"], case["Yi"], case["ref"], case["end_from"], case["end_to"], case["kind"], case["where"])


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return torch.from_numpy(a.reshape(-1).copy()).cuda()


def _empty(count):
    import torch
    return torch.empty(max(int(count), 1), dtype=torch.float64, device="cuda")


class _Device:
    """The arrays of a case on the device, and the pointers in the order the *_dev calls take them."""

    def __init__(self, case, vm=None, va=None):
        self.Yz, self.Ye, self.z, self.w = (_dev(case[k]) for k in ("Yz", "Ye", "z", "w"))
        self.vm, self.va = _dev(case["vm0"] if vm is None else vm), _dev(case["va0"] if va is None else va)

    @property
    def args(self):
        return tuple(t.data_ptr() for t in (self.Yz, self.Ye, self.z, self.w, self.vm, self.va))

    def voltages(self):
        return self.vm.cpu().numpy(), self.va.cpu().numpy()


@pytest.mark.parametrize("key", sc.EVERY)
def test_kernels_against_the_restatement(gpu, key):
    case, P = sc.case_of(key), sc.plan_of(key)
    vm, va = sc.moved_voltages(case)
    with _plan(gpu, case) as plan:
        r, J = plan.measure(case["Yz"], case["Ye"], case["z"], case["w"], vm, va)
        Hr, Hc, WHc = plan.jacobian(case["Yz"], case["Ye"], case["w"], vm, va)
    ref = R.measure_ref(P, case["Yz"], case["Ye"], case["z"], vm, va)
    excess = np.abs(r - ref["r"]) - ref["bound"]
    assert excess.max() <= 0, (key, int(excess.argmax()), excess.max())
    Href, Hbound = R.jacobian_ref(P, case["Yz"], case["Ye"], vm, va, ref)
    excess = np.abs(Hr - Href) - Hbound
    print("%s: nnz_h=%d worst |H - ref| / bound %.3f" % (key, P["nnz_h"], (np.abs(Hr - Href)[Hbound > 0] / Hbound[Hbound > 0]).max()))
    assert excess.max() <= 0, (key, int(excess.argmax()), excess.max())
    assert np.array_equal(Hc[P["cpos"]], Hr)                           # the three copies of one value, bit for bit
    assert np.array_equal(WHc, case["w"][P["Hi"]] * Hc)
    assert J == R.cost_ref(case["w"], r)                               # the tree, on the device's own r


@pytest.mark.parametrize("key", sc.STARS + ["star_col63", "star_col64", "star_col65", "chain_m255", "chain_m256", "chain_m257",
                                            "chain_nnz255", "chain_nnz256", "chain_nnz257", "ac_large", "grid_edge"])
def test_the_gradient_bit_for_bit(gpu, key):
    """k_se_gradient against gradient_ref fed the device's own Hc and w r: lane columns, wave columns, both sides of wave_col."""
    case, P = sc.case_of(key), sc.plan_of(key)
    vm, va = sc.moved_voltages(case)
    D = _Device(case, vm, va)
    r, Hc, g = _empty(P["m"]), _empty(P["nnz_h"]), _empty(P["ns"])
    with _plan(gpu, case) as plan:
        plan.measure_dev(*D.args, r_ptr=r.data_ptr())
        plan.jacobian_dev(D.Yz.data_ptr(), D.Ye.data_ptr(), D.w.data_ptr(), D.vm.data_ptr(), D.va.data_ptr(), hc_ptr=Hc.data_ptr())
        wr = D.w * r
        plan.gradient_dev(Hc.data_ptr(), wr.data_ptr(), g.data_ptr())
        mine = g.cpu().numpy()
        plan.gradient_dev(Hc.data_ptr(), plan.residuals_dev()[1], g.data_ptr())        # the plan's own w r: the same bits
        assert np.array_equal(g.cpu().numpy(), mine)
    want = R.gradient_ref(P, Hc.cpu().numpy()[:P["nnz_h"]], wr.cpu().numpy(), sc.limits()["wave_col"])
    assert np.array_equal(mine, want), (key, np.flatnonzero(mine != want)[:8])


@pytest.fixture(scope="module")
def runs(gpu):
    """The driver from the flat start on every solved case, once, through the device form."""
    out = {}
    for key in sc.SOLVED:
        case = sc.case_of(key)
        D = _Device(case)
        with _plan(gpu, case) as plan:
            info = plan.solve_dev(*D.args, tol=sc.TOL, max_iters=sc.MAX_ITERS)
        out[key] = (D.voltages(), info)
    return out


@pytest.mark.parametrize("key", sc.SOLVED)
def test_the_driver_against_the_restatement(gpu, runs, key):
    case, P, ref = sc.case_of(key), sc.plan_of(key), sc.reference(key)
    (vm, va), info = runs[key]
    assert (info["iters"], info["flag"]) == (ref["iters"], ref["flag"]) == (ref["iters"], 0), (key, info, ref["steps"])
    x = R.state_of(P, vm, va)
    if key != "noisy":
        err = np.abs(x - R.state_of(P, case["vm"], case["va"])).max()
    else:
        err = np.abs(x - R.state_of(P, ref["vm"], ref["va"])).max()
    print("%s: iters %d step %.2e error %.2e" % (key, info["iters"], info["step"], err))
    assert err <= sc.TOL, (key, err)
    assert info["step"] <= sc.TOL and abs(info["step"] - ref["step"]) <= 1e-3 * sc.TOL
    assert np.array_equal(va[case["ref"]], case["va0"][case["ref"]])   # a reference angle never moves
    assert abs(info["J"] - ref["J"]) <= 1e-6 * abs(ref["J"]) + 1e-18


@pytest.mark.parametrize("key", ["ac169", "noisy", "star_col65", "star_row64", "star_row65", "star_row129", "two_refs", "no_ends"])
def test_the_driver_adds_nothing(gpu, runs, key):
    """measure_dev, jacobian_dev, gradient_dev, SpgemmPlan.values_dev and factor_solve_dev on the lent handle, driven by
    hand for as many steps as the driver took: its voltages, bit for bit."""
    import torch
    case, P = sc.case_of(key), sc.plan_of(key)
    (vm, va), info = runs[key]
    D = _Device(case)
    m, ns, na = P["m"], P["ns"], P["na"]
    nonref = torch.from_numpy(P["sbus"][:na].astype(np.int64)).cuda()
    Hc, WHc, g = _empty(P["nnz_h"]), _empty(P["nnz_h"]), _empty(ns)
    with _plan(gpu, case) as plan, gpu.SpgemmPlan(m, ns, P["Hp"], P["Hi"], m, ns, P["Hp"], P["Hi"], transpose_a=True) as gain:
        fz = plan.factorization
        Gp, Gi = plan.gain_pattern()
        assert np.array_equal(Gp, gain.pattern()[0]) and np.array_equal(Gi, gain.pattern()[1])
        Gx = _empty(len(Gi))
        for _ in range(info["iters"]):
            plan.measure_dev(*D.args)
            plan.jacobian_dev(D.Yz.data_ptr(), D.Ye.data_ptr(), D.w.data_ptr(), D.vm.data_ptr(), D.va.data_ptr(), hc_ptr=Hc.data_ptr(),
                              whc_ptr=WHc.data_ptr())
            plan.gradient_dev(Hc.data_ptr(), plan.residuals_dev()[1], g.data_ptr())
            gain.values_dev(Hc.data_ptr(), WHc.data_ptr(), Gx.data_ptr())
            fz.factor_solve_dev(Gx.data_ptr(), g.data_ptr(), k=1, tol=0.0)
            fz.factor_status()
            D.va[nonref] += g[:na]
            D.vm += g[na:ns]
        step = float(g[:ns].abs().max())
    assert step == info["step"]
    got_vm, got_va = D.voltages()
    assert np.array_equal(got_vm, vm) and np.array_equal(got_va, va)


@pytest.mark.parametrize("key", ["ac442", "noisy", "both_ends"])
def test_runs_repeat_and_the_host_form_is_the_device_form(gpu, runs, key):
    case = sc.case_of(key)
    (vm, va), info = runs[key]
    with _plan(gpu, case) as plan:
        for _ in range(2):                                             # the same plan twice: nothing is left over from a run
            D = _Device(case)
            again = plan.solve_dev(*D.args, tol=sc.TOL, max_iters=sc.MAX_ITERS)
            assert again == info
            assert all(np.array_equal(a, b) for a, b in zip(D.voltages(), (vm, va)))
        hvm, hva, hinfo = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=sc.MAX_ITERS)
        assert hinfo == info and np.array_equal(hvm, vm) and np.array_equal(hva, va)
        # measure and jacobian: host arrays against device arrays
        r, J = plan.measure(case["Yz"], case["Ye"], case["z"], case["w"], vm, va)
        D = _Device(case, vm, va)
        dr, dJ, dH = _empty(plan.m), _empty(1), [_empty(plan.nnz_h) for _ in range(3)]
        plan.measure_dev(*D.args, r_ptr=dr.data_ptr(), j_ptr=dJ.data_ptr())
        assert np.array_equal(dr.cpu().numpy(), r) and float(dJ[0]) == J == info["J"]
        plan.jacobian_dev(D.Yz.data_ptr(), D.Ye.data_ptr(), D.w.data_ptr(), D.vm.data_ptr(), D.va.data_ptr(), *[t.data_ptr() for t in dH])
        for got, want in zip(dH, plan.jacobian(case["Yz"], case["Ye"], case["w"], vm, va)):
            assert np.array_equal(got.cpu().numpy(), want)


def test_the_flags(gpu):
    case, P = sc.case_of("ac416"), sc.plan_of("ac416")
    with _plan(gpu, case) as plan:
        vm, va, info = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=0)
        r, J = plan.measure(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"])
        assert info == dict(iters=0, step=0.0, J=J, flag=1)
        assert np.array_equal(vm, case["vm0"]) and np.array_equal(va, case["va0"])
        vm, va, info = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=1)
        first = sc.reference("ac416")["steps"][0]
        assert (info["iters"], info["flag"]) == (1, 1) and abs(info["step"] - first) <= 1e-9 * first
        z = case["z"].copy()
        z[3] = np.nan
        vm, va, info = plan.solve(case["Yz"], case["Ye"], z, case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=sc.MAX_ITERS)
        assert (info["iters"], info["flag"]) == (1, 2) and np.isnan(info["step"]) and np.isnan(info["J"])      # CS3_OK: no exception
        for bad in (dict(tol=-1.0), dict(tol=np.inf), dict(tol=np.nan), dict(max_iters=-1)):
            with pytest.raises(gpu.Cs3Error) as err:
                plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], **bad)
            assert err.value.code == gpu.CS3_ERR_ARG
        # the plan still solves after all that
        vm, va, info = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=sc.MAX_ITERS)
        assert info["flag"] == 0 and np.abs(R.state_of(P, vm, va) - R.state_of(P, case["vm"], case["va"])).max() <= sc.TOL


def test_an_unobservable_state_is_not_positive_definite(gpu):
    case = sc.case_of("unobservable")
    D = _Device(case)
    with _plan(gpu, case) as plan:
        with pytest.raises(gpu.NotPositiveDefinite) as err:
            plan.solve_dev(*D.args, tol=sc.TOL, max_iters=sc.MAX_ITERS)
        assert err.value.code == gpu.CS3_ERR_NOT_SPD
        vm, va = D.voltages()
        assert np.array_equal(vm, case["vm0"]) and np.array_equal(va, case["va0"])          # k_se_update applied nothing
        # through the C ABI: iters and step of the completed iterations (none), flag 1, J not written
        import ctypes as C
        iters, step, J, flag = C.c_int32(-7), C.c_double(-7.0), C.c_double(-7.0), C.c_int32(-7)
        rc = gpu.lib().cs3_se_solve_dev(plan._p, *[C.c_void_p(a) for a in D.args], sc.TOL, sc.MAX_ITERS, C.byref(iters), C.byref(step),
                                        C.byref(J), C.byref(flag), None)
        assert (rc, iters.value, step.value, J.value, flag.value) == (gpu.CS3_ERR_NOT_SPD, 0, 0.0, -7.0, 1)
        with pytest.raises(gpu.NotPositiveDefinite):
            plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"])


def test_bad_data_finds_the_planted_row(gpu):
    case, bad = sc.bad_data_case()
    P = sc.plan_of("noisy")
    m = P["m"]
    with _plan(gpu, case) as plan:
        vm, va, info = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=sc.MAX_ITERS)
        assert info["flag"] == 0
        out = plan.bad_data(case["Yz"], case["Ye"], case["z"], case["w"], vm, va, crit_tol=sc.CRIT_TOL)
        Hr, Hc, WHc = plan.jacobian(case["Yz"], case["Ye"], case["w"], vm, va)
        r, J = plan.measure(case["Yz"], case["Ye"], case["z"], case["w"], vm, va)
        assert out["worst_row"] == bad and out["worst"] == out["rn"][bad] == out["rn"].max() and out["worst"] > 5.0
        assert out["J"] == J == info["J"] and out["critical"] == 0
        # against the dense Omega at the device's state, under the bound policy of test_gpu_quad.py
        bd = R.baddata_ref(P, Hr, case["w"], r)
        assert bd["cond"] <= quad_ref.COND_MAX
        assert (np.abs(out["t"] - bd["t"]) <= quad_ref.BOUND * bd["scale"]).all()
        # omega = 1/w - t carries t's error and one rounding; rn = |r| / sqrt(omega) moves by rn d(omega) / (2 omega) to first
        # order: (1 + x)^(-1/2) - 1 lies within |x| (1/2 + 3/8 |x| + ...) < |x| for |x| = BOUND * scale / omega <= 1e-3, which
        # the reference's own numbers are held to below; 4 eps for the division, the root and omega's own rounding.  r is the
        # device's own on both sides.
        slack = quad_ref.BOUND * bd["scale"]
        assert (np.abs(out["omega"] - bd["omega"]) <= slack + 2 * R.EPS / case["w"]).all()       # (the division and the difference round)
        assert (slack <= 1e-3 * bd["omega"]).all()
        assert (np.abs(out["rn"] - bd["rn"]) <= bd["rn"] * (slack / bd["omega"] + 4 * R.EPS)).all()
        # and omega, rn and the summary are the restated functions of the device's own t, bit for bit
        omega_want, rn_want, summary_want = quad_ref.restated_normres(out["t"], case["w"], r, sc.CRIT_TOL, gpu.quad_limits())
        assert np.array_equal(out["omega"], omega_want) and np.array_equal(out["rn"], rn_want)
        assert [out["worst"], float(out["worst_row"]), out["J"], float(out["critical"])] == summary_want.tolist()
        # the device form, and a direct normalized_residuals_dev on the lent handle with the plan's own Hr: the same bits
        D = _Device(case, vm, va)
        summary, t, omega, rn = _empty(4), _empty(m), _empty(m), _empty(m)
        plan.bad_data_dev(*D.args, sc.CRIT_TOL, summary.data_ptr(), t.data_ptr(), omega.data_ptr(), rn.data_ptr())
        fz = plan.factorization
        fz.factor_status()
        for got, want in ((t, out["t"]), (omega, out["omega"]), (rn, out["rn"])):
            assert np.array_equal(got.cpu().numpy(), want)
        assert summary.cpu().numpy().tolist() == [out["worst"], float(bad), J, 0.0]
        with fz.quad_plan((m, P["Hrp"], P["Hrj"])) as rows:
            dHr, dr = _dev(Hr), _empty(m)
            plan.measure_dev(*D.args, r_ptr=dr.data_ptr())
            s2, t2, o2, r2 = _empty(4), _empty(m), _empty(m), _empty(m)
            fz.normalized_residuals_dev(rows, dHr.data_ptr(), D.w.data_ptr(), dr.data_ptr(), sc.CRIT_TOL, s2.data_ptr(), t2.data_ptr(),
                                        o2.data_ptr(), r2.data_ptr())
            for got, want in ((t2, t), (o2, omega), (r2, rn), (s2, summary)):
                assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
        # the values of G that were factorised, from the public product: G is what the restatement says
        with gpu.SpgemmPlan(m, P["ns"], P["Hp"], P["Hi"], m, P["ns"], P["Hp"], P["Hi"], transpose_a=True) as gain:
            Gx = gain.values(Hc, WHc)
        Gp, Gi = plan.gain_pattern()
        G = np.zeros((P["ns"], P["ns"]))
        G[Gi, np.repeat(np.arange(P["ns"]), np.diff(Gp))] = Gx
        want = R.gain_ref(P, Hr, case["w"])[1]
        assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()


def test_the_lent_handle_is_a_full_handle_and_goes_with_the_plan(gpu):
    case, P = sc.case_of("ac169"), sc.plan_of("ac169")
    gc.collect()
    live0 = gpu.debug_live_device_buffers()
    plan = _plan(gpu, case)
    fz = plan.factorization
    assert fz.kind == gpu.CS3_CHOLESKY and plan.info.nnz_g == len(plan.gain_pattern()[1]) > 0
    vm, va, info = plan.solve(case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], tol=sc.TOL, max_iters=sc.MAX_ITERS)
    assert gpu.debug_live_device_buffers() > live0
    # the factors are those of the last gain matrix the driver built: at the iterate before the converged one, which lies
    # within the last step (<= 1e-8) of it
    Hr, Hc, WHc = plan.jacobian(case["Yz"], case["Ye"], case["w"], vm, va)
    with gpu.SpgemmPlan(P["m"], P["ns"], P["Hp"], P["Hi"], P["m"], P["ns"], P["Hp"], P["Hi"], transpose_a=True) as gain:
        Gx = gain.values(Hc, WHc)
    G = R.gain_ref(P, Hr, case["w"])[1]
    cond, inv_norm = fz.condest(Gx)
    exact = np.abs(np.linalg.inv(G)).sum(axis=0).max()
    assert 0.3 * exact <= np.ravel(inv_norm)[0] <= 1.01 * exact           # Hager's estimate is a lower bound of ||G^-1||_1, seldom far below
    sign, logabs = fz.slogdet()
    s_ref, l_ref = np.linalg.slogdet(G)
    assert np.ravel(sign)[0] == s_ref == 1.0 and abs(np.ravel(logabs)[0] - l_ref) <= 1e-6 * abs(l_ref)
    plan.close()
    gc.collect()
    assert gpu.debug_live_device_buffers() == live0
    with pytest.raises(gpu.Cs3Error):
        fz.slogdet()
    with pytest.raises(gpu.Cs3Error):
        fz.info
    fz.close()                                                           # frees nothing: the handle went with the plan
    assert gpu.debug_live_device_buffers() == live0


def test_the_state_estimator_class(gpu):
    from csparse3_amd.csc import CscMat
    from csparse3_amd.stateest import StateEstimator
    case, P, ref = sc.case_of("ac442"), sc.plan_of("ac442"), sc.reference("ac442")
    n = case["n"]
    Y = CscMat(n, n, indptr=case["Yp"], indices=case["Yi"], data=case["Yz"])
    V0 = case["vm0"] * np.exp(1j * case["va0"])
    for net in (Y, (n, case["Yp"], case["Yi"])):
        with StateEstimator(net, case["ref"], (case["end_from"], case["end_to"]), (case["kind"], case["where"])) as se:
            V, info = se.solve(None if net is Y else case["Yz"], case["Ye"], case["z"], case["w"], V0)
            assert (info["iters"], info["flag"]) == (ref["iters"], 0)
            assert np.abs(V - case["vm"] * np.exp(1j * case["va"])).max() <= 2 * sc.TOL
            r, J = se.residuals(case["Yz"], case["Ye"], case["z"], case["w"], V)
            assert np.abs(r).max() <= 1e-6 and J == np.float64(J) >= 0
            rn, bd = se.bad_data(case["Yz"], case["Ye"], case["z"], case["w"], V)
            assert rn.shape == (P["m"],) and bd["worst"] == rn[bd["worst_row"]] and (bd["omega"] > 0).all()
            assert se.factorization.slogdet()[0][0] == 1.0
