"""The AC power flow on the device (include/csparse3_amd.h, "AC power flow") against the NumPy restatement (pf_ref.py) on
the shared cases (pf_cases.py, whose convergence facts test_pf_cpu.py asserts).

Kernels: per entry |dev - ref| <= (d + 16) eps sum |terms| (+ eps |S_i| for the mismatch), d the stored entries of the
row (1 for an off-diagonal Jacobian entry): a term is three roundings deep plus 2 ulp each from sin and cos, under 8 eps,
a sum of d terms adds d - 1, and the bound doubles that.  Device and NumPy sincos differ in the last bits: no bit test
against the restatement.  The exact invariants compare the device with itself, bit for bit."""
import gc

import numpy as np
import pytest

import pf_cases as pc
import pf_ref as R

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def limits(hip):
    return hip.pf_limits()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64).copy()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return torch.from_numpy(a.reshape(-1).copy()).cuda()


def _plan(hip, case, **kw):
    return hip.PowerFlowPlan(case["n"], case["Yp"], case["Yi"], case["pv"], case["pq"], **kw)


KERNEL_KEYS = ["planted0", "planted1", "planted2", "planted3", "planted4", "star62", "star63", "star64", "star65", "star129",
               "star130", "one_sided"] + pc.SHAPES + ["grid_edge"]


def _case(limits, key):
    assert pc.star_sizes(int(limits.wave_row)) == [62, 63, 64, 65, 129, 130]      # the keys above name hub rows around the limit
    return pc.grid_edge(limits) if key == "grid_edge" else dict(pc.newton_cases(int(limits.wave_row)))[key]


@pytest.mark.parametrize("key", KERNEL_KEYS)
def test_kernels_against_the_restatement(gpu, limits, key):
    case = _case(limits, key)
    n = case["n"]
    P = R.plan_ref(n, case["Yp"], case["Yi"], case["pv"], case["pq"]) if key == "grid_edge" else pc.reference(key, case)["P"]
    # two scenarios: the start, and voltages moved off it
    vm = np.stack([case["vm0"], case["vm0"] + 0.01 * np.cos(np.arange(n))])
    va = np.stack([case["va0"], case["va0"] + 0.1 * np.sin(np.arange(n))])
    S = np.stack([case["S"], case["S"] * 1.1])
    with _plan(gpu, case, batch=2) as plan:
        F, norm = plan.mismatch(case["Yz"], S, vm, va)
        Jx = plan.jacobian(case["Yz"], vm, va)
    for b in range(2):
        ref = R.mismatch_ref(P, case["Yz"], S[b], vm[b], va[b])
        excess = np.abs(F[b] - ref["F"]) - ref["bound"]
        assert excess.max() <= 0, (key, b, int(excess.argmax()), excess.max())
        assert norm[b] == np.abs(F[b]).max()                             # the integer max of the bit patterns, exactly
        Jref, Jbound = R.jacobian_ref(P, case["Yz"], vm[b], va[b], ref)
        excess = np.abs(Jx[b] - Jref) - Jbound
        assert excess.max() <= 0, (key, b, int(excess.argmax()), excess.max())


@pytest.fixture(scope="module")
def trio(gpu):
    """pf_cases.trio() -- three scenarios of planted2 that need different numbers of steps, with the one tolerance that
    test_pf_cpu.py shows to separate them -- run once on the device."""
    t = dict(pc.trio())
    with _plan(gpu, t["case"], batch=3) as plan:
        t["vm"], t["va"], t["info"] = plan.solve(t["case"]["Yz"], t["S"], t["vm0"], t["va0"], tol=t["tol"], max_iters=20)
    t["want"] = t["runs"]
    return t


def test_batch_members_stop_on_their_own(gpu, trio):
    t = trio
    assert list(t["info"]["flag"]) == [0, 0, 0]
    assert list(t["info"]["iters"]) == [w["iters"] for w in t["want"]]
    with _plan(gpu, t["case"], batch=3) as plan:
        for b in range(3):
            k = int(t["info"]["iters"][b])
            vm, va, info = plan.solve(t["case"]["Yz"], t["S"], t["vm0"], t["va0"], tol=t["tol"], max_iters=k)
            assert np.array_equal(_bits(vm[b]), _bits(t["vm"][b])) and np.array_equal(_bits(va[b]), _bits(t["va"][b])), b
            assert info["flag"][b] == 0 and info["iters"][b] == k and _bits(info["norm"])[b] == _bits(t["info"]["norm"])[b]
            assert all(info["flag"][m] == (0 if t["info"]["iters"][m] <= k else 1) for m in range(3))


def test_same_call_twice_host_and_device_forms_and_replicated_y(gpu, trio):
    import torch
    t = trio
    case, S, vm0, va0 = t["case"], t["S"], t["vm0"], t["va0"]
    with _plan(gpu, case, batch=3) as plan, _plan(gpu, case, batch=3, y_batch=3) as plan3:
        F, norm = plan.mismatch(case["Yz"], S, vm0, va0)
        Jx = plan.jacobian(case["Yz"], vm0, va0)
        again = plan.mismatch(case["Yz"], S, vm0, va0)
        assert np.array_equal(_bits(F), _bits(again[0])) and np.array_equal(_bits(norm), _bits(again[1]))
        assert np.array_equal(_bits(Jx), _bits(plan.jacobian(case["Yz"], vm0, va0)))
        vm, va, info = plan.solve(case["Yz"], S, vm0, va0, tol=t["tol"], max_iters=20)
        assert np.array_equal(_bits(vm), _bits(t["vm"])) and np.array_equal(_bits(va), _bits(t["va"]))
        # the device forms
        yz, s, dvm, dva = _dev(case["Yz"]), _dev(S), _dev(vm0), _dev(va0)
        f, nr, jx = torch.empty(3 * plan.nj, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda"), \
            torch.empty(3 * plan.nnz_j, dtype=torch.float64, device="cuda")
        plan.mismatch_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), f.data_ptr(), nr.data_ptr())
        plan.jacobian_dev(yz.data_ptr(), dvm.data_ptr(), dva.data_ptr(), jx.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(f.cpu().numpy()), _bits(F).reshape(-1)) and np.array_equal(_bits(nr.cpu().numpy()), _bits(norm))
        assert np.array_equal(_bits(jx.cpu().numpy()), _bits(Jx).reshape(-1))
        dinfo = plan.solve_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), tol=t["tol"], max_iters=20)
        assert np.array_equal(_bits(dvm.cpu().numpy()), _bits(vm).reshape(-1)) and np.array_equal(_bits(dva.cpu().numpy()), _bits(va).reshape(-1))
        for name in ("iters", "norm", "flag"):
            assert np.array_equal(dinfo[name], info[name]), name
        # one Y for all against one Y per scenario, replicated
        Y3 = np.tile(case["Yz"], (3, 1))
        F3, norm3 = plan3.mismatch(Y3, S, vm0, va0)
        assert np.array_equal(_bits(F3), _bits(F)) and np.array_equal(_bits(norm3), _bits(norm))
        assert np.array_equal(_bits(plan3.jacobian(Y3, vm0, va0)), _bits(Jx))
        vm3, va3, info3 = plan3.solve(Y3, S, vm0, va0, tol=t["tol"], max_iters=20)
        assert np.array_equal(_bits(vm3), _bits(vm)) and np.array_equal(_bits(va3), _bits(va)) and np.array_equal(info3["iters"], info["iters"])


def test_entries_of_s_that_are_never_read(gpu, trio):
    t = trio
    case, S = t["case"], t["S"].copy()
    S[:, 0] = complex(np.nan, np.nan)                                    # the reference bus
    S.imag[:, case["pv"]] = np.nan                                       # Im S at the PV buses (the real parts stay)
    assert np.isnan(S.imag[:, case["pv"]]).all() and np.array_equal(S.real[:, 1:], t["S"].real[:, 1:])
    with _plan(gpu, case, batch=3) as plan:
        F, norm = plan.mismatch(case["Yz"], S, t["vm0"], t["va0"])
        F0, norm0 = plan.mismatch(case["Yz"], t["S"], t["vm0"], t["va0"])
        assert np.array_equal(_bits(F), _bits(F0)) and np.array_equal(_bits(norm), _bits(norm0))
        vm, va, info = plan.solve(case["Yz"], S, t["vm0"], t["va0"], tol=t["tol"], max_iters=20)
    assert np.array_equal(_bits(vm), _bits(t["vm"])) and np.array_equal(_bits(va), _bits(t["va"]))
    assert np.array_equal(info["iters"], t["info"]["iters"]) and np.array_equal(_bits(info["norm"]), _bits(t["info"]["norm"]))


def test_a_converged_start_is_left_alone(gpu, trio):
    t = trio
    with _plan(gpu, t["case"], batch=3) as plan:
        vm, va, info = plan.solve(t["case"]["Yz"], t["S"], t["vm"], t["va"], tol=t["tol"], max_iters=20)
    assert list(info["iters"]) == [0, 0, 0] and list(info["flag"]) == [0, 0, 0]
    assert np.array_equal(_bits(vm), _bits(t["vm"])) and np.array_equal(_bits(va), _bits(t["va"]))


def test_the_driver_adds_nothing_to_a_hand_driven_loop(gpu, trio):
    import torch
    t = trio
    case = t["case"]
    with _plan(gpu, case, batch=3) as plan:
        fz = plan.factorization
        vm, va = t["vm0"].copy(), t["va0"].copy()
        yz, s = _dev(case["Yz"]), _dev(t["S"])
        f = torch.empty((3, plan.nj), dtype=torch.float64, device="cuda")
        nr = torch.empty(3, dtype=torch.float64, device="cuda")
        jx = torch.empty(3 * plan.nnz_j, dtype=torch.float64, device="cuda")
        pvpq, pq, npvpq = np.concatenate([case["pv"], case["pq"]]), case["pq"], len(case["pv"]) + len(case["pq"])
        active, iters = np.ones(3, dtype=bool), np.zeros(3, dtype=int)
        for it in range(21):
            dvm, dva = _dev(vm), _dev(va)
            plan.mismatch_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), f.data_ptr(), nr.data_ptr())
            norm = nr.cpu().numpy()
            newly = active & (norm <= t["tol"])
            iters[newly] = it
            active &= ~newly
            if not active.any():
                break
            plan.jacobian_dev(yz.data_ptr(), dvm.data_ptr(), dva.data_ptr(), jx.data_ptr())
            fz.factor_solve_dev(jx.data_ptr(), f.data_ptr(), k=1, tol=1e-3)
            fz.factor_status()
            dx = f.cpu().numpy()
            for b in np.flatnonzero(active):                             # the NumPy += of the definition
                va[b, pvpq] += dx[b, :npvpq]
                vm[b, pq] += dx[b, npvpq:]
    assert list(iters) == list(t["info"]["iters"])
    assert np.array_equal(_bits(vm), _bits(t["vm"])) and np.array_equal(_bits(va), _bits(t["va"]))


def test_a_member_that_is_not_finite_is_flagged_alone(gpu, trio):
    t = trio
    case = t["case"]
    S = t["S"].copy()
    S[1, case["pq"][3]] = np.nan
    good = t["S"].copy()
    good[1] = good[0]
    with _plan(gpu, case, batch=3) as plan:
        vm, va, info = plan.solve(case["Yz"], S, t["vm0"], t["va0"], tol=t["tol"], max_iters=20)
        gvm, gva, ginfo = plan.solve(case["Yz"], good, t["vm0"], t["va0"], tol=t["tol"], max_iters=20)
    assert info["flag"][1] == 2 and info["iters"][1] == 0 and not np.isfinite(info["norm"][1])
    for b in (0, 2):
        assert info["flag"][b] == 0 and info["iters"][b] == ginfo["iters"][b]
        assert np.array_equal(_bits(vm[b]), _bits(gvm[b])) and np.array_equal(_bits(va[b]), _bits(gva[b])), b


NEWTON_KEYS = [k for k in KERNEL_KEYS if k != "grid_edge"]


def _inverse_norm(P, case, vm, va):
    J = R.dense_jacobian(P, R.jacobian_ref(P, case["Yz"], vm, va)[0])
    return np.abs(np.linalg.inv(J)).sum(axis=1).max()


@pytest.mark.parametrize("key", NEWTON_KEYS)
def test_newton_against_the_restatement(gpu, limits, key):
    case = _case(limits, key)
    ref = pc.reference(key, case)
    P, tol = ref["P"], ref["tol"]
    with _plan(gpu, case) as plan:
        vm, va, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=tol, max_iters=20)
    assert info["flag"][0] == 0 and info["iters"][0] == ref["iters"], (info, ref["run"]["norms"])
    at = R.mismatch_ref(P, case["Yz"], case["S"], vm[0], va[0])
    assert (np.abs(at["F"]) <= tol + at["bound"]).all()
    want = R.newton_ref(P, case["Yz"], case["S"], case["vm0"], case["va0"], tol, 20)
    bound = 2 * _inverse_norm(P, case, want["vm"], want["va"]) * 2 * tol    # a first-order Newton estimate, doubled for the second-order term
    assert np.abs(R.unknowns(P, vm[0], va[0]) - R.unknowns(P, want["vm"], want["va"])).max() <= bound


@pytest.mark.parametrize("every", [2, 3])
def test_dishonest_newton_reaches_the_same_solution(gpu, every):
    case = pc.planted(1)
    ref = pc.reference("planted1", case)
    P, tol = ref["P"], ref["tol"]
    with _plan(gpu, case) as plan:
        vm, va, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=tol, max_iters=40, refactor_every=every)
    assert info["flag"][0] == 0 and info["iters"][0] >= ref["iters"]
    bound = 2 * _inverse_norm(P, case, ref["run"]["vm"], ref["run"]["va"]) * 2 * tol
    assert np.abs(R.unknowns(P, vm[0], va[0]) - R.unknowns(P, ref["run"]["vm"], ref["run"]["va"])).max() <= bound


def test_flags_of_three_scenarios(gpu):
    case = pc.planted(2)
    S, vm0, va0 = pc.scaled(case, [1.0, 1.3, 0.5])
    with _plan(gpu, case, batch=3) as plan:
        vm, va, info = plan.solve(case["Yz"], S, vm0, va0, tol=pc.NOMINAL_TOL, max_iters=11)
    assert list(info["flag"]) == [0, 1, 0]
    assert info["iters"][1] == 11 and np.isfinite(info["norm"][1]) and info["norm"][1] > pc.NOMINAL_TOL
    assert info["iters"][0] == pc.PLANTED_ITERS[2] and (info["norm"][[0, 2]] <= pc.NOMINAL_TOL).all()


def test_max_iters_zero_evaluates_the_mismatch_only(gpu):
    case = pc.planted(1)
    with _plan(gpu, case) as plan:
        F, norm = plan.mismatch(case["Yz"], case["S"], case["vm0"], case["va0"])
        vm, va, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=1e-8, max_iters=0)
    assert info["flag"][0] == 1 and info["iters"][0] == 0 and _bits(info["norm"])[0] == _bits(norm)[0]
    assert np.array_equal(_bits(vm[0]), _bits(case["vm0"])) and np.array_equal(_bits(va[0]), _bits(case["va0"]))


def test_a_rejected_pivot_and_the_perturbed_handle(gpu):
    """Scenario 1 gets a dead bus: the values of a PQ bus's column of Y zeroed -- and of its row, since the diagonal
    entries of the Jacobian come from the bus's current, which the column alone leaves standing.  Column and row of that
    bus in J are then exactly zero."""
    case = pc.planted(1)
    dead = int(case["pq"][5])
    cols = np.repeat(np.arange(case["n"]), np.diff(case["Yp"]))
    Y2 = np.tile(case["Yz"], (2, 1))
    Y2[1, (cols == dead) | (case["Yi"] == dead)] = 0.0
    S, vm0, va0 = pc.scaled(case, [1.0, 1.0])
    S[1, dead] = 0.0
    with _plan(gpu, case, batch=2, y_batch=2) as plan:
        yz, s, dvm, dva = _dev(Y2), _dev(S), _dev(vm0), _dev(va0)
        with pytest.raises(gpu.SingularMatrix):
            plan.solve_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), tol=1e-8, max_iters=20, pivot_tol=1e-3)
        # the first factorisation failed: no update was completed
        assert np.array_equal(_bits(dvm.cpu().numpy()), _bits(vm0).reshape(-1)) and np.array_equal(_bits(dva.cpu().numpy()), _bits(va0).reshape(-1))
        plan.factorization.set_perturbation(1e-8)
        info = plan.solve_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), tol=1e-8, max_iters=20, pivot_tol=1e-3)
        assert info["flag"][0] == 0 and info["iters"][0] == pc.PLANTED_ITERS[1]
        n = case["n"]
        got_vm, got_va = dvm.cpu().numpy().reshape(2, n), dva.cpu().numpy().reshape(2, n)
        # the dead bus has a zero row, a zero column and a zero right-hand side: behind the replaced pivots its dx is 0 / delta
        assert _bits(got_vm[1, dead]) == _bits(vm0[1, dead]) and _bits(got_va[1, dead]) == _bits(va0[1, dead])
        # and scenario 0 is what it is beside a healthy neighbour, bit for bit
        ovm, ova, oinfo = plan.solve(np.tile(case["Yz"], (2, 1)), pc.scaled(case, [1.0, 1.0])[0], vm0, va0, tol=1e-8, max_iters=20)
        assert oinfo["iters"][0] == info["iters"][0]
        assert np.array_equal(_bits(got_vm[0]), _bits(ovm[0])) and np.array_equal(_bits(got_va[0]), _bits(ova[0]))


def test_a_pivot_rejected_at_a_later_iteration_keeps_the_completed_update(gpu):
    """planted3 in the natural order with pivot_tol = LATE_PIVOT_TOL: the Jacobian at the flat start passes, the one at the
    first iterate is rejected (test_pf_cpu.py asserts both, with room).  The call ends with CS3_ERR_PIVOT and the
    voltages are those after ONE update: k_pf_update skipped the second on the handle's status word."""
    case = pc.planted(3)
    n = case["n"]
    with _plan(gpu, case, order=gpu.ORDER_NATURAL) as plan:
        yz, s, dvm, dva = _dev(case["Yz"]), _dev(case["S"]), _dev(case["vm0"]), _dev(case["va0"])
        with pytest.raises(gpu.SingularMatrix):
            plan.solve_dev(yz.data_ptr(), s.data_ptr(), dvm.data_ptr(), dva.data_ptr(), tol=1e-8, max_iters=20, pivot_tol=pc.LATE_PIVOT_TOL)
        vm1, va1, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=1e-8, max_iters=1, pivot_tol=pc.LATE_PIVOT_TOL)
        assert info["flag"][0] == 1 and info["iters"][0] == 1
        assert not np.array_equal(vm1[0], case["vm0"]) and not np.array_equal(va1[0], case["va0"])
        assert np.array_equal(_bits(dvm.cpu().numpy()), _bits(vm1[0])) and np.array_equal(_bits(dva.cpu().numpy()), _bits(va1[0]))
        # at the usual threshold the same plan runs through
        vm, va, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=pc.reference("planted3", case)["tol"], max_iters=20)
        assert info["flag"][0] == 0 and info["iters"][0] == pc.PLANTED_ITERS[3]


def test_the_powerflow_class(gpu, trio):
    """csparse3_amd.powerflow.PowerFlow is sugar: complex voltages in and out, around the plan's vm and va."""
    from csparse3_amd.csc import CscMat
    from csparse3_amd.powerflow import PowerFlow
    t = trio
    case, n = t["case"], t["case"]["n"]
    want = t["vm"] * np.exp(1j * t["va"])
    V0 = case["vm0"] * np.exp(1j * case["va0"])                          # va0 = 0: |V0| and angle(V0) are vm0 and +0 exactly
    assert np.array_equal(_bits(np.abs(V0)), _bits(case["vm0"])) and np.array_equal(_bits(np.angle(V0)), _bits(case["va0"]))
    Y = CscMat(n, n, indptr=case["Yp"], indices=case["Yi"], data=case["Yz"])
    with PowerFlow(Y, case["pv"], case["pq"], batch=3) as pf:            # a CscMat: its values are the default Yz; V0 [n] serves all
        V, info = pf.solve(None, t["S"], V0, tol=t["tol"])
        assert V.shape == (3, n) and V.dtype == np.complex128
        assert np.array_equal(_bits(V.view(np.float64)), _bits(want.view(np.float64)))
        assert np.array_equal(info["iters"], t["info"]["iters"]) and np.array_equal(info["flag"], t["info"]["flag"])
        F, norm = pf.mismatch(None, t["S"], V0)
        Jx = pf.jacobian(None, V0)
        with _plan(gpu, case, batch=3) as plan:
            F0, norm0 = plan.mismatch(case["Yz"], t["S"], t["vm0"], t["va0"])
            assert np.array_equal(_bits(F), _bits(F0)) and np.array_equal(_bits(norm), _bits(norm0))
            assert np.array_equal(_bits(Jx), _bits(plan.jacobian(case["Yz"], t["vm0"], t["va0"])))
        assert pf.factorization is pf.plan.factorization and pf.factorization.info.n == pf.plan.nj
    # the pattern as a tuple, one Y per scenario from ONE value array, S and V0 per scenario
    with PowerFlow((n, case["Yp"], case["Yi"]), case["pv"], case["pq"], batch=3, y_batch=3) as pf:
        V, info = pf.solve(case["Yz"], t["S"], np.tile(V0, (3, 1)), tol=t["tol"])
        assert np.array_equal(_bits(V.view(np.float64)), _bits(want.view(np.float64)))
        with pytest.raises(AssertionError):
            pf.solve(None, t["S"], V0)                                   # a pattern has no values of its own
    # one S for all scenarios
    with PowerFlow(Y, case["pv"], case["pq"], batch=2) as pf:
        V, info = pf.solve(None, t["S"][0], V0, tol=t["tol"])
        assert np.array_equal(_bits(V[0].view(np.float64)), _bits(V[1].view(np.float64))) and list(info["iters"]) == [t["info"]["iters"][0]] * 2


def test_the_lent_handle_is_a_full_handle_and_goes_with_the_plan(gpu):
    case = pc.planted(1)
    ref = pc.reference("planted1", case)
    gc.collect()
    live0 = gpu.debug_live_device_buffers()
    plan = _plan(gpu, case)
    fz = plan.factorization
    vm, va, info = plan.solve(case["Yz"], case["S"], case["vm0"], case["va0"], tol=ref["tol"], max_iters=20)
    assert gpu.debug_live_device_buffers() > live0
    # the factors are those of the last Jacobian the driver built: at the iterate before the converged one
    Jx = plan.jacobian(case["Yz"], vm, va)
    J = R.dense_jacobian(ref["P"], Jx[0])
    cond, inv_norm = fz.condest(Jx)
    exact = np.abs(np.linalg.inv(J)).sum(axis=0).max()
    assert 0.3 * exact <= np.ravel(inv_norm)[0] <= 1.01 * exact           # Hager's estimate is a lower bound of ||J^-1||_1, seldom far below
    sign, logabs = fz.slogdet()
    s_ref, l_ref = np.linalg.slogdet(J)
    assert np.ravel(sign)[0] == s_ref and abs(np.ravel(logabs)[0] - l_ref) <= 1e-3 * abs(l_ref) + 1e-3     # (the held Jacobian is one step back)
    plan.close()
    assert gpu.debug_live_device_buffers() == live0
    with pytest.raises(gpu.Cs3Error):
        fz.slogdet()
    with pytest.raises(gpu.Cs3Error):
        fz.info
    fz.close()                                                           # frees nothing: the handle went with the plan
    assert gpu.debug_live_device_buffers() == live0
