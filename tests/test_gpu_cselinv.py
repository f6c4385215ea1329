"""Complex selected inversion (cs3_cplx_selinv_*) on the GPU.

Bit for bit against the restatement (tests/cselinv_ref.py), which takes the REAL handle's own getters and the plan's
rotation as input; and against numpy.linalg.inv of the complex matrix with the project's bound for the selected
inversion: max |Z - Z_ref| <= 1e-10 max |Z_ref| on matrices with cond_1 <= 1e4 (asserted per case), four times that for the
Thevenin table, which sums four such entries (relative to max |Z_ref|, not to |T|).
Gather edges of the three kernels, even-wide fronts of the real form across the kernel classes of the real selected
inversion, a batch, state, memory, and the route through sens_solve that the diagonal replaces."""
import numpy as np
import pytest

import cselinv_cases as cc
import cselinv_ref as cr

pytestmark = pytest.mark.gpu

KEYS = ("entries", "entries_t", "diagonal", "thevenin")
_REF = {}


def _reference(name, case):
    """(dense results, max |Z_ref|, cond_1) of a case, computed once and left alone."""
    if name not in _REF:
        n, Ap, Ai, Az = case[:4]
        Z, cond = cr.dense_inverse(n, Ap, Ai, Az)
        want = cr.dense_results(Z, n, Ap, Ai)
        for v in want.values():
            v.setflags(write=False)
        _REF[name] = (want, float(np.abs(Z).max()), cond)
    return _REF[name]


def _host_results(F):
    return {"entries": F.inverse_entries(), "entries_t": F.inverse_entries(trans=True), "diagonal": F.inverse_diagonal(),
            "thevenin": F.thevenin()}


def _dev_results(F, torch):
    """The four `_dev` getters on the current stream, after selinv() on it."""
    st = torch.cuda.current_stream().cuda_stream
    F.selinv(st)
    out = {key: torch.full((F.batch, F.n if key == "diagonal" else F.nnz), complex(-7.0, -7.0), dtype=torch.complex128, device="cuda:0")
           for key in KEYS}
    F.inverse_entries_dev(out["entries"].data_ptr(), False, st)
    F.inverse_entries_dev(out["entries_t"].data_ptr(), True, st)
    F.inverse_diagonal_dev(out["diagonal"].data_ptr(), st)
    F.thevenin_dev(out["thevenin"].data_ptr(), st)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


def _factorised(gpu, case, rotate=None, batch=1, values=None):
    n, Ap, Ai, Az = case[:4]
    F = gpu.ComplexFactorization(n, Ap, Ai, kind=cc.kind_of(case), rotate=case[5] if rotate is None else rotate, batch=batch)
    try:
        return F.factor(Az if values is None else values)
    except Exception:
        F.close()
        raise


def _assert_restated(F, case, got, what):
    n, Ap, Ai = case[:3]
    want = cr.restate_from_handle(F, Ap, Ai)
    for key in KEYS:
        g = np.asarray(got[key]).reshape(F.batch, -1)
        assert cr.same_bits(g, want[key]), "%s: %s differs from the restatement in %d of %d numbers" % (
            what, key, int((g != want[key]).sum()), g.size)


def _assert_dense(name, case, got, what):
    want, scale, cond = _reference(name, case)
    assert cond <= cr.COND_MAX, (name, cond)
    for key in KEYS:
        err = cr.max_error(np.asarray(got[key]).reshape(-1), want[key], scale)
        print("%s %s: %.3e (cond %.2e)" % (what, key, err, cond))
        assert err <= (4 if key == "thevenin" else 1) * cr.BOUND, (what, key, err)


# -- 1. the restatement, bit for bit; 2. the dense inverse

@pytest.mark.parametrize("name", sorted(cc.matrices()))
def test_restatement_bit_for_bit_and_dense_inverse(gpu, name):
    import torch
    case = cc.matrices()[name]
    for rotate in cc.rotations(name, case):
        what = "%s rotate=%d" % (name, rotate)
        with _factorised(gpu, case, rotate) as F:
            got = _host_results(F)
            assert got["entries"].shape == (F.nnz,) and got["diagonal"].shape == (F.n,) and got["thevenin"].dtype == np.complex128
            _assert_restated(F, case, got, what)
            dev = _dev_results(F, torch)
            for key in KEYS:
                assert cr.same_bits(dev[key][0], got[key]), (what, key, "device and host forms differ")
            if rotate:
                assert not np.all(F.plan.rotation() == 1.0)                  # the rotation is at work in these cases
            if rotate == case[5]:
                _assert_dense(name, case, got, what)
            if case[4] == "chol":                                            # Hermitian to rounding
                want, scale, _ = _reference(name, case)
                assert np.abs(got["entries"] - np.conj(got["entries_t"])).max() <= 2 * cr.BOUND * scale
                assert np.all(F.plan.rotation() == 1.0)


# -- 3. gather edges

@pytest.mark.parametrize("n", cc.gather_edge_orders())
def test_gather_edges_on_diagonal_matrices(gpu, n):
    """n = nnz one below, at and one above a workgroup: 1 / a_ii, and the restatement bit for bit."""
    import torch
    case = cc.diagonal(n, seed=n)
    with _factorised(gpu, case) as F:
        got = _dev_results(F, torch)
        _assert_restated(F, case, got, "diagonal %d" % n)
        _assert_dense("diagonal%d" % n, case, {k: v[0] for k, v in got.items()}, "diagonal %d" % n)
        assert cr.max_error(got["diagonal"][0], 1.0 / case[3], np.abs(1.0 / case[3]).max()) <= cr.BOUND


def test_gather_edge_on_a_network(gpu):
    import torch
    case = cc.synth.ybus(257, 330, 7) + ("lu", True)
    assert case[0] == int(cc.LIMITS.block) + 1
    with _factorised(gpu, case) as F:
        got = _dev_results(F, torch)
        _assert_restated(F, case, got, "ybus257")
        _assert_dense("ybus257", case, {k: v[0] for k, v in got.items()}, "ybus257")


def test_one_number_past_the_grid_takes_a_second_pass(gpu):
    import torch
    n = cc.grid_stride_order()
    case = cc.diagonal(n, seed=5)
    with _factorised(gpu, case) as F:
        got = _dev_results(F, torch)
        _assert_restated(F, case, got, "grid stride")
        inv = 1.0 / case[3]
        scale = np.abs(inv).max()
        assert np.abs(case[3]).max() / np.abs(case[3]).min() <= cr.COND_MAX
        for key in ("entries", "entries_t", "diagonal"):
            assert cr.max_error(got[key][0], inv, scale) <= cr.BOUND, key
        assert cr.max_error(got["thevenin"][0], np.zeros(n), scale) <= 4 * cr.BOUND      # ((z + z) - z) - z


# -- 4. even-wide fronts of the real form across the kernel classes of the real selected inversion

@pytest.mark.parametrize("order2", cc.dense_root_orders())
def test_dense_root_of_the_real_form(gpu, order2):
    case = cc.dense_root(order2)
    name = "dense_root_%d" % order2
    with _factorised(gpu, case) as F:
        orders = cc.front_orders(F.real)
        assert [r for r, w, parent in orders if parent < 0] == [order2]
        assert all(w % 2 == 0 and r % 2 == 0 for r, w, parent in orders)      # every supernode of a real form is even-wide
        assert (F.real.selinv_info().nfronts_big > 0) == (order2 > cc.REAL_LIMITS.lds_max_order)
        got = _host_results(F)
        _assert_restated(F, case, got, name)
        _assert_dense(name, case, got, name)
        s = F.plan.rotation()[0]
        assert np.abs(s.imag).min() > 0.5                                      # diagonal phases near pi / 2: the rotation matters


# -- 5. a batch of three

def test_batch_of_three_equals_each_alone(gpu):
    import torch
    case = cc.matrices()["ybus40"]
    AZ = cc.batch_values(case, 3, seed=8)
    with _factorised(gpu, case, batch=3, values=AZ) as F:
        s = F.plan.rotation()
        assert not np.array_equal(s[0], s[1]) and not np.array_equal(s[1], s[2])
        got = _host_results(F)
        assert got["entries"].shape == (3, F.nnz) and got["diagonal"].shape == (3, F.n)
        _assert_restated(F, case, got, "batch of three")
        dev = _dev_results(F, torch)
        for key in KEYS:
            assert cr.same_bits(dev[key], got[key]), key
    for b in range(3):
        one = case[:3] + (AZ[b],) + case[4:]
        with _factorised(gpu, one) as F1:
            alone = _host_results(F1)
            for key in KEYS:
                assert cr.same_bits(alone[key], got[key][b]), "matrix %d: %s differs from the same matrix alone" % (b, key)
            _assert_dense("batch%d" % b, one, alone, "matrix %d" % b)


# -- 6. state

def _rc(gpu, fn, *args):
    rc = fn(*args)
    return rc, gpu.lib().cs3_last_error().decode()


def test_state(gpu):
    import torch
    L = gpu.lib()
    case = cc.matrices()["ybus40"]
    n, Ap, Ai, Az = case[:4]
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(int(Ap[n]) + 1, dtype=torch.complex128, device="cuda:0")          # (one more: room behind a misaligned start)
    with _factorised(gpu, case) as F:
        p, h = F.plan._p, F.real._h
        getters = {"entries": lambda ptr: L.cs3_cplx_selinv_entries_dev(p, h, 0, ptr, st),
                   "diagonal": lambda ptr: L.cs3_cplx_selinv_diag_dev(p, h, ptr, st),
                   "thevenin": lambda ptr: L.cs3_cplx_selinv_thevenin_dev(p, h, ptr, st)}
        for key, call in getters.items():                                    # before selinv()
            rc, msg = _rc(gpu, call, out.data_ptr())
            assert rc == gpu.CS3_ERR_STATE and "no selected inverse of the current factors" in msg, (key, msg)
        F.selinv(st)
        for key, call in getters.items():
            assert call(out.data_ptr()) == 0, key
            rc, msg = _rc(gpu, call, out.data_ptr() + 8)                     # a misaligned pointer
            assert rc == gpu.CS3_ERR_ARG and "aligned to 16 bytes" in msg, (key, msg)
        torch.cuda.synchronize()
        d0, s0 = F.inverse_diagonal(), F.plan.rotation().copy()
        # a refactorisation with other values and another rotation: the old Z is refused, the host forms recompute
        Az2 = cc.batch_values(case, 1, seed=21)[0]
        F.factor(Az2)
        assert not np.array_equal(F.plan.rotation(), s0)
        for key, call in getters.items():
            rc, msg = _rc(gpu, call, out.data_ptr())
            assert rc == gpu.CS3_ERR_STATE, (key, msg)
        got = _host_results(F)
        assert not np.array_equal(got["diagonal"], d0)
        two = case[:3] + (Az2,) + case[4:]
        _assert_restated(F, two, got, "after a refactorisation")
        _assert_dense("ybus40_refactored", two, got, "after a refactorisation")
        assert getters["diagonal"](out.data_ptr()) == 0                       # the host forms left a valid ZR
        torch.cuda.synchronize()
        assert cr.same_bits(out[:n].cpu().numpy(), got["diagonal"])
        # a plan / handle pair of different order
        with gpu.ComplexFactorization(*cc.matrices()["unsorted"][:3]) as G:
            for pp, hh in ((G.plan._p, h), (p, G.real._h)):
                rc, msg = _rc(gpu, L.cs3_cplx_selinv_diag_dev, pp, hh, out.data_ptr(), st)
                assert rc == gpu.CS3_ERR_ARG and "not one on the real form" in msg, msg
    # a Schur ComplexFactorization is refused with the real wording
    with gpu.ComplexFactorization(n, Ap, Ai, schur=[37, 3, 11]) as FS:
        FS.factor(Az)
        for call in (FS.inverse_diagonal, FS.inverse_entries, FS.thevenin):
            with pytest.raises(gpu.Cs3Error, match="not available on a Schur handle") as e:
                call()
            assert e.value.code == gpu.CS3_ERR_ARG


# -- 7. memory

@pytest.mark.parametrize("plan_first", [True, False])
def test_memory_goes_with_plan_and_handle_in_either_order(gpu, plan_first):
    import torch
    live = gpu.debug_live_device_buffers()
    case = cc.matrices()["ybus40"]
    F = _factorised(gpu, case)
    first = _host_results(F)
    _dev_results(F, torch)
    held = gpu.debug_live_device_buffers()
    assert held > live
    again = _host_results(F)                                                 # a second call of every getter allocates nothing
    dev = _dev_results(F, torch)
    assert gpu.debug_live_device_buffers() == held
    for key in KEYS:
        assert cr.same_bits(again[key], first[key]) and cr.same_bits(dev[key][0], first[key]), key
    if plan_first:
        F.plan.close()
        F.real.close()
    else:
        F.real.close()
        F.plan.close()
    assert gpu.debug_live_device_buffers() == live


# -- 8. the route this replaces

def test_diagonal_equals_the_sensitivities_route(gpu):
    """diag(Z-bus) from sens_solve with unit columns: both within the bound of the truth, so within twice of each other."""
    name = "ybus300"
    case = cc.matrices()[name]
    n = case[0]
    want, scale, cond = _reference(name, case)
    assert cond <= cr.COND_MAX
    with _factorised(gpu, case) as F:
        with F.sens_plan((n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)), None) as plan:
            Y = F.sens_solve(plan, np.ones(n, dtype=np.complex128), None)
        d = F.inverse_diagonal()
    assert cr.max_error(Y.diagonal(), want["diagonal"], scale) <= cr.BOUND
    assert cr.max_error(d, want["diagonal"], scale) <= cr.BOUND
    assert cr.max_error(d, Y.diagonal(), scale) <= 2 * cr.BOUND
