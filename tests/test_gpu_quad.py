"""Bilinear forms on the selected inverse (cs3_quad_*) on the GPU.
Accuracy: |t - t_ref| <= 1e-10 * sum |c_a| |Z_ref(a, b)| |b_b| per row against the dense inverse (tests/quad_ref.py), on
matrices with cond_1 <= 1e4 (asserted per test).  Bits: t equals the restated sums on the Z the handle hands out, in every
class; between runs, between the device and the host form, between a matrix of a batch and the same matrix alone.  The
incidence form against the sens route, the normalised residuals of synth.se_case, state and memory."""
import math

import numpy as np
import pytest

import quad_cases as qc
import quad_ref as ref
import selinv_ref

pytestmark = pytest.mark.gpu

FORM_CASES = sorted(qc.form_cases())
_REF = {}


def _reference(name, matrix):
    """(Z_ref, cond) of a matrix, computed once."""
    if name not in _REF:
        _REF[name] = selinv_ref.dense_inverse(matrix[1], matrix[2], matrix[3], matrix[4])
        _REF[name][0].setflags(write=False)
    return _REF[name]


def _matrix_name(name):
    return "dense" if name.startswith(("two_", "one_", "single_", "classes_")) else name


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _forms_dev(torch, F, plan, Cx, Bx):
    """quad_forms_dev on the current stream, into an array that held something else."""
    cx, bx = _dev(torch, Cx), (None if Bx is None else _dev(torch, Bx))
    t = torch.full((F.batch, plan.m), -7.0, dtype=torch.float64, device="cuda:0")
    F.quad_forms_dev(plan, cx.data_ptr(), 0 if bx is None else bx.data_ptr(), t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t = t.cpu().numpy()
    return t[0] if F.batch == 1 else t


def _restated(F, plan, case, Cx=None, Bx=None):
    """The restated sums on the Z that inverse_entries() hands out (every case pairs columns on the pattern of A)."""
    mat = case["matrix"]
    Z = ref.scatter_entries(mat[1], mat[2], mat[3], F.inverse_entries())
    zterm = ref.z_at_terms(Z, case["Ct"], case["Bt"])
    assert np.isfinite(zterm).all()
    return ref.restated_forms(case["Ct"], case["Bt"], case["Cx"] if Cx is None else Cx, case["Bx"] if Bx is None else Bx, zterm,
                              plan.debug_plan()[0])


# -- 1. accuracy and bits, every case

@pytest.mark.parametrize("name", FORM_CASES)
def test_forms(gpu, name):
    import torch
    case = qc.form_cases()[name]
    mat = case["matrix"]
    Zref, cond = _reference(_matrix_name(name), mat)
    assert cond <= ref.COND_MAX, (name, cond)
    t_ref, scale = ref.dense_forms(Zref, case["Ct"], case["Bt"], case["Cx"], case["Bx"])
    with qc.analysed(case) as F, F.quad_plan(case["Ct"], case["Bt"]) as plan:
        F.factor(mat[4])
        t = F.quad_forms(plan, case["Cx"], case["Bx"])              # (the host form computes Z)
        assert t.shape == (case["Ct"][0],)
        err = np.abs(t - t_ref)
        print("%s: m=%d terms=%d max err / scale %.3e" % (name, plan.m, plan.info.nterms, (err[scale > 0] / scale[scale > 0]).max(initial=0.0)))
        assert (err <= ref.BOUND * scale).all(), name
        want = _restated(F, plan, case)
        assert np.array_equal(t, want), (name, np.flatnonzero(t != want)[:8])
        assert np.array_equal(F.quad_forms(plan, case["Cx"], case["Bx"]), t), "two runs differ"
        assert np.array_equal(_forms_dev(torch, F, plan, case["Cx"], case["Bx"]), t), "the device form differs from the host form"


# -- 2. batch

def test_batch_of_three_with_values_of_their_own(gpu):
    import torch
    case = qc.two_operands()
    mat = case["matrix"]
    AX, CX, BX = qc.batch_values(case)
    with qc.analysed(case, batch=3) as F, F.quad_plan(case["Ct"], case["Bt"]) as plan:
        F.factor(AX)
        T = F.quad_forms(plan, CX, BX)
        assert T.shape == (3, plan.m)
        assert np.array_equal(_forms_dev(torch, F, plan, CX, BX), T)
        for b in range(3):
            Zref, cond = selinv_ref.dense_inverse(mat[1], mat[2], mat[3], AX[b])
            assert cond <= ref.COND_MAX
            t_ref, scale = ref.dense_forms(Zref, case["Ct"], case["Bt"], CX[b], BX[b])
            assert (np.abs(T[b] - t_ref) <= ref.BOUND * scale).all(), b
            with qc.analysed(case) as F1, F1.quad_plan(case["Ct"], case["Bt"]) as plan1:
                F1.factor(AX[b])
                assert np.array_equal(F1.quad_forms(plan1, CX[b], BX[b]), T[b]), "matrix %d differs from the same matrix alone" % b
        assert not np.array_equal(T[0], T[1])


# -- 3. the incidence form against the sens route

@pytest.mark.parametrize("name", ["jacobian_like", "tridiagonal"])
def test_incidence_form_equals_the_sens_route(gpu, name):
    case = qc.incidence(name)
    mat, Ct, Cx = case["matrix"], case["Ct"], case["Cx"]
    Zref, cond = _reference("incidence_" + name, mat)
    assert cond <= ref.COND_MAX
    _, scale = ref.dense_forms(Zref, Ct, None, Cx, None)
    with qc.analysed(case) as F:
        F.factor(mat[4])
        with F.quad_plan(Ct) as plan:
            t = F.quad_forms(plan, Cx)
        with F.sens_plan(Ct, Ct) as splan:                          # B = C' by columns, C by rows: Y = C A^-1 C'
            Y = F.sens_solve(splan, Cx, Cx)
        assert (np.abs(t - Y.diagonal()) <= ref.BOUND * scale).all()
        Z = ref.scatter_entries(mat[1], mat[2], mat[3], F.inverse_entries())
        i, j = Ct[2][0::2], Ct[2][1::2]
        assert (np.abs(t - (Z[i, i] + Z[j, j] - Z[i, j] - Z[j, i])) <= ref.BOUND * scale).all()


def test_cscmat_methods(gpu):
    from csparse3_amd.csc import CscMat
    case = qc.incidence("jacobian_like")
    m, n, Ap, Ai, Ax = case["matrix"]
    Zref, _ = _reference("incidence_jacobian_like", case["matrix"])
    t_ref, scale = ref.dense_forms(Zref, case["Ct"], None, case["Cx"], None)
    A = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    nl = case["Ct"][0]
    order = np.lexsort((np.repeat(np.arange(nl), 2), case["Ct"][2]))           # C (nl x n) by columns
    Cp = np.concatenate([[0], np.cumsum(np.bincount(case["Ct"][2], minlength=n))]).astype(np.int32)
    Cm = CscMat(nl, n, indptr=Cp, indices=np.repeat(np.arange(nl), 2)[order].astype(np.int32), data=case["Cx"][order])
    for kw in ({}, {"B": Cm}):
        assert (np.abs(A.quad_forms(Cm, **kw) - t_ref) <= ref.BOUND * scale).all()
    se = qc.se(40, 60)
    gm, gn, Gp, Gi, Gx = se["matrix"]
    H = se["H"]
    hi, hj = np.nonzero(H.T)
    hi, hj = hj, hi
    Hm = CscMat(H.shape[0], gn, indptr=np.concatenate([[0], np.cumsum(np.bincount(hj, minlength=gn))]).astype(np.int32),
                indices=hi.astype(np.int32), data=H[hi, hj])
    r = np.cos(np.arange(H.shape[0]))
    rn, info = CscMat(gm, gn, indptr=Gp, indices=Gi, data=Gx).normalized_residuals(Hm, se["w"], r, crit_tol=qc.CRIT_TOL)
    assert info["critical"] == len(se["critical_rows"]) and (rn[se["critical_rows"]] == 0.0).all()
    assert info["worst"] == rn.max() and info["worst_row"] == int(np.argmax(rn))


# -- 4. normalised residuals

def _estimate(F, se, bad, gross):
    """One weighted-least-squares solve of z = H x + noise with a gross error at row `bad`: the residuals."""
    H, w = se["H"], se["w"]
    rng = np.random.default_rng(5)
    z = H @ rng.standard_normal(H.shape[1]) + rng.standard_normal(H.shape[0]) / np.sqrt(w)
    z[bad] += gross / math.sqrt(w[bad])
    x = F.solve(H.T @ (w * z))
    return z - H @ x


@pytest.mark.parametrize("size", sorted(qc.SE_SEEDS))
def test_normalized_residuals_find_the_planted_error(gpu, size):
    se = qc.se(*size)
    mat, w, crit = se["matrix"], se["w"], se["critical_rows"]
    Zref, cond = _reference("se_%d_%d" % size, mat)
    assert cond <= ref.COND_MAX
    t_ref, scale = ref.dense_forms(Zref, se["Ct"], None, se["Cx"], None)
    m = len(w)
    bad = int(np.argmax(np.where(np.isin(np.arange(m), crit), -1.0, 1.0 - w * t_ref)))     # the best-checked measurement
    with qc.analysed(se) as F, F.quad_plan(se["Ct"]) as plan:
        F.factor(mat[4])
        r = _estimate(F, se, bad, 40.0)
        rn, info = F.normalized_residuals(plan, se["Cx"], w, r, qc.CRIT_TOL)
        print("se %s: worst %.3f at row %d (planted %d), J %.6g, critical %d" % (size, info["worst"], info["worst_row"], bad, info["J"],
                                                                                 info["critical"]))
        assert info["worst_row"] == bad and info["worst"] == rn[bad] == rn.max() and info["worst"] > 10.0
        assert (rn[crit] == 0.0).all() and info["critical"] == len(crit)
        assert (np.abs(info["t"] - t_ref) <= ref.BOUND * scale).all()
        assert np.array_equal(info["t"], _restated(F, plan, se))
        assert np.array_equal(info["t"], F.quad_forms(plan, se["Cx"]))
        omega, rn_want, summary = ref.restated_normres(info["t"], w, r, qc.CRIT_TOL, qc.LIMITS)
        assert np.array_equal(info["omega"], omega) and np.array_equal(rn, rn_want)
        assert [info["worst"], info["worst_row"], info["J"], info["critical"]] == summary.tolist()
        J_ref = math.fsum((w * r * r).tolist())
        print("   |J - J_ref| = %.3e, allowed %.3e" % (abs(info["J"] - J_ref), m * 2.0 ** -52 * J_ref))
        assert abs(info["J"] - J_ref) <= m * 2.0 ** -52 * J_ref


def _normres_dev(torch, F, plan, Hx, w, r, tol, outputs):
    """normalized_residuals_dev on the current stream -> (summary, t, omega, rn), None where no pointer was given."""
    hx, wd, rd = _dev(torch, Hx), _dev(torch, w), _dev(torch, r)
    summary = torch.full((F.batch, 4), -7.0, dtype=torch.float64, device="cuda:0")
    outs = [torch.full((F.batch, plan.m), -7.0, dtype=torch.float64, device="cuda:0") if want else None for want in outputs]
    ptr = [0 if o is None else o.data_ptr() for o in outs]
    F.normalized_residuals_dev(plan, hx.data_ptr(), wd.data_ptr(), rd.data_ptr(), tol, summary.data_ptr(), ptr[0], ptr[1], ptr[2],
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [summary.cpu().numpy()[0]] + [None if o is None else o.cpu().numpy()[0] for o in outs]


def test_normalized_residuals_long_ties_and_nans(gpu):
    """One row past reduce_rows * block rows; a tie takes the lowest row; a NaN residual wins; null outputs."""
    import torch
    case = qc.normres_long()
    mat, m, n = case["matrix"], case["Ct"][0], case["matrix"][1]
    with qc.analysed(case) as F, F.quad_plan(case["Ct"]) as plan:
        F.factor(mat[4])
        Hx, w, r = case["Cx"].copy(), case["w"].copy(), case["r"].copy()
        rn, info = F.normalized_residuals(plan, Hx, w, r, 0.7)
        assert np.array_equal(info["t"], _restated(F, plan, case))
        omega, rn_want, summary = ref.restated_normres(info["t"], w, r, 0.7, qc.LIMITS)
        assert 0 < summary[3] < m, "the case is meant to have critical and other rows at this tolerance"
        assert np.array_equal(info["omega"], omega) and np.array_equal(rn, rn_want)
        assert [info["worst"], info["worst_row"], info["J"], info["critical"]] == summary.tolist()
        for outputs in ((True, True, True), (False, False, False), (False, True, False)):
            got = _normres_dev(torch, F, plan, Hx, w, r, 0.7, outputs)
            assert got[0].tolist() == summary.tolist(), outputs
            for have, want_arr, asked in zip(got[1:], (info["t"], omega, rn), outputs):
                assert (have is None) == (not asked) and (have is None or np.array_equal(have, want_arr))
        # a tie: three rows on one column with the same values, far apart; everything else smaller
        rows = [5 + n * k for k in (1500, 3, 700)]
        r[:] = 0.125 * np.sign(r)
        Hx[rows], w[rows], r[rows] = 1.0, 0.5, -4.0
        rn, info = F.normalized_residuals(plan, Hx, w, r, 1e-3)
        assert rn[rows[0]] == rn[rows[1]] == rn[rows[2]] == rn.max() == info["worst"] and info["worst_row"] == min(rows)
        # a NaN residual ranks above every number, the lowest of two
        r[[60000, 333]] = np.nan
        rn, info = F.normalized_residuals(plan, Hx, w, r, 1e-3)
        assert np.isnan(info["worst"]) and info["worst_row"] == 333 and np.isnan(info["J"]) and np.isnan(rn[[333, 60000]]).all()
        assert np.isfinite(np.delete(rn, [333, 60000])).all()


# -- 5. state and memory

def test_state_and_memory(gpu):
    import torch
    L = gpu.lib()
    case = qc.se(40, 60)
    mat, w = case["matrix"], case["w"]
    live0 = gpu.debug_live_device_buffers()
    F = qc.analysed(case)
    F.factor(mat[4])
    st = torch.cuda.current_stream().cuda_stream
    cx, wd = _dev(torch, case["Cx"]), _dev(torch, w)
    t = torch.zeros(len(w), dtype=torch.float64, device="cuda:0")
    summary = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    plan = F.quad_plan(case["Ct"])
    forms = lambda: L.cs3_quad_dev(F._h, plan._u, cx.data_ptr(), None, t.data_ptr(), st)
    normres = lambda: L.cs3_quad_normres_dev(F._h, plan._u, cx.data_ptr(), wd.data_ptr(), wd.data_ptr(), 1e-8, None, None, None,
                                             summary.data_ptr(), st)
    assert forms() == gpu.CS3_ERR_STATE and normres() == gpu.CS3_ERR_STATE          # before selinv()
    F.selinv(st)
    assert forms() == 0
    torch.cuda.synchronize()
    t0 = t.cpu().numpy().copy()
    counters = F.debug_alloc_counters()
    assert forms() == 0 and normres() == 0 and normres() == 0                       # later calls: nothing allocated, no synchronisation
    assert F.debug_alloc_counters() == counters
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), t0)
    F.solve(np.ones(F.n))                                                           # solves leave Z alone
    assert forms() == 0
    Ax2 = mat[4] * 1.5                                                              # new values: the old Z is refused
    F.factor(Ax2)
    assert forms() == gpu.CS3_ERR_STATE and normres() == gpu.CS3_ERR_STATE
    t_host = F.quad_forms(plan, case["Cx"])                                         # (the host form computes Z)
    assert np.allclose(t_host, t0 / 1.5, rtol=1e-9, atol=0.0)
    assert forms() == 0
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), t_host)
    x = torch.ones(F.n, dtype=torch.float64, device="cuda:0")                       # the fused step invalidates as well
    F.factor_solve_dev(_dev(torch, mat[4]).data_ptr(), x.data_ptr(), 1, stream=st)
    torch.cuda.synchronize()
    assert forms() == gpu.CS3_ERR_STATE
    plan.close()
    F.close()
    assert gpu.debug_live_device_buffers() == live0


@pytest.mark.parametrize("kind", ["chol", "lu"])
def test_memory_goes_with_the_plan(gpu, kind):
    case = dict(qc.se(40, 60), kind=gpu.CS3_CHOLESKY if kind == "chol" else gpu.CS3_LU)
    live0 = gpu.debug_live_device_buffers()
    F = qc.analysed(case)
    F.factor(case["matrix"][4])
    F.selinv()
    live1 = gpu.debug_live_device_buffers()
    plan = F.quad_plan(case["Ct"])
    assert gpu.debug_live_device_buffers() == live1                                 # (the plan is made on the host)
    t = F.quad_forms(plan, case["Cx"])
    F.normalized_residuals(plan, case["Cx"], case["w"], case["w"])                  # the host forms' staging blocks are the plan's too
    assert gpu.debug_live_device_buffers() > live1
    plan.close()
    assert gpu.debug_live_device_buffers() == live1
    plan = F.quad_plan(case["Ct"])                                                  # a plan that outlives its handle
    assert np.array_equal(F.quad_forms(plan, case["Cx"]), t)
    F.close()
    assert gpu.debug_live_device_buffers() == live0
    with pytest.raises(gpu.Cs3Error):
        F2 = qc.analysed(case)
        try:
            gpu._check(gpu.lib().cs3_quad(F2._h, plan._u, gpu._pf(case["Cx"]), None, gpu._pf(t)))
        finally:
            F2.close()
    plan.close()
    assert gpu.debug_live_device_buffers() == live0
