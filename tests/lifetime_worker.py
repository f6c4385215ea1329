"""Worker of tests/test_gpu_lifetime.py: one process that reaches every device-allocation site of the host layer and checks
cs3_debug_live_device_buffers() == 0 before the first call and after the last.  Every call is a supported call or a clean
error return.  Prints the count after each stage; exit status 0 = all assertions held."""
import ctypes as C
import sys

import numpy as np
import scipy.sparse as sp
import torch

from csparse3_amd import csc_hip as hip, synth

live = hip.debug_live_device_buffers
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(11)


def stage(name, want_zero=False):
    n = live()
    print("%-34s live = %d" % (name, n), flush=True)
    assert n >= 0 and (not want_zero or n == 0), (name, n)
    return n


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raises(code, call):
    try:
        call()
    except hip.Cs3Error as e:
        assert e.code == code, (e.code, code, str(e))
        return str(e)
    raise AssertionError("no error")


def diag_cases(rows):
    """One rank-1 modification of a diagonal entry per row: (pattern, values)."""
    rows = np.asarray(rows, dtype=np.int32)
    return (np.arange(len(rows) + 1, dtype=np.int32), rows, rows), np.full(len(rows), 0.125)


assert hip.device_count() >= 1
stage("start", want_zero=True)

# ---- an LU handle with a bottom forest -------------------------------------------------------------------------------
m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=7)
A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
scale = abs(A).sum(axis=0).max()
lib = hip.lib()
lib.cs3_debug_forest.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
lib.cs3_debug_forest.restype = C.c_int64
F = hip.Factorization(m, n, Ap, Ai)
assert lib.cs3_debug_forest(F._h, None, None, None, None) > 0, "this handle must have a bottom forest"
stage("analysed", want_zero=True)
F.factor(Ax, 1e-3)
held = stage("factorised")
assert held > 0, "the counter must move: a factorised handle holds device memory"
for k in (1, 32, 200):                                        # two growths of the sweep buffers
    B = rng.standard_normal((n, k))
    X = F.solve(B)
    assert np.abs(A @ X - B).max() <= 1e-12 * (scale * np.abs(X).max() + np.abs(B).max())
    now = stage("solve, %d right-hand sides" % k)
    assert now > held and (k == 1 or now == grown), "a regrown sweep buffer replaces the old block"
    grown = now
held = grown
b = rng.standard_normal(n)
x = F.solve(b, trans=True)
assert np.abs(A.T @ x - b).max() <= 1e-12 * (scale * np.abs(x).max() + np.abs(b).max())
d_ax, d_b, d_x = t(Ax), t(b), t(b)
F.factor_solve_dev(d_ax.data_ptr(), d_x.data_ptr(), 1, 1e-3, sh)
F.factor_status(sh)
x = d_x.cpu().numpy()
assert np.abs(A @ x - b).max() <= 1e-12 * (scale * np.abs(x).max() + np.abs(b).max())
assert stage("transposed solve, fused step") == held
Lp, Li, Lx, Up, Ui, Ux = F.factors()
held = stage("factors()")
F.factors()
assert stage("factors() again") == held, "the export buffers are built once"
d_r = torch.empty_like(d_b)
F.residual_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), 1, sh)
stage("residual_dev")
F.refine_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, 1, sh)
stage("refine_dev")
d_xt = t(F.solve(b, trans=True))
F.refine_dev(d_ax.data_ptr(), d_b.data_ptr(), d_xt.data_ptr(), 1, 1, sh, trans=True)
held = stage("refine_t_dev")
d_B3, d_X3 = t(rng.standard_normal((n, 3))), t(np.zeros((n, 3)))
F.refine_dev(d_ax.data_ptr(), d_B3.data_ptr(), d_X3.data_ptr(), 3, 2, sh)
assert stage("refine_dev, 3 right-hand sides") == held, "a regrown residual replaces the old block"
cond, inv_norm = F.condest(Ax)
stage("condest")
d_c = torch.empty(2, dtype=torch.float64, device=dev)
F.condest_dev(d_ax.data_ptr(), d_c.data_ptr(), d_c.data_ptr() + 8, sh)
torch.cuda.synchronize()
assert np.array_equal(d_c.cpu().numpy(), [cond[0], inv_norm[0]])
sign, logabs = F.slogdet()
assert sign[0] in (-1.0, 1.0) and np.isfinite(logabs[0])
held = stage("condest_dev, slogdet")

pat1, cx1 = diag_cases(np.arange(10) * 7)                    # 10 touched rows: a tile of 64 columns
pat2, cx2 = diag_cases(np.arange(100) * 13)                  # 100 touched rows: 128 columns, Z regrows
plan1 = F.updates_plan(pat1)
X1, rpiv1 = F.solve_updates(plan1, cx1, b)
with_plan = stage("updates, host form")
assert with_plan > held
d_X1 = torch.empty((n, 10), dtype=torch.float64, device=dev)
d_cx1 = t(cx1)
F.solve_updates_dev(plan1, d_cx1.data_ptr(), d_b.data_ptr(), d_X1.data_ptr(), 0, 0.0, sh)
torch.cuda.synchronize()
assert np.array_equal(d_X1.cpu().numpy(), X1)
assert stage("updates, device form") == with_plan, "the device form needs nothing the host form has not built"
plan2 = F.updates_plan(pat2)
X2, _ = F.solve_updates(plan2, cx2, b)
assert np.allclose(X2[:, 0], X1[:, 0], rtol=1e-10, atol=0.0)   # (both lists begin with the same case)
both = stage("a wider plan")
assert both > with_plan
plan1.close()                                                # a plan closed before its handle
one = stage("first plan closed")
assert held < one < both
raises(hip.CS3_ERR_PIVOT, lambda: F.factor(np.zeros_like(Ax), 1e-3))     # a factorisation that stops at a rejected pivot
assert stage("rejected pivot") == one
F.close()                                                    # a handle closed before its plan: the plan holds no HBM
stage("handle closed", want_zero=True)
plan2.close()
stage("second plan closed", want_zero=True)

# ---- a batched Cholesky handle on the interleaved pool ---------------------------------------------------------------
ei, ej = synth.spd_grid_pattern(200, seed=200)
sm, sn, Sp, Si, Sx = synth.spd_grid_matrix(200, ei, ej, seed=201)
nb = 128                                                     # (the pool is interleaved from 128 matrices on)
SX = Sx[None, :] * (1.0 + rng.uniform(0.0, 1.0, size=(nb, 1)))
with hip.Factorization(sm, sn, Sp, Si, kind=hip.CS3_CHOLESKY, batch=nb) as G:
    G.factor(SX)
    room = torch.empty(nb * int(G.info.factor_bytes) // 8, dtype=torch.float64, device=dev)    # (what an export would fill)
    assert "interleaved" in raises(hip.CS3_ERR_STATE, lambda: G.export_factor_dev(room.data_ptr(), sh)), \
        "this handle must use the interleaved pool"
    Bb = rng.standard_normal((nb, sn, 2))
    Xb = G.solve(Bb)
    S63 = sp.csc_matrix((SX[63], Si, Sp), shape=(sn, sn))
    assert np.abs(S63 @ Xb[63] - Bb[63]).max() <= 1e-11 * np.abs(Bb[63]).max() * sn
    G.factors(b=63)
    G.condest(SX)
    G.slogdet()
    assert stage("Cholesky batch of 128") > 0
stage("Cholesky batch closed", want_zero=True)

# ---- the stand-alone functions, and their error returns behind an allocation -----------------------------------------
for fn, (Gp, Gi, Gx) in ((hip.csc_lsolve_f, (Lp, Li, Lx)), (hip.csc_usolve_f, (Up, Ui, Ux)),
                         (hip.csc_ltsolve_f, (Lp, Li, Lx)), (hip.csc_utsolve_f, (Up, Ui, Ux))):
    fn(n, Gp, Gi, Gx, rng.standard_normal((n, 2)))
assert np.array_equal(hip.csc_mat_vec_ff(m, n, Ap, Ai, Ax, b), hip.csc_mat_vec_ff(m, n, Ap, Ai, Ax, b))
stage("triangular solves, matvec", want_zero=True)
blk = (m, n, Ai, Ap, Ax)
pm, pn, Pi, Pp, Px = hip.csc_stack_4_by_4_ff(*(blk * 4))
assert (pm, pn, len(Pi)) == (2 * m, 2 * n, 4 * len(Ai))
tn, tm, Tp, Ti, Tx = hip.csc_transpose(m, n, Ap, Ai, Ax)
assert abs(sp.csc_matrix((Tx, Ti, Tp), shape=(n, m)) - A.T).nnz == 0
coo = A.tocoo()
hip.coo_to_csc(m, n, coo.row, coo.col, coo.data, coo.nnz)
assert np.isclose(hip.csc_norm(n, Ap, Ax), scale, rtol=1e-14)
hip.csc_add_ff(m, n, Ap, Ai, Ax, m, n, Tp, Ti, Tx, 1.0, -0.5)
every = np.arange(n, dtype=np.int32)
nz, _, _, _ = hip.csc_sub_matrix(m, int(Ap[n]), Ap, Ai, Ax, every, every)
assert nz == int(Ap[n])
assert len(hip.find_islands(n, Ap, Ai)) >= 1
stage("stack, conversions, utilities", want_zero=True)
assert "room for" in raises(hip.CS3_ERR_ARG, lambda: hip.csc_sub_matrix(m, int(Ap[n]), Ap, Ai, Ax, np.r_[every, every], every))
bad = Ai.copy()
bad[5] = m + 3
assert "out of range" in raises(hip.CS3_ERR_ARG, lambda: hip.csc_transpose(m, n, Ap, bad, Ax))
badc = coo.col.astype(np.int32)
badc[5] = n + 3
assert "out of range" in raises(hip.CS3_ERR_ARG, lambda: hip.coo_to_csc(m, n, coo.row, badc, coo.data, coo.nnz))
stage("error returns", want_zero=True)
print("lifetime ok")
sys.exit(0)
