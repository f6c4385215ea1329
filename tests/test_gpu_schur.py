"""Schur handles on the GPU: factor the interior, return the dense border (cs3_analyze_schur, k_schur_take, the half-solves).

Reference: NumPy float64, dense, S = A22 - A21 @ solve(A11, A12) with the blocks in the caller's list order
(tests/schur_cases.py); tolerance helpers.RTOL, norm-wise (helpers.rel_err).  The LDS is poisoned before the numeric calls."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import schur_cases as sc
from helpers import RTOL, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def poisoned(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check_S(S, want, what):
    assert S.shape == want.shape, what
    assert np.isfinite(S).all(), what + ": non-finite entries"
    err = rel_err(S, want)
    print("%s: rel.err %.3e" % (what, err))
    assert err <= RTOL, "%s: relative error %.3e > %.1e" % (what, err, RTOL)


# --------------------------------------------------------------------------------------------------------- S, LU --

LU_CASES = [("toy10", 3)] + [("grid2k", ns) for ns in (1, 31, 32, 33, 64, 65, 136, 137, 200)] + \
           [("denseblock300", 150), ("grid20k", 300)]


@pytest.mark.parametrize("name,ns", LU_CASES)
def test_schur_complement_lu(gpu, name, ns):
    m, n, Ap, Ai, Ax = sc.matrix(name)
    idx = sc.schur_set(name, ns)
    with gpu.Factorization(m, n, Ap, Ai, schur=idx) as F:
        S = F.factor(Ax).schur()
        assert np.array_equal(F.schur_info(), idx)
        assert int(F.info.fail_col) == -1
    _check_S(S, sc.reference_of(name, ns), "%s ns %d" % (name, ns))


def test_cscmat_schur_complement(gpu):
    from csparse3_amd.csc import CscMat
    m, n, Ap, Ai, Ax = sc.matrix("grid2k")
    A = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    _check_S(A.schur_complement(sc.schur_set("grid2k", 33)), sc.reference_of("grid2k", 33), "CscMat.schur_complement")
    F = A.lu(schur=sc.schur_set("grid2k", 33))
    _check_S(F.schur(), sc.reference_of("grid2k", 33), "CscMat.lu(schur=)")
    ms, nsp, Sp, Si, Sx = sc.matrix("spd200")
    B = CscMat(ms, nsp, indptr=Sp, indices=Si, data=Sx)
    _check_S(B.schur_complement(sc.schur_set("spd200", 20), kind="chol"), sc.reference_of("spd200", 20), "chol")


# --------------------------------------------------------------------------------------------------- S, Cholesky --

@pytest.mark.parametrize("name,ns", [("spd200", 20), ("spd4000", 137), ("spd4000_lower", 137)])
def test_schur_complement_cholesky(gpu, name, ns):
    m, n, Ap, Ai, Ax = sc.matrix(name)
    idx = sc.schur_set(name, ns)
    with gpu.Factorization(m, n, Ap, Ai, gpu.CS3_CHOLESKY, schur=idx) as F:
        S = F.factor(Ax).schur()
    assert np.array_equal(S, S.T), "S is not symmetric bit for bit"
    _check_S(S, sc.reference_of(name, ns), "%s ns %d" % (name, ns))


# -------------------------------------------------------------------------------- what no plain handle factorises --

def test_saddle_point_constraints_as_schur_set(gpu):
    n, Ap, Ai, Ax, con, H, G = sc.saddle_point()
    with gpu.Factorization(n, n, Ap, Ai, schur=con) as F:
        S = F.factor(Ax, 1e-3).schur()
    want = -G @ np.linalg.solve(H.toarray(), G.T)
    _check_S(S, want, "saddle point")
    with gpu.Factorization(n, n, Ap, Ai) as P:
        with pytest.raises(gpu.SingularMatrix) as e:
            P.factor(Ax, 1e-3)
        assert e.value.code == gpu.CS3_ERR_PIVOT


# ----------------------------------------------------------------------------------------------------- half-solves --

HALF = {"grid2k": (65, 0), "spd4000": (137, 1)}


@pytest.fixture(scope="module")
def half_handles(gpu):
    held = {}
    for name, (ns, kind) in HALF.items():
        m, n, Ap, Ai, Ax = sc.matrix(name)
        idx = sc.schur_set(name, ns)
        F = gpu.Factorization(m, n, Ap, Ai, kind, schur=idx)
        F.factor(Ax)
        A = sc.to_scipy(n, Ap, Ai, Ax)
        held[name] = (F, A, idx, F.schur(), spla.splu(A.tocsc()))
    yield held
    for F, *_ in held.values():
        F.close()


@pytest.mark.parametrize("name", list(HALF))
@pytest.mark.parametrize("k", [1, 5, 16, 64, 130])
def test_half_solves(gpu, half_handles, name, k):
    import torch
    F, A, idx, S, lu = half_handles[name]
    n = A.shape[0]
    rng = np.random.default_rng(100 + k)
    B = rng.standard_normal(n) if k == 1 else rng.standard_normal((n, k))
    want_g = sc.condensed_rhs(A, idx, B)
    want_x = lu.solve(B)
    sh = torch.cuda.current_stream().cuda_stream

    def round_trip():
        d = torch.from_numpy(B.copy()).to("cuda:0")
        F.schur_forward_dev(d.data_ptr(), k, sh)
        Y = d.cpu().numpy()
        Z = Y.copy()
        Z[idx] = np.linalg.solve(S, Y[idx])
        d2 = torch.from_numpy(Z).to("cuda:0")
        F.schur_backward_dev(d2.data_ptr(), k, sh)
        return Y, d2.cpu().numpy()

    Y, X = round_trip()
    e_g, e_x = rel_err(Y[idx], want_g), rel_err(X, want_x)
    print("%s k %d: condensed rhs %.3e, solution %.3e" % (name, k, e_g, e_x))
    assert e_g <= RTOL, "condensed right-hand side: %.3e" % e_g
    assert e_x <= RTOL, "solution: %.3e" % e_x
    # from the second call with this k on: no allocation, no synchronisation
    torch.cuda.synchronize()
    d = torch.from_numpy(B.copy()).to("cuda:0")
    before = F.debug_alloc_counters()
    F.schur_forward_dev(d.data_ptr(), k, sh)
    F.schur_backward_dev(d.data_ptr(), k, sh)
    after = F.debug_alloc_counters()
    torch.cuda.synchronize()
    assert after == before, (before, after)
    # the host forms: the same kernels, the same bits
    Yh = F.schur_forward(B)
    assert _bits_equal(Yh, Y)
    Zh = Yh.copy()
    Zh[idx] = np.linalg.solve(S, Yh[idx])
    assert _bits_equal(F.schur_backward(Zh), X)


# ------------------------------------------------------------------------------------------------ refactorisation --

def test_three_factorisations_on_one_handle(gpu):
    m, n, Ap, Ai, Ax = sc.matrix("grid2k")
    idx = sc.schur_set("grid2k", 33)
    got = []
    with gpu.Factorization(m, n, Ap, Ai, schur=idx) as F:
        for t in (1, 2, 3):
            vals = sc.varied(Ax, t)
            S = F.factor(vals).schur()
            _check_S(S, sc.reference(sc.to_scipy(n, Ap, Ai, vals), idx), "factorisation %d" % t)
            got.append(S)
        assert not _bits_equal(got[0], got[1]) and not _bits_equal(got[1], got[2])
    with gpu.Factorization(m, n, Ap, Ai, schur=idx) as F2:
        assert _bits_equal(F2.factor(sc.varied(Ax, 3)).schur(), got[2]), "a fresh handle gives other bits"


# -------------------------------------------------------------------------------------------------------- batches --

def test_batch_of_three_lu(gpu):
    m, n, Ap, Ai, Ax = sc.matrix("grid2k")
    idx = sc.schur_set("grid2k", 33)
    vals = np.stack([sc.varied(Ax, t) for t in range(3)])
    with gpu.Factorization(m, n, Ap, Ai, schur=idx, batch=3) as F:
        S = F.factor(vals).schur()
    assert S.shape == (3, 33, 33)
    for t in range(3):
        _check_S(S[t], sc.reference(sc.to_scipy(n, Ap, Ai, vals[t]), idx), "grid2k batch 3, matrix %d" % t)


@pytest.mark.parametrize("batch", [48, 130])
def test_batches_of_cholesky(gpu, batch):
    m, n, Ap, Ai, _ = sc.matrix("spd200")
    idx = sc.schur_set("spd200", 20)
    vals = np.stack([sc.spd_values(n, t) for t in range(batch)])
    with gpu.Factorization(m, n, Ap, Ai, gpu.CS3_CHOLESKY, schur=idx, batch=batch) as F:
        S = F.factor(vals).schur()
    assert S.shape == (batch, 20, 20)
    worst = 0.0
    for t in range(batch):
        assert np.array_equal(S[t], S[t].T)
        want = sc.reference(sc.to_scipy(n, Ap, Ai, vals[t]), idx)
        assert np.isfinite(S[t]).all()
        worst = max(worst, rel_err(S[t], want))
    print("spd200 batch %d: worst rel.err %.3e" % (batch, worst))
    assert worst <= RTOL


# -------------------------------------------------------------------------------------------------------- slogdet --

@pytest.mark.parametrize("name,ns,kind", [("grid2k", 65, 0), ("spd200", 20, 1)])
def test_slogdet_is_that_of_the_interior(gpu, name, ns, kind):
    m, n, Ap, Ai, Ax = sc.matrix(name)
    idx = sc.schur_set(name, ns)
    inter, _ = sc.split(n, idx)
    want_sign, want_log = np.linalg.slogdet(sc.to_scipy(n, Ap, Ai, Ax).tocsr()[inter][:, inter].toarray())
    with gpu.Factorization(m, n, Ap, Ai, kind, schur=idx) as F:
        sign, logabs = F.factor(Ax).slogdet()
    assert sign[0] == want_sign
    assert abs(logabs[0] - want_log) <= RTOL * max(1.0, abs(want_log)), (logabs[0], want_log)


# --------------------------------------------------------------------------------------------------- perturbation --

def test_perturbed_interior_pivot_next_to_the_border(gpu):
    n, Ap, Ai, Ax, idx, v = sc.pendant_zero()
    delta = 0.05
    with gpu.Factorization(n, n, Ap, Ai, schur=idx) as F:
        col = int(F.ordering()["pinv"][v])
        with pytest.raises(gpu.SingularMatrix) as e:
            F.factor(Ax)
        assert e.value.code == gpu.CS3_ERR_PIVOT
        assert int(F.info.fail_col) == col
        S = F.set_perturbation(delta).factor(Ax).schur()
        assert F.perturbed().tolist() == [1]
    A = sc.to_scipy(n, Ap, Ai, Ax).tolil()
    A[v, v] = delta
    _check_S(S, sc.reference(A.tocsc(), idx), "perturbed")


# ----------------------------------------------------------------------------------------- refusals and lifetime --

def test_refused_entry_points_and_state(gpu):
    import torch
    m, n, Ap, Ai, Ax = sc.matrix("toy10")
    lib = gpu.lib()
    f64p = C.POINTER(C.c_double)
    x = np.ones(n)
    d_x = torch.ones(n, dtype=torch.float64, device="cuda:0")
    d_b = torch.ones(n, dtype=torch.float64, device="cuda:0")
    d_ax = torch.from_numpy(np.asarray(Ax, dtype=np.float64).copy()).to("cuda:0")
    d_out = torch.zeros(4 * n * n, dtype=torch.float64, device="cuda:0")
    vp = C.c_void_p
    with gpu.Factorization(m, n, Ap, Ai, schur=[7, 2, 5]) as F:
        h = F._h
        S = np.zeros((3, 3))
        # before a factorisation: CS3_ERR_STATE
        assert lib.cs3_schur_get(h, S.ctypes.data_as(f64p)) == gpu.CS3_ERR_STATE
        assert lib.cs3_schur_get_dev(h, vp(d_out.data_ptr()), None) == gpu.CS3_ERR_STATE
        for fn in (lib.cs3_schur_fwd, lib.cs3_schur_bwd):
            assert fn(h, x.ctypes.data_as(f64p), 1) == gpu.CS3_ERR_STATE
        for fn in (lib.cs3_schur_fwd_dev, lib.cs3_schur_bwd_dev):
            assert fn(h, vp(d_x.data_ptr()), 1, None) == gpu.CS3_ERR_STATE
        F.factor(Ax)
        xp, axp = x.ctypes.data_as(f64p), np.asarray(Ax, dtype=np.float64).ctypes.data_as(f64p)
        dx, db, dax, dout = vp(d_x.data_ptr()), vp(d_b.data_ptr()), vp(d_ax.data_ptr()), vp(d_out.data_ptr())
        corr = C.c_double(0.0)
        plan = vp()
        i32 = lambda *a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
        refused = {
            "cs3_solve": lambda: lib.cs3_solve(h, xp, 1),
            "cs3_solve_t": lambda: lib.cs3_solve_t(h, xp, 1),
            "cs3_lsolve": lambda: lib.cs3_lsolve(h, xp, 1),
            "cs3_usolve": lambda: lib.cs3_usolve(h, xp, 1),
            "cs3_ltsolve": lambda: lib.cs3_ltsolve(h, xp, 1),
            "cs3_utsolve": lambda: lib.cs3_utsolve(h, xp, 1),
            "cs3_solve_dev": lambda: lib.cs3_solve_dev(h, dx, 1, None),
            "cs3_solve_t_dev": lambda: lib.cs3_solve_t_dev(h, dx, 1, None),
            "cs3_lsolve_dev": lambda: lib.cs3_lsolve_dev(h, dx, 1, None),
            "cs3_usolve_dev": lambda: lib.cs3_usolve_dev(h, dx, 1, None),
            "cs3_ltsolve_dev": lambda: lib.cs3_ltsolve_dev(h, dx, 1, None),
            "cs3_utsolve_dev": lambda: lib.cs3_utsolve_dev(h, dx, 1, None),
            "cs3_factor_solve_dev": lambda: lib.cs3_factor_solve_dev(h, dax, 0.0, dx, 1, None),
            "cs3_factor_solve_bx_dev": lambda: lib.cs3_factor_solve_bx_dev(h, dax, 0.0, db, dx, 1, None),
            "cs3_refine": lambda: lib.cs3_refine(h, axp, xp, xp, 1, 1, C.byref(corr)),
            "cs3_refine_dev": lambda: lib.cs3_refine_dev(h, dax, db, dx, 1, 1, C.byref(corr), None),
            "cs3_refine_t_dev": lambda: lib.cs3_refine_t_dev(h, dax, db, dx, 1, 1, C.byref(corr), None),
            "cs3_condest": lambda: lib.cs3_condest(h, axp, xp, None),
            "cs3_condest_dev": lambda: lib.cs3_condest_dev(h, dax, dout, None, None),
            "cs3_updates_plan": lambda: lib.cs3_updates_plan(h, 1, i32(0, 1), i32(0), i32(1), C.byref(plan)),
            "cs3_get_factors": lambda: lib.cs3_get_factors(h, 0, None, None, None, None, None, None),
            "cs3_export_factor_dev": lambda: lib.cs3_export_factor_dev(h, dout, None),
            "cs3_import_factor_dev": lambda: lib.cs3_import_factor_dev(h, dout, None),
        }
        for name, call in refused.items():
            assert call() == gpu.CS3_ERR_ARG, name
            assert "Schur handle" in lib.cs3_last_error().decode(), name
        # and the handle still answers afterwards
        _check_S(F.schur(), sc.reference_of("toy10", 3), "toy10 after the refusals")
        torch.cuda.synchronize()
        S_dev = torch.zeros((3, 3), dtype=torch.float64, device="cuda:0")
        F.schur_dev(S_dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _bits_equal(S_dev.cpu().numpy(), F.schur())
    # a plain handle has no Schur set
    with gpu.Factorization(m, n, Ap, Ai) as P:
        P.factor(Ax)
        assert lib.cs3_schur_get(P._h, S.ctypes.data_as(f64p)) == gpu.CS3_ERR_STATE
        assert lib.cs3_schur_fwd(P._h, x.ctypes.data_as(f64p), 1) == gpu.CS3_ERR_STATE


def test_device_buffers_are_released(gpu):
    import torch
    m, n, Ap, Ai, Ax = sc.matrix("grid2k")
    torch.cuda.synchronize()
    before = gpu.debug_live_device_buffers()
    F = gpu.Factorization(m, n, Ap, Ai, schur=sc.schur_set("grid2k", 65))
    F.factor(Ax).schur()
    F.schur_backward(F.schur_forward(np.ones((n, 16))))
    assert gpu.debug_live_device_buffers() > before
    F.close()
    assert gpu.debug_live_device_buffers() == before
