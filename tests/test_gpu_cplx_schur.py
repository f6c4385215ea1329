"""Complex Schur handles (Kron reduction) on the GPU: S = A22 - A21 A11^-1 A12 of a complex matrix from a real Schur handle
on its real form, with border rows that are never rotated.

S against NumPy complex128, elementwise within 1e3 cond(A11) 2^-53 (|A22| + |A21| |A11^-1| |A12|); S bit for bit the first
column of the 2 x 2 blocks of the real handle's Schur complement, the twin column within the same bound; the half-solves
around a dense solve of S against the solve of a plain complex handle; Cholesky, a lossless network with zero border
diagonals, a batch, rotation on and off, the refusals."""
import numpy as np
import pytest

import cplx_cases
import cplx_ref as ref
import csens_cases as cc
import csens_ref as cr
from csparse3_amd import synth

pytestmark = pytest.mark.gpu

N40 = 40
BORDERS = {"five": cc.BORDER, "one": [17], "n_minus_1": [b for b in range(N40) if b != 22], "unsorted": [9, 2, 30, 1]}
EPS = 2.0 ** -53


def check_s(F, n, Ap, Ai, Az, border, S, SR, what):
    """One matrix: S against the definition, against the real handle's blocks, and its twin column."""
    want, size, cond = cr.schur_dense(ref.dense_complex(n, Ap, Ai, Az), border)
    tol = 1e3 * cond * EPS * size
    err = np.abs(S - want)
    ratio = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)       # (a structural zero of S: 0 <= 0)
    print("%s: max |S - S_np| / bound = %.3e (cond(A11) %.2e)" % (what, ratio.max(), cond))
    assert S.shape == want.shape and np.all(err <= tol), what
    assert cr.same(S, SR[0::2, 0::2] + 1j * SR[1::2, 0::2]), what + ": S is not the first column of the real blocks"
    twin = SR[1::2, 1::2] - 1j * SR[0::2, 1::2]
    assert np.all(np.abs(twin - want) <= tol), what + ": the twin column"
    return tol


@pytest.mark.parametrize("border", sorted(BORDERS))
def test_s_against_numpy_and_the_real_handle(gpu, border):
    import torch
    n, Ap, Ai, Az = cc.ybus40()
    idx = BORDERS[border]
    ns = len(idx)
    with gpu.ComplexFactorization(n, Ap, Ai, schur=idx) as F:
        assert F.ns == ns and np.array_equal(F.schur_info(), idx) and np.array_equal(F.real.schur_info(), ref.doubled_order(idx))
        F.factor(Az)
        # the border was not rotated, every other row was
        Azr, Azi = ref.split(Az, (1, -1))
        s = F.plan.rotation()
        assert cr.same(s, ref.join(*cr.rotation_with_border(n, Ap, Ai, Azr, Azi, True, idx)))
        assert np.all(s[0, idx] == 1.0) and np.all(s[0, np.setdiff1d(np.arange(n), idx)] != 1.0)
        S = F.schur()
        assert S.shape == (ns, ns) and S.dtype == np.complex128
        check_s(F, n, Ap, Ai, Az, idx, S, F.real.schur(), border)
        # the device form: the same bits, nothing behind the array
        d_s = torch.full((ns * ns + 1,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda:0")
        F.schur_dev(d_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_s.cpu().numpy()
        assert np.isnan(got[-1]) and cr.same(got[:-1].reshape(ns, ns), S)
        with pytest.raises(gpu.Cs3Error) as e:
            F.schur_dev(d_s.data_ptr() + 8)
        assert e.value.code == gpu.CS3_ERR_ARG and "16 bytes" in str(e.value)


def residual_bound(n, Ap, Az, x, b):
    return 1e-12 * (cplx_cases.norm1(n, Ap, Az) * np.abs(x).max() + np.abs(b).max())


@pytest.mark.parametrize("border", ["five", "unsorted", "one"])
@pytest.mark.parametrize("k", [1, 3])
def test_half_solves_around_a_dense_solve_of_s_solve_the_system(gpu, border, k):
    import torch
    n, Ap, Ai, Az = cc.ybus40()
    idx = np.array(BORDERS[border])
    A = ref.dense_complex(n, Ap, Ai, Az)
    rng = np.random.default_rng(5 + k)
    b = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    with gpu.ComplexFactorization(n, Ap, Ai, schur=idx) as F, gpu.ComplexFactorization(n, Ap, Ai) as P:
        F.factor(Az)
        x_plain = P.factor(Az).solve(b)
        y = F.schur_forward(b)
        interior = np.setdiff1d(np.arange(n), idx)
        want_g = b[idx] - A[np.ix_(idx, interior)] @ np.linalg.solve(A[np.ix_(interior, interior)], b[interior])
        assert np.abs(y[idx] - want_g).max() <= 1e-10 * np.abs(want_g).max()
        y[idx] = np.linalg.solve(F.schur(), y[idx])
        x = F.schur_backward(y)
        bound = residual_bound(n, Ap, Az, x, b)
        res, res_plain = np.abs(b - A @ x).max(), np.abs(b - A @ x_plain).max()
        print("border %s k=%d: residual %.3e (plain handle %.3e), bound %.3e" % (border, k, res, res_plain, bound))
        assert x.shape == b.shape and res <= bound and res_plain <= bound
        assert np.abs(A @ (x - x_plain)).max() <= 2 * bound
        # the device forms give the same bits, in place too
        st = torch.cuda.current_stream().cuda_stream
        d_b = torch.from_numpy(b).to("cuda:0")
        d_y = torch.empty_like(d_b)
        F.schur_forward_dev(d_b.data_ptr(), d_y.data_ptr(), k, st)
        torch.cuda.synchronize()
        y_dev = d_y.cpu().numpy()
        assert cr.same(y_dev, F.schur_forward(b)) and cr.same(d_b.cpu().numpy(), b)
        d_y = torch.from_numpy(y).to("cuda:0")
        F.schur_backward_dev(d_y.data_ptr(), d_y.data_ptr(), k, st)
        torch.cuda.synchronize()
        assert cr.same(d_y.cpu().numpy(), x)
        # what a Schur handle refuses, it refuses here too, in the real handle's words
        with pytest.raises(gpu.Cs3Error) as e:
            F.solve(b)
        assert e.value.code == gpu.CS3_ERR_ARG and "not available on a Schur handle" in str(e.value)
        with pytest.raises(gpu.Cs3Error) as e:
            F.solve_dev(d_b.data_ptr(), d_y.data_ptr(), k, st)
        assert "not available on a Schur handle" in str(e.value)


def test_cholesky_gives_a_hermitian_s_and_lu_without_rotation_the_same_matrix(gpu):
    n, Ap, Ai, Az = cplx_cases.hermitian_pd(40, 60, seed=3)
    idx = cc.BORDER
    with gpu.ComplexFactorization(n, Ap, Ai, kind=gpu.CS3_CHOLESKY, rotate=False, schur=idx) as F:
        S = F.factor(Az).schur()
        tol = check_s(F, n, Ap, Ai, Az, idx, S, F.real.schur(), "cholesky")
        # the real S is symmetric bit for bit: so are the real parts; the imaginary parts are the twin column's, to rounding
        assert np.array_equal(S.real, S.real.T) and np.all(np.abs(S - S.conj().T) <= 2 * tol)
        assert np.linalg.eigvalsh((S + S.conj().T) / 2).min() > 0
    for rotate in (False, True):
        with gpu.ComplexFactorization(n, Ap, Ai, rotate=rotate, schur=idx) as G:
            S_lu = G.factor(Az).schur()
            check_s(G, n, Ap, Ai, Az, idx, S_lu, G.real.schur(), "lu, rotate=%s" % rotate)
            assert np.all(np.abs(S_lu - S) <= 2 * tol)
            if rotate:                                          # a real positive diagonal: s = (1, -0) on the interior, nothing turns
                assert np.all(G.plan.rotation().real == 1.0)


def test_a_lossless_network_with_zero_border_diagonals(gpu):
    """The border is never pivoted: a zero diagonal there is no obstacle, with the rotation taking care of the interior."""
    n, Ap, Ai, Az = synth.ybus(40, 60, seed=40, lossless=True)
    idx = cc.BORDER
    col = np.repeat(np.arange(n), np.diff(Ap))
    Az = Az.copy()
    Az[(Ai == col) & np.isin(col, idx)] = 0.0
    assert not Az.real.any()
    with gpu.ComplexFactorization(n, Ap, Ai, schur=idx) as F:
        S = F.factor(Az).schur()
        check_s(F, n, Ap, Ai, Az, idx, S, F.real.schur(), "lossless")
    with gpu.ComplexFactorization(n, Ap, Ai, rotate=False, schur=idx) as F:
        with pytest.raises(gpu.SingularMatrix):                    # without the rotation the first interior pivot is Re d = 0
            F.factor(Az)


def test_a_batch_of_three(gpu):
    n, Ap, Ai, Az = cc.ybus40()
    idx = BORDERS["unsorted"]
    rng = np.random.default_rng(9)
    Az3 = np.stack([Az, Az * (1.0 + 0.2 * rng.uniform(-1, 1, len(Az))) + 0.05 * rng.uniform(0, 1, len(Az)),
                    Az * (1.0 + 0.2 * rng.uniform(-1, 1, len(Az))) - 0.05j * rng.uniform(0, 1, len(Az))])
    with gpu.ComplexFactorization(n, Ap, Ai, batch=3, schur=idx) as F:
        S = F.factor(Az3).schur()
        SR = F.real.schur()
        assert S.shape == (3, len(idx), len(idx))
        for m in range(3):
            check_s(F, n, Ap, Ai, Az3[m], idx, S[m], SR[m], "matrix %d of the batch" % m)
        assert not np.array_equal(S[0], S[1]) and not np.array_equal(S[1], S[2])
        b = rng.standard_normal((3, n, 2)) + 1j * rng.standard_normal((3, n, 2))
        y = F.schur_forward(b)
        for m in range(3):
            y[m, idx] = np.linalg.solve(S[m], y[m, idx])
        x = F.schur_backward(y)
        for m in range(3):
            A = ref.dense_complex(n, Ap, Ai, Az3[m])
            assert np.abs(b[m] - A @ x[m]).max() <= residual_bound(n, Ap, Az3[m], x[m], b[m])


def test_what_does_not_fit_is_refused(gpu):
    n, Ap, Ai, Az = cc.ybus40()
    S = np.empty((5, 5), dtype=np.complex128)
    L = gpu.lib()
    with gpu.ComplexFactorization(n, Ap, Ai, schur=cc.BORDER) as F, gpu.ComplexFactorization(n, Ap, Ai) as P, \
            gpu.ComplexFactorization(n, Ap, Ai, schur=[1, 2]) as G:
        with pytest.raises(gpu.Cs3Error) as e:                     # before a factorisation
            F.schur()
        assert e.value.code == gpu.CS3_ERR_STATE
        F.factor(Az)
        P.factor(Az)
        G.factor(Az)
        assert L.cs3_cplx_schur_get(F.plan._p, None, gpu._pc(S)) == gpu.CS3_ERR_ARG
        assert L.cs3_cplx_schur_get(None, F.real._h, gpu._pc(S)) == gpu.CS3_ERR_ARG
        assert L.cs3_cplx_schur_get(F.plan._p, P.real._h, gpu._pc(S)) == gpu.CS3_ERR_STATE and "no Schur set" in L.cs3_last_error().decode()
        assert L.cs3_cplx_schur_get(F.plan._p, F.real._h, None) == gpu.CS3_ERR_ARG
        assert L.cs3_cplx_schur_get(P.plan._p, F.real._h, gpu._pc(S)) == gpu.CS3_ERR_STATE and "no border" in L.cs3_last_error().decode()
        assert L.cs3_cplx_schur_get(G.plan._p, F.real._h, gpu._pc(S)) == gpu.CS3_ERR_ARG and "2 ns" in L.cs3_last_error().decode()
        assert F.schur().shape == (5, 5)
