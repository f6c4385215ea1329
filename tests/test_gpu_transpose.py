"""Transposed solves A' x = b on the factors a handle already holds, against the CPU oracle.

The oracle's x is  x = P' (L' \\ (U' \\ (Q' b)))  on the oracle's own factors with the handle's column order:
pvec(q) -> csc_utsolve_f -> csc_ltsolve_f -> pinv.  Solutions within 1e-10 relative, as the plain solves.
"""
import numpy as np
import pytest

from csparse3_amd import synth
from helpers import RTOL, csc_to_scipy, rel_err
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu


def _oracle_solve_t(orc, n, Ap, Ai, Ax, q, B, tol=1e-3):
    """A' X = B column by column through the oracle's transposed sweeps."""
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, tol)
    B2 = B.reshape(n, -1)
    X = np.empty_like(B2)
    for t in range(B2.shape[1]):
        c = np.ascontiguousarray(B2[q, t])
        orc.csc_utsolve_f(n, Up, Ui, Ux, c)
        orc.csc_ltsolve_f(n, Lp, Li, Lx, c)
        X[:, t] = c[pinv]
    return X.reshape(B.shape)


def _rhs(n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)) if k > 1 else rng.standard_normal(n)


def _residual_ok(A, X, B):
    R = A.T @ X - B
    return np.abs(R).max() <= 1e-12 * (abs(A).sum(axis=1).max() * np.abs(X).max() + np.abs(B).max())


def test_transposed_solve_matches_oracle(gpu, orc):
    """Every case, k in {1, 5, 16, 70, 128}: wave (1 / 8 right-hand sides), block, big, lane = right-hand side and
    GEMM sweeps.  The transposed result must differ from the plain one (a path that ignores the flag fails)."""
    differs = False
    for name, (m, n, Ap, Ai, Ax) in CASES.items():
        A = csc_to_scipy(m, n, Ap, Ai, Ax)
        with gpu.Factorization(m, n, Ap, Ai) as F:
            F.factor(Ax, 1e-3)
            q = F.ordering()["q"]
            for k in (1, 5, 16, 70, 128):
                B = _rhs(n, k, 10 + k)
                X = F.solve(B, trans=True)
                want = _oracle_solve_t(orc, n, Ap, Ai, Ax, q, B)
                err = rel_err(X, want)
                assert err <= RTOL, "%s k=%d: relative error %.3e" % (name, k, err)
                assert _residual_ok(A, X, B), "%s k=%d: residual" % (name, k)
                Xp = F.solve(B)
                differs = differs or rel_err(X, Xp) > 1e-2
    assert differs, "solve(trans=True) gave what solve() gives on every case"


@pytest.mark.parametrize("name", ["toy10", "jacobian118", "grid2k", "denseblock150"])
def test_utsolve_ltsolve_on_the_handle_match_oracle(gpu, orc, name):
    m, n, Ap, Ai, Ax = CASES[name]
    rng = np.random.default_rng(5)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        Lp, Li, Lx, Up, Ui, Ux = F.factors()
        b = rng.standard_normal(n)
        y = F.utsolve(b)
        x = F.ltsolve(y)
    wy = b.copy(); orc.csc_utsolve_f(n, Up, Ui, Ux, wy)
    wx = wy.copy(); orc.csc_ltsolve_f(n, Lp, Li, Lx, wx)
    assert rel_err(y, wy) <= RTOL and rel_err(x, wx) <= RTOL


@pytest.mark.parametrize("nb", [1, 20])
def test_class_boundaries(gpu, orc, nb):
    """Dense blocks around the sweep classes' limits (20 .. 180 pivots), k = 256 for the fused-permutation graphs."""
    for nd in (20, 33, 48, 64, 65, 100, 136, 137, 180):
        m, n, Ap, Ai, Ax = synth.dense_block_matrix(n=nd + nb + 40, nd=nd, seed=nd + nb)
        with gpu.Factorization(m, n, Ap, Ai) as F:
            F.factor(Ax, 1e-3)
            q = F.ordering()["q"]
            for k in (1, 8, 256):
                B = _rhs(n, k, nd + k)
                err = rel_err(F.solve(B, trans=True), _oracle_solve_t(orc, n, Ap, Ai, Ax, q, B))
                assert err <= RTOL, "nd=%d nb=%d k=%d: relative error %.3e" % (nd, nb, k, err)


def _batch_check(gpu, orc, m, n, Ap, Ai, AX, k, sample, seed):
    nbat = AX.shape[0]
    B = np.random.default_rng(seed).standard_normal((nbat, n, k))
    with gpu.Factorization(m, n, Ap, Ai, batch=nbat) as F:
        F.factor(AX, 1e-3)
        X = F.solve(B, trans=True)
        q = F.ordering()["q"]
    for i in sample:
        err = rel_err(X[i], _oracle_solve_t(orc, n, Ap, Ai, AX[i], q, B[i]))
        assert err <= RTOL, "matrix %d: relative error %.3e" % (i, err)


def test_batches(gpu, orc):
    """batch 4 (lane = row), batch 130 (interleaved, lane = matrix), and a many-RHS batch."""
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=21)
    rng = np.random.default_rng(1)
    AX4 = Ax[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(4, len(Ax))))
    _batch_check(gpu, orc, m, n, Ap, Ai, AX4, 2, range(4), 1)
    _batch_check(gpu, orc, m, n, Ap, Ai, AX4, 70, (0, 3), 2)
    AX130 = Ax[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(130, len(Ax))))
    _batch_check(gpu, orc, m, n, Ap, Ai, AX130, 1, (0, 63, 64, 129), 3)
    _batch_check(gpu, orc, m, n, Ap, Ai, AX130, 3, (5, 128), 4)


def test_full_size_config3(gpu, orc):
    """The 50 000-column matrix: 1 and 128 right-hand sides against the oracle's sweeps on the oracle's factors, the
    residual, and a second transposed solve bitwise equal to the first."""
    m, n, Ap, Ai, Ax = synth.grid_jacobian()
    A = csc_to_scipy(m, n, Ap, Ai, Ax)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        q = F.ordering()["q"]
        for k in (1, 128):
            B = _rhs(n, k, 50 + k)
            X = F.solve(B, trans=True)
            Bo = B if k == 1 else B[:, :4]
            Xo = X if k == 1 else X[:, :4]
            assert rel_err(Xo, _oracle_solve_t(orc, n, Ap, Ai, Ax, q, np.ascontiguousarray(Bo))) <= RTOL
            assert _residual_ok(A, X, B)
            assert np.array_equal(F.solve(B, trans=True), X)


def test_no_cross_talk_between_plain_and_transposed(gpu):
    """Interleaved plain and transposed solves on one handle (256 right-hand sides with rotating buffers included):
    every plain result equals a fresh handle's bit for bit, every _dev result equals the host form."""
    import torch
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=20000, seed=11)
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    with gpu.Factorization(m, n, Ap, Ai) as F0:
        F0.factor(Ax, 1e-3)
        ref = {k: F0.solve(_rhs(n, k, k)) for k in (1, 16, 256)}
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        host_t = {}
        for rnd in range(2):
            for k in (1, 16, 256):
                B = _rhs(n, k, k)
                assert np.array_equal(F.solve(B), ref[k])
                host_t[k] = F.solve(B, trans=True)
                bufs = [torch.from_numpy(B.copy()).to(dev) for _ in range(3 if k == 256 else 1)]
                for d in bufs:                                           # fresh addresses: the (nrhs, X) graph caches
                    F.solve_dev(d.data_ptr(), k, sh, trans=True)
                    torch.cuda.synchronize()
                    assert np.array_equal(d.cpu().numpy(), host_t[k])
                d = torch.from_numpy(B.copy()).to(dev)
                F.solve_dev(d.data_ptr(), k, sh)
                torch.cuda.synchronize()
                assert np.array_equal(d.cpu().numpy(), ref[k])


def test_cholesky_transposed_is_plain(gpu):
    n = 1500
    ei, ej = synth.spd_grid_pattern(n, seed=5)
    m, n, Ap, Ai, Ax = synth.spd_grid_matrix(n, ei, ej, seed=6)
    with gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY) as F:
        F.factor(Ax)
        for k in (1, 20):
            B = _rhs(n, k, k)
            assert np.array_equal(F.solve(B, trans=True), F.solve(B))
            assert np.array_equal(F.ltsolve(B), F.usolve(B))
        with pytest.raises(gpu.Cs3Error):
            F.utsolve(B)


@pytest.mark.parametrize("k", [1, 4])
def test_general_csc_transposed_triangular_solves_match_oracle(gpu, orc, k):
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    q = orc.csc_amd_f(1, n, n, Ap, Ai)
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, 1e-3)
    B = _rhs(n, k, 9)
    X = np.ascontiguousarray(B.copy())
    W = np.ascontiguousarray(B.copy())

    def oracle(fn, G):
        for t in range(k):
            col = np.ascontiguousarray(W[:, t]) if k > 1 else W
            fn(n, *G, col)
            if k > 1:
                W[:, t] = col

    gpu.csc_utsolve_f(n, Up, Ui, Ux, X); oracle(orc.csc_utsolve_f, (Up, Ui, Ux))
    assert rel_err(X, W) <= RTOL
    gpu.csc_ltsolve_f(n, Lp, Li, Lx, X); oracle(orc.csc_ltsolve_f, (Lp, Li, Lx))
    assert rel_err(X, W) <= RTOL


def test_transposed_matvec_residual_and_refinement(gpu, orc):
    import torch
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=7)
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(12)
    x = rng.standard_normal(n)
    _, _, Tp, Ti, Tx = orc.csc_transpose(m, n, Ap, Ai, Ax)
    want = orc.csc_mat_vec_ff(n, m, Tp, Ti, Tx, x)
    A = csc_to_scipy(m, n, Ap, Ai, Ax)
    b = rng.standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        d_ax = torch.from_numpy(np.asarray(Ax, dtype=np.float64).copy()).to(dev)
        d_x = torch.from_numpy(x.copy()).to(dev)
        d_y = torch.empty(n, dtype=torch.float64, device=dev)
        F.matvec_dev(d_ax.data_ptr(), d_x.data_ptr(), d_y.data_ptr(), 1, sh, trans=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_y.cpu().numpy(), np.asarray(want).reshape(-1))
        xs = F.solve(b, trans=True)
        r_direct = np.abs(A.T @ xs - b).max()
        d_b = torch.from_numpy(b.copy()).to(dev)
        d_r = torch.empty(n, dtype=torch.float64, device=dev)
        d_xs = torch.from_numpy(xs.copy()).to(dev)
        F.residual_dev(d_ax.data_ptr(), d_b.data_ptr(), d_xs.data_ptr(), d_r.data_ptr(), 1, sh, trans=True)
        torch.cuda.synchronize()
        assert np.allclose(d_r.cpu().numpy(), b - A.T @ xs, rtol=0.0, atol=1e-12 * np.abs(b).max())
        d_xp = torch.from_numpy(xs * (1.0 + 1e-4 * rng.standard_normal(n))).to(dev)
        F.refine_dev(d_ax.data_ptr(), d_b.data_ptr(), d_xp.data_ptr(), 1, 1, sh, trans=True)
        torch.cuda.synchronize()
        r_ref = np.abs(A.T @ d_xp.cpu().numpy() - b).max()
        assert r_ref <= 10.0 * max(r_direct, 1e-14 * np.abs(b).max())
