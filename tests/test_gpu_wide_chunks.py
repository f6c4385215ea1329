"""Big fronts swept four 64-blocks (256 columns) per launch: k_fwd_big_step4 / k_bwd_big_step4, and the backward sweep of
a parentless root without k_bwd_big_init.  The matrices and the rule that sends a (batch, right-hand sides) pair down
that path are in tests/wide_chunk_cases.py (shapes asserted from the host analysis by tests/test_wide_chunk_cases_cpu.py).

LU, Cholesky and the transposed LU sweeps; (batch, nrhs) in wc.PAIRS_NEW on the 256 path and wc.PAIRS_OLD on the
unchanged one.  Per pair and mode (every half sweep alone -- a front with a parent still needs its init launch -- and
the full solves):
  every column of every matrix against sweep_cases.substitute (np.longdouble) on the handle's own factors;
  the residual of every matrix;
  a second call, and a call after every CU's LDS was filled with NaN patterns, give the same bits.
The fused step equals factor-then-solve bit for bit.

Bounds: those of tests/test_gpu_big_fronts_below_root.py (see its docstring).  Per column max|x - ref| / max|ref| <= RTOL;
|b - T x| <= 2 n u |T||x| componentwise per half sweep (Higham's bound for substitution in any order, which covers the
four-block order of summation too); the norm-wise residual 1e-12 (norm(T) max|x| + max|b|) per column."""
import collections
import ctypes as C

import numpy as np
import pytest

import sweep_cases as sc
import wide_chunk_cases as wc
from helpers import RTOL, U_ROUND
from rhs_cases import right_hand_sides
from test_gpu_big_fronts_below_root import MODES, _factors, _reference, _run

pytestmark = pytest.mark.gpu

LU_TOL = 1e-3
KINDS = ("lu", "chol")
Held = collections.namedtuple("Held", "F AX mat q factors")


@pytest.fixture(scope="module")
def handles(gpu):
    """One factorised handle per (case, kind, batch), shared by every test of this module."""
    held = {}

    def get(name, kind, batch):
        key = (name, kind, batch)
        if key not in held:
            sym = kind == "chol"
            mat = wc.case_matrix(name, symmetric=sym)
            m, n, Ap, Ai, _ = mat
            F = gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY if sym else gpu.CS3_LU, batch=batch)
            AX = wc.case_values(name, batch, symmetric=sym)
            F.factor(AX, 0.0 if sym else LU_TOL)
            held[key] = Held(F, AX, mat, F.ordering()["q"], {})
        return held[key]

    yield get
    for h in held.values():
        h.F.close()


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


PAIRS = wc.PAIRS_NEW + wc.PAIRS_OLD


@pytest.mark.parametrize("pair", PAIRS, ids=["b%d-k%d" % p for p in PAIRS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(wc.CASES))
def test_sweeps_in_256_column_chunks(gpu, handles, name, kind, pair):
    batch, nrhs = pair
    h = handles(name, kind, batch)
    F = h.F
    m, n, Ap, Ai, _ = h.mat
    K = sc.solve_kinds(gpu, F)
    wide = sc.wide_fronts(K)
    assert tuple((int(K.r[s]), int(K.w[s])) for s in wide) == wc.FRONTS[name] and {K.kind[s] for s in wide} == {"big"}
    assert wc.chunk_width(batch, nrhs, int(K.w[wide[-1]])) == (256 if pair in wc.PAIRS_NEW else 64)
    B = right_hand_sides(batch, n, nrhs, seed=500 * batch + nrhs)
    for mode, (sweeps, permute) in MODES[kind].items():
        what = "%s %s batch %d nrhs %d %s" % (name, kind, batch, nrhs, mode)
        X = _run(F, mode, B)
        assert X.shape == B.shape
        for b in range(batch):
            L, U = _factors(h, b)
            Xb, Bb = X[b], B[b]
            ref = _reference(h, b, mode, kind, Bb)
            scale = np.abs(ref).max(axis=0)
            err = np.abs(Xb - ref).max(axis=0)
            for j in range(nrhs):
                if scale[j] == 0:
                    assert not Xb[:, j].any(), "%s matrix %d column %d: a zero column came back nonzero" % (what, b, j)
                else:
                    assert err[j] <= RTOL * scale[j], "%s matrix %d column %d: relative error %.3e" % (what, b, j, float(err[j] / scale[j]))
            if permute:                                  # the system itself (solve_t: its transpose)
                T64 = sc.dense64(n, Ap, Ai, h.AX[b], trans=mode == "solve_t")
            else:
                which, lower, trans = sweeps[0]
                T64 = sc.dense64(n, *(L if which == "L" else U), trans=trans)
            # the project's norm-wise residual, per column; what the float64 product T x itself can be off by is taken off
            res = np.abs(T64 @ Xb - Bb).max(axis=0) + n * U_ROUND * (np.abs(T64) @ np.abs(Xb)).max(axis=0)
            lim = 1e-12 * (np.abs(T64).sum(axis=0).max() * np.abs(Xb).max(axis=0) + np.abs(Bb).max(axis=0))
            assert (res <= lim).all(), "%s matrix %d: residual / limit %.3g" % (what, b, float((res / np.where(lim > 0, lim, 1)).max()))
            if not permute:
                ratio = sc.substitution_error_ratio(T64.astype(np.longdouble), Xb, Bb)
                assert (ratio <= 2 * n).all(), "%s matrix %d: max |b - T x| / (u |T||x|) = %.2f > %d" % (what, b, ratio.max(), 2 * n)
        assert np.array_equal(_run(F, mode, B), X), what + ": two calls differ"
        _poison(gpu)
        assert np.array_equal(_run(F, mode, B), X), what + ": stale LDS reaches the result"


@pytest.mark.parametrize("pair", PAIRS, ids=["b%d-k%d" % p for p in PAIRS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(wc.CASES))
def test_fused_step_equals_factor_then_solve(gpu, handles, name, kind, pair):
    """factor_solve_bx_dev == factor_dev + solve_dev bit for bit, three times (the third call replays the graph); the
    root's pipelined forward sweep releases its chunks by the plan's chunk width."""
    import torch
    batch, nrhs = pair
    h = handles(name, kind, batch)
    F = h.F
    n = F.n
    tol = 0.0 if kind == "chol" else LU_TOL
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    B = right_hand_sides(batch, n, nrhs, seed=77 + nrhs)
    d_ax = torch.from_numpy(h.AX.copy()).to(dev)
    d_b = torch.from_numpy(B).to(dev)
    x_split = d_b.clone()
    F.factor_dev(d_ax.data_ptr(), tol, sh)
    F.solve_dev(x_split.data_ptr(), nrhs, sh)
    F.factor_status(sh)
    x_fused = torch.zeros_like(d_b)
    for _ in range(3):
        x_fused.zero_()
        _poison(gpu)
        F.factor_solve_bx_dev(d_ax.data_ptr(), d_b.data_ptr(), x_fused.data_ptr(), nrhs, tol, sh)
        F.factor_status(sh)
        assert torch.equal(x_fused, x_split)
    assert torch.equal(d_b, torch.from_numpy(B).to(dev))
    X = x_split.cpu().numpy()
    for b in sorted({0, batch - 1}):
        ref = _reference(h, b, "solve", kind, B[b])
        scale = np.abs(ref).max(axis=0)
        assert (np.abs(X[b] - ref).max(axis=0) <= RTOL * scale).all()
