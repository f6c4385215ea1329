"""GMRES refinement on held factors on the GPU (cs3_gmres / cs3_gmres_dev, csrc/krylov.hip): F is factorised from A0 and
the values of A go to gmres, on the engineered cases of tests/gmres_cases.py; tests/test_gmres_cpu.py says what the NumPy
reference does on them.

Agreement of the recurrence's residual with the true one at a cycle's end: the reference's own figure is
max |estimate - true| / ||b|| = 2.0e-16 (test_gmres_cpu.py); the GPU gets 10 x that, and its figure is printed by tests
1 and 2: 3.8e-16 at r = 5, 2e-17 .. 9e-17 on the other cases."""
import numpy as np
import pytest

import gmres_cases as gc
import perturb_cases as pp
from helpers import rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-12
CHUNK = 1024


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dense(case, b=None, trans=False):
    A = case.A.toarray()
    return np.linalg.solve(A.T if trans else A, case.b if b is None else b)


@pytest.fixture(scope="module")
def held(gpu):
    """Handles factorised from A0, one per (n, seed, batch) of grid_jacobian, shared by the tests of this module."""
    made = {}

    def get(case, batch=1):
        key = (case.mat[1], case.mat[2].tobytes(), batch)
        if key not in made:
            m, n, Ap, Ai, Ax0 = case.mat
            F = gpu.Factorization(m, n, Ap, Ai, batch=batch)
            F.factor(np.tile(Ax0, (batch, 1)) if batch > 1 else Ax0)
            made[key] = F
        return made[key]

    yield get
    for F in made.values():
        F.close()


def _gap_after_every_cycle(F, case, rtol, restart, ncycles):
    """max |estimate - true| / ||b|| over the cycles: the call stopped after c cycles gives the true residual in relres and
    the recurrence's last estimate through the diagnostic."""
    gap = 0.0
    for c in range(1, ncycles + 1):
        _, iters, relres = F.gmres(case.Ax, case.b, rtol=rtol, restart=restart, max_iters=c * restart)
        est = F.debug_gmres_estimates(1)
        gap = max(gap, abs(float(est[0]) - float(relres[0])))
    return gap


# 1. finite termination: exactly r iterations, where the stationary rounds grow
@pytest.mark.parametrize("r", [1, 3, 5])
def test_finite_termination(gpu, held, r):
    case = gc.diag_case(300, 7, r)
    F = held(case)
    x, iters, relres = F.gmres(case.Ax, case.b, rtol=RTOL)
    print("r=%d iters %s relres %s" % (r, iters, relres))
    assert list(iters) == [r] and relres[0] <= 1e-12
    assert rel_err(x, _dense(case)) <= 1e-10
    xs, corr = F.solve(case.b), []
    for _ in range(3):
        xs, c = F.refine(case.Ax, case.b, xs, 1)
        corr.append(c)
    print("stationary corrections %s" % ["%.2e" % c for c in corr])
    assert corr[0] < corr[1] < corr[2]
    gap, bound = _gap_after_every_cycle(F, case, RTOL, 30, 1), 10.0 * gc.reference_gap()
    print("r=%d: |estimate - true| / ||b|| = %.3e (bound %.3e)" % (r, gap, bound))
    assert gap <= bound


# 2. restarts: the reference's iteration count
@pytest.mark.parametrize("r,restart", gc.RESTART_CASES)
def test_restart_cases(gpu, held, r, restart):
    rc = gc.restart_case(r, restart)
    F = held(rc.case)
    x, iters, relres = F.gmres(rc.case.Ax, rc.case.b, rtol=rc.rtol, restart=restart)
    print("r=%d restart=%d rtol %.3e: iters %s (reference %d) relres %s" % (r, restart, rc.rtol, iters, rc.iters, relres))
    assert list(iters) == [rc.iters] and relres[0] <= rc.rtol
    ncycles = -(-rc.iters // restart)
    gap, bound = _gap_after_every_cycle(F, rc.case, rc.rtol, restart, ncycles), 10.0 * gc.reference_gap()
    print("|estimate - true| / ||b|| over %d cycles = %.3e (bound %.3e)" % (ncycles, gap, bound))
    assert gap <= bound


# 3. fresh factors: nothing to do from solve(b), the lucky breakdown from zero
def test_fresh_factors(gpu, held):
    case = gc.diag_case(300, 7, 1)
    F = held(case)
    Ax0 = case.mat[4]
    x0 = F.solve(case.b)
    x, iters, relres = F.gmres(Ax0, case.b, x0=x0, rtol=RTOL)
    assert list(iters) == [0] and _same_bits(x, x0) and relres[0] <= RTOL
    x, iters, relres = F.gmres(Ax0, case.b, x0=np.zeros(300), rtol=RTOL)
    print("from zero: iters %s relres %s" % (iters, relres))
    assert list(iters) == [1] and np.isfinite(x).all() and relres[0] <= RTOL
    assert rel_err(x, x0) <= 1e-10


# 4. a batch whose systems need 0, 1 and 5 iterations in one call: the frozen-column path
def test_mixed_batch(gpu, held):
    mb = gc.mixed_batch()
    F3, F1 = held(mb.cases[0], batch=3), held(mb.cases[0])
    x, iters, relres = F3.gmres(mb.AX, mb.B, rtol=RTOL)
    want_iters = [gc.reference(mb.cases[b], b=mb.B[b, :, t], rtol=RTOL).iters for b in range(3) for t in range(2)]
    print("iters %s reference %s relres %s" % (iters, want_iters, relres))
    assert want_iters == [0, 0, 1, 1, 5, 5] and list(iters) == want_iters
    assert (relres <= RTOL).all()
    for b in range(3):
        for t in range(2):
            alone, it1, _ = F1.gmres(mb.AX[b], mb.B[b, :, t], rtol=RTOL)
            assert list(it1) == [want_iters[2 * b + t]]
            assert rel_err(x[b, :, t], alone) <= 1e-10, (b, t)
            assert rel_err(x[b, :, t], _dense(mb.cases[b], mb.B[b, :, t])) <= 1e-10, (b, t)
    x2, iters2, relres2 = F3.gmres(mb.AX, mb.B, rtol=RTOL)
    assert _same_bits(x, x2) and np.array_equal(iters, iters2) and _same_bits(relres, relres2)


# 5. row edges of the chunked reductions, with k = 3 (idle tx lanes)
@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_row_edges(gpu, n):
    assert gpu.gmres_limits().chunk_rows == CHUNK
    r = min(2, n)
    case = gc.diag_case(n, 11, r, mat=gc.tridiagonal(1, 3) if n == 1 else None)
    m, _, Ap, Ai, Ax0 = case.mat
    B = np.random.default_rng(n).standard_normal((n, 3))
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax0)
        x, iters, relres = F.gmres(case.Ax, B, rtol=RTOL)
    want = [gc.reference(case, b=B[:, t], rtol=RTOL).iters for t in range(3)]
    print("n=%d iters %s reference %s relres %s" % (n, iters, want, relres))
    assert list(iters) == want and max(want) <= r and (relres <= RTOL).all()
    assert rel_err(x, _dense(case, B)) <= 1e-10


# 6. right-hand-side tile edges: every column its own b
@pytest.mark.parametrize("k", [63, 64, 65])
def test_rhs_tile_edges(gpu, held, k):
    assert gpu.gmres_limits().rhs_tile == 64
    case = gc.diag_case(40, 5, 2)
    F = held(case)
    B = np.random.default_rng(k).standard_normal((40, k))
    x, iters, relres = F.gmres(case.Ax, B, rtol=RTOL)
    want = _dense(case, B)
    assert iters.shape == (k,) and (iters <= 2).all() and (relres <= RTOL).all(), (iters, relres)
    for t in range(k):
        assert rel_err(x[:, t], want[:, t]) <= 1e-10, t


# 7. max_iters below need: not an error, and the residual of the iterations that ran
def test_max_iters_below_need(gpu, held):
    case = gc.diag_case(300, 7, 5)
    F = held(case)
    full = gc.reference(case, rtol=RTOL)
    x0 = F.solve(case.b)
    r0 = np.linalg.norm(case.b - case.A @ x0) / np.linalg.norm(case.b)
    x, iters, relres = F.gmres(case.Ax, case.b, x0=x0, rtol=RTOL, max_iters=2)
    # (the history counts from the initial residual: its third value is the residual after two iterations)
    print("relres %.6e, reference after two iterations %.6e, initial %.3e" % (relres[0], full.history[1], r0))
    assert list(iters) == [2]
    assert abs(relres[0] - full.history[1]) <= 1e-6 * full.history[1]
    assert relres[0] <= r0
    true = np.linalg.norm(case.b - case.A @ x) / np.linalg.norm(case.b)
    assert abs(true - relres[0]) <= 1e-6 * relres[0]


# 8. the transposed system
def test_transposed(gpu, held):
    case = gc.diag_case(300, 7, 3)
    F = held(case)
    x, iters, relres = F.gmres(case.Ax, case.b, rtol=RTOL, trans=True)
    want = gc.reference(case, rtol=RTOL, trans=True)
    print("trans: iters %s (reference %d) relres %s" % (iters, want.iters, relres))
    assert list(iters) == [want.iters] == [3] and relres[0] <= RTOL
    assert rel_err(x, _dense(case, trans=True)) <= 1e-10


# 9. a matched handle: products and solves are with A
def test_matched_handle(gpu, orc):
    c = pp.matched_case(gpu, orc)["c"]
    n = c.n
    Ap, Ai, Ax0 = np.asarray(c.Ap), np.asarray(c.Ai), np.asarray(c.Ax, dtype=np.float64)
    stored = [j for j in range(n) for p in range(Ap[j], Ap[j + 1]) if Ai[p] == j and Ax0[p] != 0.0]
    rng = np.random.default_rng(9)
    rows = np.sort(rng.choice(stored, size=3, replace=False))
    mat = (n, n, Ap, Ai, Ax0)
    Ax = gc.scale_diagonal(mat, rows, 4.0)
    b = rng.standard_normal(n)
    with gpu.Factorization(n, n, Ap, Ai, match_values=Ax0) as F:
        F.factor(Ax0)
        x, iters, relres = F.gmres(Ax, b, rtol=RTOL)
    want = np.linalg.solve(gc.to_scipy(mat, Ax).toarray(), b)
    print("matched %s: iters %s relres %s err %.2e" % (c.name, iters, relres, rel_err(x, want)))
    assert iters[0] <= 3 + 1 and relres[0] <= RTOL
    assert rel_err(x, want) <= 1e-10


# 10. the perturbation through the public path
def test_perturbation_through_the_public_path(gpu, orc):
    import scipy.sparse.linalg as spla

    import gmres_ref
    from csparse3_amd import csc
    (m, n, Ap, Ai, Ax), b, x_ref, _ = pp.end_to_end(gpu, orc)
    A = csc.CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    x = csc.lusol(A, b, perturb=True, refine="gmres")
    assert rel_err(x, x_ref) <= 1e-10, rel_err(x, x_ref)
    # a delta so large that the reference's stationary loop on A + E_ref grows: 0.1 max |A| replaces 5 pivots
    delta = 0.1 * float(np.abs(Ax).max())
    with gpu.Factorization(m, n, Ap, Ai) as F:
        q = F.ordering()["q"]
    ref = pp.reference(orc, (m, n, Ap, Ai, Ax), q, delta)
    lu = spla.splu(gc.to_scipy((m, n, Ap, Ai, Ax), ref.Ax).tocsc())
    As = gc.to_scipy((m, n, Ap, Ai, Ax)).tocsr()
    _, corr = pp.refine_loop(lu.solve, As, b)
    g = gmres_ref.gmres(As, lu.solve, b, lu.solve(b), 1e-12, 30, 100)
    print("delta %.3e: %d perturbed, reference corrections %s, reference gmres %d iterations"
          % (delta, len(ref.perturbed), ["%.1e" % c for c in corr], g.iters))
    assert len(corr) >= 2 and corr[-1] > corr[-2], "the reference's stationary loop must grow"
    x_stat = csc.lusol(A, b, perturb=delta)
    assert not rel_err(x_stat, x_ref) <= 1e-10, "the stationary rounds cannot refine this"
    x_gm = csc.lusol(A, b, perturb=delta, refine="gmres", max_refine=g.iters + 1)
    print("stationary error %.2e, gmres error %.2e" % (rel_err(x_stat, x_ref), rel_err(x_gm, x_ref)))
    assert rel_err(x_gm, x_ref) <= 1e-10
    assert _same_bits(A.solve(b, perturb=delta, refine="gmres", max_refine=g.iters + 1), x_gm)


# 11. zero and NaN right-hand sides stay with their own system
def test_zero_and_nan_right_hand_sides(gpu, held):
    case = gc.diag_case(300, 7, 3)
    F = held(case)
    B = np.stack([np.zeros(300), case.b], axis=1)
    x, iters, relres = F.gmres(case.Ax, B, x0=np.ones((300, 2)), rtol=RTOL)
    assert not x[:, 0].any() and iters[0] == 0 and relres[0] == 0.0
    assert iters[1] >= 3 and relres[1] <= RTOL and rel_err(x[:, 1], _dense(case)) <= 1e-10
    B = np.stack([case.b, case.b], axis=1)
    B[17, 0] = np.nan
    x0 = np.zeros((300, 2))
    x, iters, relres = F.gmres(case.Ax, B, x0=x0, rtol=RTOL)
    print("NaN in system 0: iters %s relres %s" % (iters, relres))
    assert np.isnan(relres[0]) and iters[0] == 0 and not x[:, 0].any()
    assert relres[1] <= RTOL and rel_err(x[:, 1], _dense(case)) <= 1e-10


# 12. the host and the device form give the same bits; the work memory goes with the handle
def test_host_and_device_forms(gpu):
    import torch
    case = gc.diag_case(300, 7, 5)
    m, n, Ap, Ai, Ax0 = case.mat
    before = gpu.debug_live_device_buffers()
    F = gpu.Factorization(m, n, Ap, Ai)
    F.factor(Ax0)
    B = np.stack([case.b, 2.0 * case.b[::-1]], axis=1)
    x0 = F.solve(B)
    x, iters, relres = F.gmres(case.Ax, B, x0=x0, rtol=RTOL, restart=3)
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    ax_d, b_d, x_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (case.Ax, B, x0))
    iters_d, relres_d = F.gmres_dev(ax_d.data_ptr(), b_d.data_ptr(), x_d.data_ptr(), k=2, rtol=RTOL, restart=3, stream=sh)
    torch.cuda.synchronize()
    assert _same_bits(x_d.cpu().numpy(), x) and np.array_equal(iters, iters_d) and _same_bits(relres, relres_d)
    assert (relres <= RTOL).all() and iters.min() > 3
    assert gpu.debug_live_device_buffers() > before
    F.close()
    assert gpu.debug_live_device_buffers() == before
