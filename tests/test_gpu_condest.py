"""Condition estimates (LAPACK dlacn2 per matrix of a batch) and log-determinants from the factors a handle holds, on the
GPU, against the NumPy port of dlacn2 (tests/lacn2_ref.py) driven by SuperLU solves, closed forms (Laplacian + shift I:
||A^-1||_1 = 1 / shift), dense references and the handle's own exported factors."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from csparse3_amd import synth
from helpers import csc_to_scipy
from lacn2_ref import lacn2
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

SHIFTS = (1e-2, 1e-3, 1e-4, 1e-5)


def _port(m, n, Ap, Ai, Ax):
    lu = spla.splu(csc_to_scipy(m, n, Ap, Ai, Ax).tocsc())
    return lacn2(n, lu.solve, lambda b: lu.solve(b, trans="T"))


def _rel(a, b):
    return abs(a - b) / abs(b)


def _condest_dev(F, AX):
    import torch
    dev = torch.device("cuda", 0)
    d_ax = torch.from_numpy(np.ascontiguousarray(AX, dtype=np.float64).reshape(-1).copy()).to(dev)
    d_c = torch.full((F.batch,), -1.0, dtype=torch.float64, device=dev)
    d_i = torch.full_like(d_c, -1.0)
    F.condest_dev(d_ax.data_ptr(), d_c.data_ptr(), d_i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_c.cpu().numpy(), d_i.cpu().numpy(), d_ax.cpu().numpy()


def _diag_from_factors(F, b=0):
    Lp, Li, Lx, Up, Ui, Ux = F.factors(b)
    return Lx[Lp[:-1]] if Ux is None else Ux[Up[1:] - 1]


def _spd_batch(n, nb, seed, shifts=SHIFTS):
    ei, ej = synth.spd_grid_pattern(n, seed=seed)
    mats = [synth.spd_grid_matrix(n, ei, ej, seed=seed + 1 + b, shift=shifts[b % len(shifts)]) for b in range(nb)]
    m, n, Ap, Ai, _ = mats[0]
    return m, n, Ap, Ai, np.stack([x[4] for x in mats])


def _perturbed(Ax, nb, seed):
    rng = np.random.default_rng(seed)
    return Ax[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(nb, len(Ax))))


# 1. parity with the port on every parity case
@pytest.mark.parametrize("name", list(CASES))
def test_condest_matches_the_port(gpu, name):
    m, n, Ap, Ai, Ax = CASES[name]
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        cond, inv = F.condest(Ax)
    want, _ = _port(m, n, Ap, Ai, Ax)
    assert _rel(inv[0], want) <= 1e-10, "%s: %.17g vs port %.17g" % (name, inv[0], want)
    assert cond[0] == gpu.csc_norm(n, Ap, Ax) * inv[0]
    if n <= 3000:
        exact = np.abs(np.linalg.inv(csc_to_scipy(m, n, Ap, Ai, Ax).toarray())).sum(axis=0).max()
        assert inv[0] <= exact * (1.0 + 1e-10)


# 2. exact on M-matrices: Laplacian + shift I has ||A^-1||_1 = 1 / shift
@pytest.mark.parametrize("chol", [False, True])
def test_m_matrices_give_one_over_shift(gpu, chol):
    n = 1500
    ei, ej = synth.spd_grid_pattern(n, seed=3)
    for shift, tol in [(s, 1e-10) for s in SHIFTS] + [(1e-8, 1e-6)]:
        m, n, Ap, Ai, Ax = synth.spd_grid_matrix(n, ei, ej, seed=4, shift=shift)
        with gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY if chol else gpu.CS3_LU) as F:
            F.factor(Ax)
            cond, inv = F.condest(Ax)
        assert _rel(inv[0], 1.0 / shift) <= tol, "shift %g: %.17g" % (shift, inv[0] * shift)


# 3. batches: the interleaved Cholesky batch of config 5, lane = row and lane = matrix LU batches
def test_cholesky_batch_of_512(gpu):
    m, n, Ap, Ai, AX = _spd_batch(5000, 512, seed=5000)
    with gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY, batch=512) as F:
        F.factor(AX)
        cond, inv = F.condest(AX)
    shift = np.array([SHIFTS[b % 4] for b in range(512)])
    assert np.abs(inv * shift - 1.0).max() <= 1e-9


@pytest.mark.parametrize("nb", [4, 130])
def test_lu_batches(gpu, nb):
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=21)
    AX = _perturbed(Ax, nb, nb)
    with gpu.Factorization(m, n, Ap, Ai, batch=nb) as F:
        F.factor(AX, 1e-3)
        cond, inv = F.condest(AX)
    for b in sorted({0, 63, 64, 129} & set(range(nb)) | {nb - 1}):
        want, _ = _port(m, n, Ap, Ai, AX[b])
        assert _rel(inv[b], want) <= 1e-10, "matrix %d" % b
        assert cond[b] == gpu.csc_norm(n, Ap, AX[b]) * inv[b]


# 4. the host form (adaptive slots) and the _dev form (11 fixed slots) give the same bits, call after call
def _mixed_batch():
    """Three M-matrices (4 solves each) and three unsymmetric mixed-sign matrices on the same pattern (5 solves)."""
    n = 1500
    ei, ej = synth.spd_grid_pattern(n, seed=3)
    m, n, Ap, Ai, Ax = synth.spd_grid_matrix(n, ei, ej, seed=4, shift=1e-2)
    off = Ai != np.repeat(np.arange(n), np.diff(Ap))
    mats = []
    for s in range(3):
        mats.append(synth.spd_grid_matrix(n, ei, ej, seed=10 + s, shift=SHIFTS[s])[4])
        g = np.random.default_rng(100 + s)
        v = Ax.copy()
        v[off] *= g.choice([-1.0, 1.0], off.sum()) * g.uniform(0.3, 1.0, off.sum())
        mats.append(v)
    return m, n, Ap, Ai, np.stack(mats)


def test_both_forms_give_the_same_bits(gpu):
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        c1, i1 = F.condest(Ax)
        c2, i2, _ = _condest_dev(F, Ax)
        c3, i3 = F.condest(Ax)
    assert np.array_equal(c1, c2) and np.array_equal(i1, i2) and np.array_equal(c1, c3) and np.array_equal(i1, i3)
    m, n, Ap, Ai, AX = _mixed_batch()
    counts = [_port(m, n, Ap, Ai, AX[b])[1] for b in range(len(AX))]
    assert min(counts) == 4 and max(counts) >= 5, counts
    for kind in (gpu.CS3_LU, gpu.CS3_CHOLESKY):
        if kind == gpu.CS3_CHOLESKY:
            AX = AX[0::2]                                        # the SPD members only
        with gpu.Factorization(m, n, Ap, Ai, kind=kind, batch=len(AX)) as F:
            F.factor(AX)
            c1, i1 = F.condest(AX)
            c2, i2, _ = _condest_dev(F, AX)
            c3, i3, _ = _condest_dev(F, AX)
        assert np.array_equal(c1, c2) and np.array_equal(i1, i2) and np.array_equal(c2, c3) and np.array_equal(i2, i3)
        for b in range(len(AX)):
            assert _rel(i1[b], _port(m, n, Ap, Ai, AX[b])[0]) <= 1e-10


# 5. the handle and the caller's values are left as they were
def test_condest_leaves_the_handle_as_it_was(gpu):
    import torch
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    b = np.random.default_rng(3).standard_normal(n)
    d_ax = torch.from_numpy(np.asarray(Ax, dtype=np.float64).copy()).to(dev)

    def fused(F):
        d_x = torch.from_numpy(b.copy()).to(dev)
        F.factor_solve_dev(d_ax.data_ptr(), d_x.data_ptr(), 1, 1e-3, sh)
        F.factor_status(sh)
        return d_x.cpu().numpy()

    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        x0, t0, f0 = F.solve(b), F.solve(b, trans=True), fused(F)
        Axc = np.array(Ax, copy=True)
        F.condest(Ax)
        _, _, ax_after = _condest_dev(F, Ax)
        F.slogdet()
        assert np.array_equal(np.asarray(Ax), Axc) and np.array_equal(ax_after, Axc)
        assert np.array_equal(F.solve(b), x0) and np.array_equal(F.solve(b, trans=True), t0)
        assert np.array_equal(fused(F), f0)
        assert np.array_equal(d_ax.cpu().numpy(), Axc)


def _perm_sign(p):
    p = np.asarray(p)
    seen = np.zeros(len(p), dtype=bool)
    sign = 1
    for i in range(len(p)):
        if not seen[i]:
            j, length = i, 0
            while not seen[j]:
                seen[j] = True
                j = p[j]
                length += 1
            sign *= -1 if length % 2 == 0 else 1
    return sign


# 6. config 3 at full size
def test_config3_full_size(gpu):
    m, n, Ap, Ai, Ax = synth.grid_jacobian()
    A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()
    lu = spla.splu(A)
    want, _ = lacn2(n, lu.solve, lambda v: lu.solve(v, trans="T"))
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        cond, inv = F.condest(Ax)
        c2, i2, _ = _condest_dev(F, Ax)
        sign, logabs = F.slogdet()
    assert _rel(inv[0], want) <= 1e-10 and np.array_equal(inv, i2) and np.array_equal(cond, c2)
    du = lu.U.diagonal()
    log_want = np.log(np.abs(du)).sum()
    assert np.isfinite(logabs[0]) and _rel(logabs[0], log_want) <= 1e-10
    sign_want = (-1.0 if (du < 0).sum() % 2 else 1.0) * _perm_sign(lu.perm_r) * _perm_sign(lu.perm_c)
    assert sign[0] == sign_want


# 7. log-determinants
@pytest.mark.parametrize("name", list(CASES))
def test_slogdet_on_cases(gpu, name):
    m, n, Ap, Ai, Ax = CASES[name]
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        sign, logabs = F.slogdet()
        d = _diag_from_factors(F)
        Ax2 = np.array(Ax, copy=True)
        Ax2[np.asarray(Ai) == n // 2] *= -1.0                   # one row negated
        F.factor(Ax2, 1e-3)
        sign2, logabs2 = F.slogdet()
    want = np.log(np.abs(d)).sum()
    assert abs(logabs[0] - want) <= 1e-13 * max(1.0, abs(want))
    assert sign[0] == (-1.0 if (d < 0).sum() % 2 else 1.0)
    assert sign2[0] == -sign[0] and abs(logabs2[0] - logabs[0]) <= 1e-13 * max(1.0, abs(want))
    if n <= 3000:
        s, l = np.linalg.slogdet(csc_to_scipy(m, n, Ap, Ai, Ax).toarray())
        assert sign[0] == s and abs(logabs[0] - l) <= 1e-9 * max(1.0, abs(l))


def test_slogdet_cholesky_and_batches(gpu):
    m, n, Ap, Ai, AX = _spd_batch(5000, 512, seed=5000)
    with gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY, batch=512) as F:
        F.factor(AX)
        sign, logabs = F.slogdet()
        for b in (0, 63, 64, 511):
            want = 2.0 * np.log(_diag_from_factors(F, b)).sum()
            assert sign[b] == 1.0 and abs(logabs[b] - want) <= 1e-13 * max(1.0, abs(want)), b
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=21)
    AX = _perturbed(Ax, 130, 130)
    with gpu.Factorization(m, n, Ap, Ai, batch=130) as F:
        F.factor(AX, 1e-3)
        sign, logabs = F.slogdet()
        for b in (0, 63, 64, 129):
            d = _diag_from_factors(F, b)
            want = np.log(np.abs(d)).sum()
            assert sign[b] == (-1.0 if (d < 0).sum() % 2 else 1.0)
            assert abs(logabs[b] - want) <= 1e-13 * max(1.0, abs(want)), b


def test_slogdet_of_imported_factors_with_a_zero_or_nan_pivot(gpu):
    """Imported factors can hold any pivot: zero gives (0, -inf), NaN gives a NaN log|det| (numpy.linalg.slogdet)."""
    import torch
    m, n, Ap, Ai, Ax = CASES["jacobian118"]
    dev = torch.device("cuda", 0)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        sign0, _ = F.slogdet()
        u00 = _diag_from_factors(F)[0]
        buf = torch.empty(F.info.factor_bytes // 8, dtype=torch.float64, device=dev)
        F.export_factor_dev(buf.data_ptr())
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
    where = np.flatnonzero(host == u00)
    assert len(where) == 1
    rest = sign0[0] * np.sign(u00)                              # the sign of the other pivots' product
    for bad, want_sign, check in ((0.0, 0.0, lambda l: l == -np.inf), (np.nan, rest, np.isnan)):
        v = host.copy()
        v[where[0]] = bad
        d = torch.from_numpy(v).to(dev)
        with gpu.Factorization(m, n, Ap, Ai) as G:
            G.import_factor_dev(d.data_ptr())
            torch.cuda.synchronize()
            sign, logabs = G.slogdet()
        assert check(logabs[0]) and sign[0] == want_sign, (bad, sign, logabs)


# 8. the CscMat convenience and a 1 x 1 handle
def test_cscmat_and_one_by_one(gpu):
    from csparse3_amd.csc import CscMat
    m, n, Ap, Ai, Ax = CASES["jacobian118"]
    A = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax)
        cond, inv = F.condest(Ax)
        sign, logabs = F.slogdet()
    assert A.condest() == cond[0]
    assert A.slogdet() == (sign[0], logabs[0])
    one_p, one_i = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)
    for a in (4.0, -0.25):
        with gpu.Factorization(1, 1, one_p, one_i) as F:
            F.factor(np.array([a]))
            cond, inv = F.condest(np.array([a]))
            c2, i2, _ = _condest_dev(F, np.array([a]))
            sign, logabs = F.slogdet()
        assert inv[0] == 1.0 / abs(a) and cond[0] == 1.0 and i2[0] == inv[0] and c2[0] == cond[0]
        assert sign[0] == np.sign(a) and abs(logabs[0] - np.log(abs(a))) <= 1e-15
