"""Low-rank-modified solves (cs3_updates_*) on the GPU: every case of every list against a factorisation of its own
modified matrix (splu(A + dA_c).solve(b), within helpers.RTOL), rpiv against the NumPy reference of the formula
(tests/updates_ref.py), constructed-singular cases against "must be flagged"."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import RTOL, csc_to_scipy, rel_err
from test_gpu_parity import CASES, SPD
import updates_ref as ur

pytestmark = pytest.mark.gpu

SING_TOL = 1e-10
COUNTS = {"toy10": None, "grid2k": 300, "grid20k": 300}           # None: every off-diagonal pair; the others 120


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


def _scipy(case):
    m, n, Ap, Ai, Ax = case
    return csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()


def _directs(A, cases, b):
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda c: ur.direct_solve(A, c, b), cases))


def _solve(gpu, F, cases, b, sing_tol=SING_TOL, poison=False):
    pattern, cx = ur.flatten(cases)
    with F.updates_plan(pattern) as plan:
        if poison:
            _poison(gpu)
        X, rpiv = F.solve_updates(plan, cx, b, sing_tol)
        return X, rpiv, plan.info


def _assert_parity(A, b, cases, X, rpiv, what, singular=()):
    """Every case: healthy ones within RTOL of the direct solve and of the reference's rpiv, the others flagged."""
    healthy = [c for c in range(len(cases)) if c not in singular]
    want = dict(zip(healthy, _directs(A, [cases[c] for c in healthy], b)))
    _, rpiv_ref, _ = ur.solve_updates_ref(A, b, cases, SING_TOL)
    worst = 0.0
    for c in range(len(cases)):
        if c in singular:
            assert np.isnan(X[:, c]).all(), "%s: singular case %d is not flagged" % (what, c)
            assert rpiv[c] <= 1e-13, "%s: singular case %d has rpiv %.3e" % (what, c, rpiv[c])
            continue
        err = rel_err(X[:, c], want[c])
        worst = max(worst, err)
        assert err <= RTOL, "%s case %d: relative error %.3e" % (what, c, err)
        assert abs(rpiv[c] - rpiv_ref[c]) <= RTOL, "%s case %d: rpiv %.17g vs %.17g" % (what, c, rpiv[c], rpiv_ref[c])
    print("%s: %d cases, worst relative error %.2e, smallest healthy rpiv %.2e" % (what, len(cases), worst,
                                                                                  rpiv[healthy].min()))


# 1. parity on every parity case (poisoned LDS)
@pytest.mark.parametrize("name", list(CASES))
def test_branch_outages_match_direct_solves(gpu, name):
    m, n, Ap, Ai, Ax = CASES[name]
    A = _scipy(CASES[name])
    cases = ur.branch_outages(A, COUNTS.get(name, 120), seed=41)
    assert len(cases) >= (12 if name == "toy10" else COUNTS.get(name, 120))
    b = np.random.default_rng(43).standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        X, rpiv, _ = _solve(gpu, F, cases, b, poison=True)
    _assert_parity(A, b, cases, X, rpiv, name)


# 2. ranks and shapes
def _block_case(rng, n, r, s, extra, scale=0.05):
    """r distinct rows x s distinct columns, every one of them touched, + `extra` more entries of the block."""
    R = rng.choice(n, size=r, replace=False)
    Cc = rng.choice(n, size=s, replace=False)
    k = max(r, s)
    i = np.r_[np.arange(k) % r, rng.integers(0, r, size=extra)]
    j = np.r_[np.arange(k) % s, rng.integers(0, s, size=extra)]
    return R[i], Cc[j], scale * rng.standard_normal(len(i))


def _shape_list(n):
    rng = np.random.default_rng(47)
    cases = [_block_case(rng, n, r, r, extra=r) for r in (1, 2, 3, 8, 15, 16)]
    cases.append(_block_case(rng, n, 1, 9, extra=0))                       # one row x 9 columns
    cases.append(_block_case(rng, n, 9, 1, extra=0))                       # 9 rows x one column
    cases.append((np.array([5, 5, 5, 9]), np.array([7, 7, 7, 5]), np.array([0.125, 0.25, -0.0625, 0.1])))    # duplicates add
    cases.append((np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0)))                             # empty
    cases.append(cases[3])                                                 # identical to the rank-8 case
    return cases


def test_ranks_shapes_duplicates_and_empty_cases(gpu):
    import torch
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    A = _scipy(CASES["grid2k"])
    cases = _shape_list(n)
    b = np.random.default_rng(53).standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        X, rpiv, info = _solve(gpu, F, cases, b, poison=True)
        assert info.max_rank == 16 and info.ncases == len(cases)
        d_x = torch.from_numpy(b.copy()).to("cuda:0")
        F.solve_dev(d_x.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(X[:, 9], d_x.cpu().numpy()), "an empty case must give solve_dev(b) bit for bit"
        assert rpiv[9] == 1.0
        assert np.array_equal(X[:, 10], X[:, 3]) and rpiv[10] == rpiv[3]
        perm = np.random.default_rng(59).permutation(len(cases))
        Xp, rp, _ = _solve(gpu, F, [cases[k] for k in perm], b)
    _assert_parity(A, b, cases, X, rpiv, "shapes")
    merged = (np.array([5, 9]), np.array([7, 5]), np.array([0.125 + 0.25 - 0.0625, 0.1]))
    assert rel_err(X[:, 8], ur.direct_solve(A, merged, b)) <= RTOL
    for k, c in enumerate(perm):
        assert rel_err(Xp[:, k], X[:, c]) <= RTOL and abs(rp[k] - rpiv[c]) <= RTOL


# 3. tiles
def test_tile_widths_agree_and_a_row_may_sit_in_two_tiles(gpu, monkeypatch):
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    A = _scipy(CASES["grid2k"])
    cases = ur.branch_outages(A, 60, seed=61)
    cases.append(cases[0])                                   # its rows come back in the last tile
    b = np.random.default_rng(67).standard_normal(n)
    want = _directs(A, cases, b)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        for tile, min_tiles in (("8", 8), ("64", 2), (None, 1)):
            if tile is None:
                monkeypatch.delenv("CS3_UPD_TILE", raising=False)
            else:
                monkeypatch.setenv("CS3_UPD_TILE", tile)
            X, rpiv, info = _solve(gpu, F, cases, b)
            assert info.ntiles >= min_tiles and (tile is not None or info.ntiles == 1)
            for c in range(len(cases)):
                assert rel_err(X[:, c], want[c]) <= RTOL, (tile, c)
            assert rel_err(X[:, -1], X[:, 0]) <= RTOL


def test_more_touched_rows_than_one_tile_holds(gpu):
    m, n, Ap, Ai, Ax = CASES["grid20k"]
    A = _scipy(CASES["grid20k"])
    cases = ur.branch_outages(A, 560, seed=71)
    b = np.random.default_rng(73).standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        X, rpiv, info = _solve(gpu, F, cases, b)
    assert info.nrows_unique > 1024 and info.ntiles >= 2
    _assert_parity(A, b, cases, X, rpiv, "grid20k, %d rows in %d tiles" % (info.nrows_unique, info.ntiles))


# 4. singular cases
def test_singular_cases_are_flagged_and_the_others_untouched(gpu):
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    A = _scipy(CASES["grid2k"])
    cases = ur.branch_outages(A, 50, seed=79)
    where = (7, 30, 52)
    for k, i in zip(where, (3, n // 2, n - 1)):
        cases.insert(k, ur.singular_case(A, i))
    b = np.random.default_rng(83).standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        X, rpiv, _ = _solve(gpu, F, cases, b)
        X0, rpiv0, _ = _solve(gpu, F, cases, b, sing_tol=0.0)
    assert [c for c in range(len(cases)) if np.isnan(X[:, c]).any()] == list(where)
    _assert_parity(A, b, cases, X, rpiv, "singular", singular=where)
    healthy = [c for c in range(len(cases)) if c not in where]
    assert np.array_equal(X0[:, healthy], X[:, healthy]) and np.array_equal(rpiv0, rpiv)


# 5. one plan across refactorisations
def test_a_plan_survives_refactorisations(gpu):
    import torch
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    rng = np.random.default_rng(89)
    pairs = ur.offdiag_pairs(_scipy(CASES["grid2k"]))
    pairs = pairs[rng.choice(len(pairs), size=100, replace=False)]
    b = rng.standard_normal(n)
    sh = torch.cuda.current_stream().cuda_stream
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        first = [ur.branch_outage(_scipy(CASES["grid2k"]), int(i), int(j)) for i, j in pairs]
        pattern, cx = ur.flatten(first)
        with F.updates_plan(pattern) as plan:
            X, rpiv = F.solve_updates(plan, cx, b, SING_TOL)
            _assert_parity(_scipy(CASES["grid2k"]), b, first, X, rpiv, "first values")
            for fused in (False, True):
                Ax2 = Ax * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=len(Ax)))
                A2 = _scipy((m, n, Ap, Ai, Ax2))
                if fused:
                    d_ax = torch.from_numpy(Ax2.copy()).to("cuda:0")
                    d_x = torch.from_numpy(b.copy()).to("cuda:0")
                    F.factor_solve_dev(d_ax.data_ptr(), d_x.data_ptr(), 1, 1e-3, sh)
                    F.factor_status(sh)
                else:
                    F.factor(Ax2, 1e-3)
                cases2 = [ur.branch_outage(A2, int(i), int(j)) for i, j in pairs]
                _, cx2 = ur.flatten(cases2)
                X2, rpiv2 = F.solve_updates(plan, cx2, b, SING_TOL)
                _assert_parity(A2, b, cases2, X2, rpiv2, "refactored, fused=%s" % fused)


# 6. Cholesky handles
@pytest.mark.parametrize("name", ["spd200", "spd4000"])
def test_cholesky_handles(gpu, name):
    m, n, Ap, Ai, Ax = SPD[name]
    A = _scipy(SPD[name])
    cases = ur.branch_outages(A, 100, seed=97)
    rng = np.random.default_rng(101)
    cases.append((np.array([3, 3, 11]), np.array([8, 40, 2]), 0.05 * rng.standard_normal(3)))      # not symmetric
    b = rng.standard_normal(n)
    with gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY) as F:
        F.factor(Ax)
        X, rpiv, _ = _solve(gpu, F, cases, b)
    _assert_parity(A, b, cases, X, rpiv, name)


# 7. the device form
def test_dev_form_equals_the_host_form_and_later_calls_do_not_allocate(gpu):
    import torch
    m, n, Ap, Ai, Ax = CASES["grid2k"]
    A = _scipy(CASES["grid2k"])
    cases = ur.branch_outages(A, 150, seed=103) + [ur.singular_case(A, 17)]
    pattern, cx = ur.flatten(cases)
    b = np.random.default_rng(107).standard_normal(n)
    dev = torch.device("cuda", 0)
    d_cx, d_b = torch.from_numpy(cx.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        with F.updates_plan(pattern) as plan:
            X, rpiv = F.solve_updates(plan, cx, b, SING_TOL)
            out = []
            side = torch.cuda.Stream()
            for stream in (torch.cuda.current_stream(), side, side):
                d_x = torch.full((n, len(cases)), -7.0, dtype=torch.float64, device=dev)
                d_r = torch.full((len(cases),), -7.0, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                before = F.debug_alloc_counters()
                F.solve_updates_dev(plan, d_cx.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), SING_TOL,
                                    stream.cuda_stream)
                out.append((before, F.debug_alloc_counters()))
                torch.cuda.synchronize()
                assert np.array_equal(d_x.cpu().numpy(), X, equal_nan=True) and np.array_equal(d_r.cpu().numpy(), rpiv)
            assert out[1][0] == out[1][1] and out[2][0] == out[2][1], "a later call allocated or synchronised: %r" % (out,)
            d_x = torch.full((n, len(cases)), -7.0, dtype=torch.float64, device=dev)
            F.solve_updates_dev(plan, d_cx.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 0, SING_TOL)    # rpiv may be null
            torch.cuda.synchronize()
            assert np.array_equal(d_x.cpu().numpy(), X, equal_nan=True)
            assert np.array_equal(d_cx.cpu().numpy(), cx) and np.array_equal(d_b.cpu().numpy(), b)
    assert np.isnan(X[:, -1]).all() and np.isfinite(X[:, :-1]).all()


# 8. the one-call form
def test_cscmat_solve_modified(gpu):
    from csparse3_amd.csc import CscMat
    m, n, Ap, Ai, Ax = CASES["jacobian118"]
    A = _scipy(CASES["jacobian118"])
    cases = ur.branch_outages(A, 20, seed=109)
    b = np.random.default_rng(113).standard_normal(n)
    X, rpiv = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax).solve_modified(b, cases, tol=1e-3, sing_tol=SING_TOL)
    _assert_parity(A, b, cases, X, rpiv, "CscMat.solve_modified")
