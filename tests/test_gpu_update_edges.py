"""Low-rank-modified solves (cs3_updates_*) on the GPU at their engineered edges: the case lists of
tests/update_cases.py -- what each is there for is asserted from the reference alone in tests/test_update_cases_cpu.py.
Every case of every list: X within helpers.RTOL of a factorisation of its own modified matrix, rpiv within RTOL of the
NumPy reference (tests/updates_ref.py); LDS is poisoned before every solve."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import RTOL, rel_err
import update_cases as uc
import updates_ref as ur

pytestmark = pytest.mark.gpu

SING_TOL = 1e-10


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


def _factored(gpu, B, spd=False):
    F = gpu.Factorization(B.m, B.n, B.Ap, B.Ai, kind=gpu.CS3_CHOLESKY if spd else gpu.CS3_LU)
    return F.factor(B.Ax) if spd else F.factor(B.Ax, 1e-3)


@pytest.fixture(scope="module")
def held(gpu):
    """held(n, spd) -> the factored handle of update_cases.base(n, spd), made once for the module."""
    handles = {}

    def get(n, spd=False):
        if (n, spd) not in handles:
            handles[(n, spd)] = _factored(gpu, uc.base(n, spd), spd)
        return handles[(n, spd)]
    yield get
    for F in handles.values():
        F.close()


def _solve(gpu, F, cases, b, sing_tol=SING_TOL):
    """-> X, rpiv, tiles of the list's plan."""
    pattern, cx = ur.flatten(cases)
    with F.updates_plan(pattern) as plan:
        _poison(gpu)
        X, rpiv = F.solve_updates(plan, cx, b, sing_tol)
        return X, rpiv, [tuple(t) for t in plan.tiles().tolist()]


def _nan_columns(X):
    assert np.array_equal(np.isnan(X).any(axis=0), np.isnan(X).all(axis=0)), "a column is NaN in part"
    return np.flatnonzero(np.isnan(X).any(axis=0)).tolist()


def _assert_parity(B, cases, X, rpiv, what, flagged=()):
    """Every case outside `flagged`: X within RTOL of the direct solve, rpiv within RTOL of the reference's."""
    healthy = [c for c in range(len(cases)) if c not in flagged]
    with ThreadPoolExecutor(8) as pool:
        want = list(pool.map(lambda c: ur.direct_solve(B.A, cases[c], B.b), healthy))
    _, rpiv_ref, _ = ur.solve_updates_ref(B.A, B.b, cases, SING_TOL)
    assert X.shape == (B.n, len(cases)) and _nan_columns(X) == sorted(flagged), what
    worst = 0.0
    for c, w in zip(healthy, want):
        err = rel_err(X[:, c], w)
        worst = max(worst, err)
        assert err <= RTOL, "%s case %d: relative error %.3e" % (what, c, err)
        assert abs(rpiv[c] - rpiv_ref[c]) <= RTOL, "%s case %d: rpiv %.17g vs %.17g" % (what, c, rpiv[c], rpiv_ref[c])
    print("%s: %d cases, worst relative error %.2e, smallest healthy rpiv %.2e" % (what, len(cases), worst, rpiv[healthy].min()))


def _set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    else:
        monkeypatch.setenv("CS3_UPD_TILE", str(tile))


# 1. pivoting: a swap at every step, the smallest pivot inside, s > r, a tie, the rectangular shapes
@pytest.mark.parametrize("tile", [None, 16])
@pytest.mark.parametrize("spd", [False, True], ids=["lu", "cholesky"])
def test_designed_pivoting(gpu, held, monkeypatch, spd, tile):
    B = uc.base(uc.N_PIVOT, spd)
    designed = uc.pivot_cases(uc.N_PIVOT, spd)
    cases = [d.case for d in designed]
    _set_tile(monkeypatch, tile)
    X, rpiv, tiles = _solve(gpu, held(uc.N_PIVOT, spd), cases, B.b)
    if tile is None:
        assert len(tiles) == 1
    else:                                                   # every rank-16 case alone in a tile it fills
        full = [c for c, d in enumerate(designed) if len(np.unique(d.case[0])) == 16]
        assert len(full) >= 5 and all((c, 1, 16, 16) in tiles for c in full), tiles
    _assert_parity(B, cases, X, rpiv, "pivoting, %s, tile %s" % ("cholesky" if spd else "lu", tile))
    for c, d in enumerate(designed):
        if d.small:
            assert 1e-4 <= rpiv[c] <= 1e-2, (d.name, rpiv[c])


# 2. rows: partial stages (n mod 8), partial row blocks (n mod 128), the odd tail of a stage
@pytest.mark.parametrize("n", uc.ROW_ORDERS)
def test_row_counts_at_even_and_odd_widths(gpu, held, monkeypatch, n):
    """Width 9 is what a tile gets while the largest rank is at most 9 (n = 1 .. 9 here); with a rank-16 case the tile
    is 16 wide, so 17 is the odd width of n = 127, 129 and 137: an odd width times an odd number of rows in the last
    stage is what sends an entry of Z through thread 0."""
    B = uc.base(n)
    cases = uc.row_list(n)
    got = {}
    for tile in (None, 9, 17):
        _set_tile(monkeypatch, tile)
        X, rpiv, tiles = _solve(gpu, held(n), cases, B.b)
        want = {None: 64, 9: 9 if n <= 9 else 16, 17: 17}[tile]
        assert all(t[3] == want for t in tiles), (tile, tiles)
        _assert_parity(B, cases, X, rpiv, "n = %d, tile %s" % (n, tile))
        got[tile] = X
    for tile in (9, 17):
        for c in range(len(cases)):
            assert rel_err(got[tile][:, c], got[None][:, c]) <= RTOL, (tile, c)


# 3. cases per tile and touched rows per tile
@pytest.mark.parametrize("name", list(uc.tile_lists()))
def test_tile_edges(gpu, held, monkeypatch, name):
    _set_tile(monkeypatch, None)
    B = uc.base(uc.N_TILES)
    cases, want_tiles = uc.tile_lists()[name]
    X, rpiv, tiles = _solve(gpu, held(uc.N_TILES), cases, B.b)
    assert tiles == want_tiles
    _assert_parity(B, cases, X, rpiv, name)
    if name == "ranks_0_1_16":
        x0 = B.lu.solve(B.b)
        for c in (0, 3, 7):
            assert rpiv[c] == 1.0 and rel_err(X[:, c], x0) <= RTOL and np.array_equal(X[:, c], X[:, 0])


def test_flagged_lanes_are_nan_and_the_others_keep_their_bits(gpu, held, monkeypatch):
    _set_tile(monkeypatch, None)
    B = uc.base(uc.N_PIVOT)
    cases, twin, lanes = uc.flagged_lists()
    F = held(uc.N_PIVOT)
    X, rpiv, tiles = _solve(gpu, F, cases, B.b)
    Xt, rpivt, _ = _solve(gpu, F, twin, B.b)
    assert len(tiles) == 1 and tiles[0][1] == uc.FLAGGED_NC
    assert _nan_columns(X) == list(lanes) and _nan_columns(Xt) == []
    assert np.all(np.abs(rpiv[list(lanes)]) <= 1e-13)
    others = np.setdiff1d(np.arange(len(cases)), lanes)
    assert np.array_equal(X[:, others], Xt[:, others]) and np.array_equal(rpiv[others], rpivt[others])
    _assert_parity(B, cases, X, rpiv, "flagged lanes", flagged=lanes)


# 4. the threshold
def test_threshold_at_equality(gpu, held, monkeypatch):
    _set_tile(monkeypatch, None)
    B = uc.base(uc.N_PIVOT)
    designed = uc.pivot_cases(uc.N_PIVOT)
    cases = [d.case for d in designed] + [ur.singular_case(B.A, 20), ur.singular_case(B.A, 99)]
    c = [d.name for d in designed].index("small8")
    F = held(uc.N_PIVOT)
    X0, rpiv0, _ = _solve(gpu, F, cases, B.b, sing_tol=0.0)
    assert _nan_columns(X0) == np.flatnonzero(rpiv0 == 0.0).tolist()
    nd = len(designed)
    assert np.all(np.abs(rpiv0[nd:]) <= 1e-13)
    _assert_parity(B, cases[:nd], X0[:, :nd], rpiv0[:nd], "threshold, sing_tol = 0")
    for tol in (rpiv0[c], np.nextafter(rpiv0[c], 0.0), -1.0, -np.inf):
        X, rpiv, _ = _solve(gpu, F, cases, B.b, sing_tol=tol)
        want = np.flatnonzero((rpiv0 == 0.0) | ((rpiv0 <= tol) if tol > 0 else False)).tolist()
        assert _nan_columns(X) == want, (tol, _nan_columns(X), want)
        assert (c in want) == (tol == rpiv0[c])
        keep = np.setdiff1d(np.arange(len(cases)), want)
        assert np.array_equal(X[:, keep], X0[:, keep]) and np.array_equal(rpiv, rpiv0), tol


def test_only_an_exact_zero_is_flagged_without_a_threshold(gpu):
    B = uc.base_exact_zero()
    i = uc.ZERO_ROW
    rng = np.random.default_rng(7800000)
    cases = [uc.light(rng, (1, 2, 3)), (np.array([i]), np.array([i]), np.array([-2.0])), uc.light(rng, (i, 8))]
    with _factored(gpu, B) as F:
        for tol in (-1.0, 0.0, SING_TOL):
            X, rpiv, _ = _solve(gpu, F, cases, B.b, sing_tol=tol)
            assert rpiv[1] == 0.0, "S = 1 + (-2)(1/2) must be an exact zero: %.17g" % rpiv[1]
            _assert_parity(B, cases, X, rpiv, "exact zero, sing_tol = %g" % tol, flagged=(1,))


# 5. the handle's Z grows when a wider plan follows a narrower one
def test_plans_of_different_widths_on_one_handle(gpu, monkeypatch):
    _set_tile(monkeypatch, None)
    B = uc.base(uc.N_TILES)
    L = uc.tile_lists()
    narrow, wide = L["cases1"][0], L["cases64_rows1024"][0]
    fresh = {}
    for name, cases in (("narrow", narrow), ("wide", wide)):
        with _factored(gpu, B) as F:
            fresh[name] = _solve(gpu, F, cases, B.b)
    assert fresh["narrow"][2][0][3] == 64 and fresh["wide"][2][0][3] == 1024
    with _factored(gpu, B) as F:
        for name, cases in (("narrow", narrow), ("wide", wide), ("narrow", narrow), ("wide", wide)):
            X, rpiv, tiles = _solve(gpu, F, cases, B.b)
            assert np.array_equal(X, fresh[name][0]) and np.array_equal(rpiv, fresh[name][1]) and tiles == fresh[name][2], name


# 6. a NaN among a case's values
def _with_nan(case, p):
    vals = case[2].copy()
    vals[p] = np.nan
    return case[0], case[1], vals


@pytest.mark.parametrize("tol", [0.0, SING_TOL])
def test_a_nan_value_flags_its_case_and_no_other(gpu, held, monkeypatch, tol):
    """One NaN triplet in row 0 of a rank-3 case, in its last row, and in row 7 of a rank-16 case: the case's column and
    its rpiv are NaN whatever sing_tol is, every other case keeps its bits."""
    _set_tile(monkeypatch, None)
    B = uc.base(uc.N_PIVOT)
    by_name = {d.name: d.case for d in uc.pivot_cases(uc.N_PIVOT)}
    cases = [by_name[k] for k in ("cyclic5", "cyclic3", "small5", "cyclic16", "rect3x16", "cyclic8")]
    F = held(uc.N_PIVOT)
    X0, rpiv0, _ = _solve(gpu, F, cases, B.b, sing_tol=tol)
    assert _nan_columns(X0) == []
    for hit in ({1: 1}, {1: 8}, {3: 7 * 16 + 5}, {1: 0, 3: 255}):          # case -> triplet (row-major in the block)
        poisoned = [_with_nan(case, hit[c]) if c in hit else case for c, case in enumerate(cases)]
        X, rpiv, _ = _solve(gpu, F, poisoned, B.b, sing_tol=tol)
        assert _nan_columns(X) == sorted(hit), (hit, _nan_columns(X))
        assert np.flatnonzero(np.isnan(rpiv)).tolist() == sorted(hit), (hit, rpiv)
        keep = np.setdiff1d(np.arange(len(cases)), list(hit))
        assert np.array_equal(X[:, keep], X0[:, keep]) and np.array_equal(rpiv[keep], rpiv0[keep]), hit
