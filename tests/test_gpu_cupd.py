"""Complex low-rank-modified solves (cs3_cplx_updates_*) on the GPU.

Accuracy against dense NumPy complex128 within 1e3 cond_1(A + dA_c) 2^-53 max |x_c| on the networks (every single-branch
outage, pairs and triples, a Hermitian positive definite matrix through Cholesky with a non-Hermitian dA, a rotated
handle with tol = 1e-3); the engineered edges within RTOL = 1e-10: designed S (a swap at every step, the smallest pivot
at an interior step, two candidates of the same bits, cabs1 against the modulus, rectangular blocks), the orders around
the stage and the row block of k_cupd_apply, odd widths, the tile and lane edges at n = 1100, flagged lanes, the exact
zero, sing_tol at its threshold, NaN containment.  Bit for bit: the units tile and rpiv against tests/cupd_ref.py driven
by the handle's own solve, an empty case against solve_dev, host against device form, narrow and wide plans interleaved
against fresh handles, a refactorisation, and no allocation or synchronisation on the second call."""
import numpy as np
import pytest

import cplx_ref as ref
import csens_ref
import cupd_cases as cc
import cupd_ref as cr
from helpers import RTOL

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def handle_solve(F):
    """solve(T [2n, w], trans): the real handle's solve_dev at the tile's width."""
    import torch

    def solve(Tl, trans):
        d = torch.from_numpy(np.ascontiguousarray(Tl)).to("cuda:0")
        F.real.solve_dev(d.data_ptr(), Tl.shape[1], _stream(), trans=trans)
        torch.cuda.synchronize()
        return d.cpu().numpy()
    return solve


def factored(gpu, B, kind="lu", rotate=True, tol=0.0):
    return gpu.ComplexFactorization(B.n, B.Ap, B.Ai, kind=gpu.CS3_CHOLESKY if kind == "chol" else gpu.CS3_LU, rotate=rotate).factor(B.Az, tol)


@pytest.fixture(scope="module")
def made(gpu):
    handles = {}

    def get(key, B, **kw):
        if key not in handles:
            handles[key] = factored(gpu, B, **kw)
        return handles[key]
    yield get
    for F in handles.values():
        F.close()


def host_call(F, cases, b, sing_tol=0.0):
    lists, cz = cr.flatten(cases)
    with F.updates_plan(lists) as plan:
        X, rpiv = F.solve_updates(plan, cz, b, sing_tol)
        return X, rpiv, plan.tiles()


def dev_call(F, plan, cz, b, sing_tol=0.0, parts=None):
    """The device form into an X with a NaN guard behind it.  -> (X, rpiv, guard intact)."""
    import torch
    n, nc = F.n, plan.ncases
    d_cz = torch.from_numpy(np.ascontiguousarray(np.concatenate([cz, [0]]), dtype=np.complex128)).to("cuda:0")
    d_b = torch.from_numpy(np.array(b, dtype=np.complex128)).to("cuda:0")
    d_x = torch.full((n * nc + 2,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda:0")
    d_r = torch.full((nc + 1,), float("nan"), dtype=torch.float64, device="cuda:0")
    args = (d_cz.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), sing_tol, _stream())
    if parts is None:
        F.solve_updates_dev(plan, *args)
    else:
        F.debug_updates_parts(plan, parts, *args)
    torch.cuda.synchronize()
    x, r = d_x.cpu().numpy(), d_r.cpu().numpy()
    return x[:n * nc].reshape(n, nc), r[:nc], bool(np.isnan(x[n * nc:]).all() and np.isnan(r[nc]))


def restated(F, B, cases, tiles, sing_tol=0.0):
    s = F.plan.rotation()[0]
    sr, si = ref.split(s)
    return cr.solve_restated(B.n, cases, [tuple(int(v) for v in t) for t in tiles], B.b, sr, si, handle_solve(F), sing_tol)


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check_bits_and_tolerance(F, B, cases, sing_tol=0.0, name=""):
    """rpiv bit for bit against the restatement on the handle's own solves; X within RTOL of the dense reference."""
    X, rpiv, tiles = host_call(F, cases, B.b, sing_tol)
    Xr, rr, caps, _ = restated(F, B, cases, tiles, sing_tol)
    assert csens_ref.same(rpiv, rr), (name, "rpiv")
    print("%s: X %s the restatement bit for bit" % (name, "equals" if np.array_equal(csens_ref.canon_bits(X), csens_ref.canon_bits(Xr)) else "differs from"))
    want = cr.x_woodbury(B.inv, B.inv @ B.b, cases)
    for c in range(len(cases)):
        if caps[c].flag:
            assert np.isnan(X[:, c].real).all() and np.isnan(X[:, c].imag).all(), (name, c)
        else:
            assert rel(X[:, c], want[:, c]) <= RTOL and rel(X[:, c], Xr[:, c]) <= RTOL, (name, c)
    return X, rpiv, tiles


# ---- accuracy ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,tol", [("ybus40", 0.0), ("ybus40_lossless", 0.0), ("ybus300", 0.0), ("hermitian_pd", 0.0), ("ybus40", 1e-3)])
def test_accuracy_against_dense_numpy(gpu, made, monkeypatch, name, tol):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B, cases = cc.accuracy_lists(name)
    _, kind, rotate = cc.network(name)
    F = made((name, tol), B, kind=kind, rotate=rotate, tol=tol)
    X, rpiv, tiles = host_call(F, cases, B.b)
    worst = 0.0
    for c, case in enumerate(cases):
        want, cond1 = cr.x_dense(B.A, case, B.b)
        worst = max(worst, float(np.abs(X[:, c] - want).max()) / cr.accuracy_bound(cond1, want))
    print("%s tol %g: %d cases in %d tile(s), smallest rpiv %.2e, worst error / bound %.2e" % (name, tol, len(cases), len(tiles), rpiv.min(), worst))
    assert worst <= 1.0 and rpiv.min() >= 1e-3


def test_cross_check_against_the_real_plan_on_the_real_form(gpu, made, monkeypatch):
    """Two independent routes: the complex plan, and the real plan on F.real with diag(s) dA expanded on the host into
    2 x 2 blocks (rank <= 8 complex, so that 2 r <= 16)."""
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B, cases = cc.accuracy_lists("ybus40")
    F = made(("ybus40", 0.0), B)
    cases = [c for c in cases if len(np.unique(c[0])) <= 8 and len(np.unique(c[1])) <= 8]
    X, rpiv, _ = host_call(F, cases, B.b)
    s = F.plan.rotation()[0]
    real_cases = []
    for rows, cols, vals in cases:
        w = s[rows] * vals
        real_cases.append((np.concatenate([2 * rows, 2 * rows, 2 * rows + 1, 2 * rows + 1]),
                           np.concatenate([2 * cols, 2 * cols + 1, 2 * cols, 2 * cols + 1]),
                           np.concatenate([w.real, -w.imag, w.imag, w.real])))
    with F.real.updates_plan([(c[0], c[1]) for c in real_cases]) as plan:
        XR, _ = F.real.solve_updates(plan, np.concatenate([c[2] for c in real_cases]), F.plan.pack(B.b))
    XC = XR[0::2] + 1j * XR[1::2]
    for c, case in enumerate(cases):
        want, cond1 = cr.x_dense(B.A, case, B.b)
        bound = cr.accuracy_bound(cond1, want)
        assert float(np.abs(XC[:, c] - want).max()) <= bound and float(np.abs(X[:, c] - XC[:, c]).max()) <= bound, c


# ---- designed S -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [None, 16])
def test_designed_capacitance_systems(gpu, made, monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    else:
        monkeypatch.setenv("CS3_UPD_TILE", str(tile))
    B = cc.base(cc.N_PIVOT)
    F = made("pivot", B)
    designed = cc.pivot_cases()
    X, rpiv, tiles = check_bits_and_tolerance(F, B, [d.case for d in designed], name="designed, tile %s" % tile)
    assert (len(tiles) == 1) == (tile is None)
    for c, d in enumerate(designed):
        if d.small:
            assert 1e-4 <= rpiv[c] <= 1e-2, d.name
        if d.name == "cabs1":                              # 0.6 + 0.6j was taken, not 1.0
            assert abs(rpiv[c] - cc.CABS1_RPIV) <= 1e-9, rpiv[c]


# ---- orders and widths ------------------------------------------------------------------------------------------------------

def test_orders_around_the_stage_and_the_row_block(gpu, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    lim = gpu.cplx_updates_limits()
    orders = cc.row_orders(lim)
    assert 1 in orders and lim.apply_stage + 1 in orders and lim.apply_rows - 1 in orders
    for n in orders:
        B = cc.base(n)
        with factored(gpu, B) as F:
            assert np.any(F.plan.rotation()[0] != 1.0)
            check_bits_and_tolerance(F, B, cc.row_list(n), name="n = %d" % n)


@pytest.mark.parametrize("name", sorted(cc.odd_width_lists()))
def test_odd_widths(gpu, made, monkeypatch, name):
    cases, env, tiles = cc.odd_width_lists()[name]
    monkeypatch.setenv("CS3_UPD_TILE", str(env))
    B = cc.base(cc.N_PIVOT)
    _, _, got = check_bits_and_tolerance(made("pivot", B), B, cases, name=name)
    assert [tuple(int(v) for v in t) for t in got] == [tuple(t) for t in tiles]


# ---- tiles and lanes at n = 1100 --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(gpu, made):
    B = cc.base(cc.N_TILES)
    return B, made("tiles", B), B.inv @ B.b


@pytest.mark.parametrize("name", sorted(cc.tile_lists()))
def test_tile_and_lane_edges(gpu, big, monkeypatch, name):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B, F, x0 = big
    cases, tiles = cc.tile_lists()[name]
    X, rpiv, got = host_call(F, cases, B.b)
    assert [tuple(int(v) for v in t) for t in got] == [tuple(t) for t in tiles]
    want = cr.x_woodbury(B.inv, x0, cases)
    err = np.abs(X - want).max(axis=0) / np.abs(want).max(axis=0)
    assert err.max() <= RTOL, (name, int(np.argmax(err)), err.max())
    empty = [c for c, case in enumerate(cases) if len(case[0]) == 0]
    assert np.all(rpiv[empty] == 1.0) and np.all(rpiv > 0.1)


# ---- flagged lanes, the exact zero, sing_tol, NaN ---------------------------------------------------------------------------

def test_flagged_lanes_leave_their_neighbours_alone(gpu, made, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base(cc.N_PIVOT)
    F = made("pivot", B)
    cases, twin, lanes = cc.flagged_lists()
    X, rpiv, tiles = host_call(F, cases, B.b, 1e-10)
    Xt, rt, _ = host_call(F, twin, B.b, 1e-10)
    assert len(tiles) == 1 and len(cases) == cc.FLAGGED_NC
    bad = np.isnan(X.real) & np.isnan(X.imag)
    assert sorted(np.flatnonzero(bad.all(axis=0))) == sorted(lanes) and not np.isnan(np.delete(X, lanes, axis=1)).any()
    assert np.all(rpiv[list(lanes)] <= 1e-13)
    keep = np.setdiff1d(np.arange(len(cases)), lanes)
    assert csens_ref.same(X[:, keep], Xt[:, keep]) and csens_ref.same(rpiv[keep], rt[keep])


def test_the_exact_zero_pivot(gpu, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base_exact_zero()
    with factored(gpu, B) as F:
        assert F.plan.rotation()[0][cc.ZERO_ROW] == -1j
        X, rpiv, _ = host_call(F, [cc.EMPTY, cc.EXACT_ZERO_CASE, cc.EMPTY], B.b, 0.0)
        assert rpiv[1] == 0.0 and np.isnan(X[:, 1].real).all() and np.isnan(X[:, 1].imag).all()
        assert list(rpiv[[0, 2]]) == [1.0, 1.0] and csens_ref.same(X[:, 0], X[:, 2]) and rel(X[:, 0], B.inv @ B.b) <= RTOL


def test_sing_tol_at_its_threshold(gpu, made, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base(cc.N_PIVOT)
    F = made("pivot", B)
    cases = [d.case for d in cc.pivot_cases() if d.small or d.name == "cabs1"]
    X, rpiv, _ = host_call(F, cases, B.b)
    assert not np.isnan(X).any()
    for c in range(len(cases)):
        at, _, _ = host_call(F, cases, B.b, float(rpiv[c]))                          # rpiv <= sing_tol flags ...
        flagged = np.flatnonzero(np.isnan(at).all(axis=0))
        assert c in flagged and set(flagged) == {k for k in range(len(cases)) if rpiv[k] <= rpiv[c]}
        below, rb, _ = host_call(F, cases, B.b, float(np.nextafter(rpiv[c], 0.0)))   # ... one ulp lower does not
        assert not np.isnan(below[:, c]).any() and csens_ref.same(below[:, c], X[:, c]) and csens_ref.same(rb, rpiv)


def test_nan_values_stay_in_their_case(gpu, made, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base(cc.N_PIVOT)
    F = made("pivot", B)
    for cases, bad in cc.nan_lists():
        clean = list(cases)
        clean[bad] = cc.EMPTY
        for sing_tol in (0.0, 1e-10):
            X, rpiv, _ = host_call(F, cases, B.b, sing_tol)
            Xc, rc, _ = host_call(F, clean, B.b, sing_tol)
            assert np.isnan(rpiv[bad]) and np.isnan(X[:, bad].real).all() and np.isnan(X[:, bad].imag).all()
            keep = np.setdiff1d(np.arange(len(cases)), [bad])
            assert csens_ref.same(X[:, keep], Xc[:, keep]) and csens_ref.same(rpiv[keep], rc[keep])


# ---- bit for bit ------------------------------------------------------------------------------------------------------------

def test_units_tile_and_an_empty_case(gpu, made, monkeypatch):
    import torch
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base(cc.N_PIVOT)
    F = made("pivot", B)
    cases = cc.row_list(cc.N_PIVOT) + [cc.EMPTY]
    lists, cz = cr.flatten(cases)
    sr, si = ref.split(F.plan.rotation()[0])
    with F.updates_plan(lists) as plan:
        tiles = plan.tiles()
        _, _, intact = dev_call(F, plan, cz, B.b, parts=1)
        w = int(tiles[-1, 3])
        got = F.real.debug_sens_tile((2 * B.n, w))
        want = cr.units(B.n, cr.tile_columns(cases, [tuple(int(v) for v in t) for t in tiles])[-1], sr, si)
        assert intact and csens_ref.same(got, want)
        assert np.count_nonzero(got) >= int(tiles[-1, 2]) and np.any((got != 0) & (got != 1))      # s != 1 on touched rows
        X, rpiv, intact = dev_call(F, plan, cz, B.b)
        Xh, rh = F.solve_updates(plan, cz, B.b)
        assert intact and csens_ref.same(X, Xh) and csens_ref.same(rpiv, rh)                       # host form == device form
    d_b = torch.from_numpy(np.array(B.b)).to("cuda:0")
    d_x = torch.empty_like(d_b)
    F.solve_dev(d_b.data_ptr(), d_x.data_ptr(), 1, _stream())
    torch.cuda.synchronize()
    assert csens_ref.same(X[:, -1], d_x.cpu().numpy()) and rpiv[-1] == 1.0                         # an empty case == solve_dev


def test_narrow_and_wide_plans_interleaved_refactorisation_and_no_allocation(gpu, monkeypatch):
    monkeypatch.delenv("CS3_UPD_TILE", raising=False)
    B = cc.base(cc.N_TILES)
    narrow, _ = cc.tile_lists()["cases1"]
    wide, _ = cc.tile_lists()["cases64_rows1024"]
    ln, czn = cr.flatten(narrow)
    lw, czw = cr.flatten(wide)
    Az2 = B.Az * (1.0 + 0.05 * np.cos(np.arange(len(B.Az))))
    with factored(gpu, B) as F1, factored(gpu, B) as F2:
        with F1.updates_plan(ln) as pn, F1.updates_plan(lw) as pw, F2.updates_plan(lw) as qw:
            assert int(pn.tiles()[0, 3]) == 64 and int(pw.tiles()[0, 3]) == 1024
            first = [dev_call(F1, pn, czn, B.b), dev_call(F1, pw, czw, B.b)]
            again = [dev_call(F1, pn, czn, B.b), dev_call(F1, pw, czw, B.b)]
            fresh = dev_call(F2, qw, czw, B.b)                                                     # a handle that never saw the narrow plan
            for a, b in zip(first, again):
                assert a[2] and b[2] and csens_ref.same(a[0], b[0]) and csens_ref.same(a[1], b[1])
            assert csens_ref.same(first[1][0], fresh[0]) and csens_ref.same(first[1][1], fresh[1])
            before = F1.real.debug_alloc_counters()
            dev_call(F1, pn, czn, B.b)
            dev_call(F1, pw, czw, B.b)
            assert F1.real.debug_alloc_counters() == before                                        # nothing allocates or synchronises
            F1.factor(Az2)                                                                         # new values: the plan stays, s is new
            F2.factor(Az2)
            X1, r1, ok = dev_call(F1, pw, czw, B.b)
            X2, r2, _ = dev_call(F2, qw, czw, B.b)
            assert ok and csens_ref.same(X1, X2) and csens_ref.same(r1, r2) and not np.array_equal(X1, fresh[0])
            A2 = ref.dense_complex(B.n, B.Ap, B.Ai, Az2)
            inv2 = np.linalg.inv(A2)
            want = cr.x_woodbury(inv2, inv2 @ B.b, wide)
            assert rel(X1, want) <= RTOL
