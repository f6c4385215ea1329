"""Complex low-rank-modified solves (cs3_cplx_updates_*), the part that needs no GPU: the plan through the C ABI equals the
real plan on the same lists; every plan check in its documented order; the restatement (tests/cupd_ref.py) with Z from a
dense inverse stays within the accuracy bound on every accuracy case -- the proof that the inputs suit the bound the GPU
tests hold the device to --; and the pivot counter asserts from the restatement's own S what each designed case is there
for, with a margin between the two best candidates that rounding cannot cross."""
import ctypes as C

import numpy as np
import pytest

import csens_cases
import cupd_cases as cc
import cupd_ref as cr
import update_cases as uc

SYMBOLS = ("cs3_cplx_updates_limits", "cs3_cplx_updates_plan", "cs3_cplx_updates_free", "cs3_cplx_updates_info",
           "cs3_debug_cplx_updates_tiles", "cs3_cplx_updates_solve_dev", "cs3_cplx_updates_solve", "cs3_debug_cplx_updates_parts")
MARGIN = 1e-6              # relative gap between the two best pivot candidates: ten orders above the rounding of S


def test_the_new_symbols_are_exported_and_the_limits_are_consistent(hip):
    for name in SYMBOLS:
        assert hasattr(hip.lib(), name), "libcsparse3_hip.so does not export " + name
    lim = hip.cplx_updates_limits()
    assert C.sizeof(hip.CplxUpdatesLimits) == 8 * 8
    assert (lim.max_rank, lim.max_tile, lim.max_tile_cases) == (uc.MAX_RANK, uc.MAX_TILE, uc.MAX_TILE_CASES)
    assert lim.apply_rows % lim.apply_stage == 0 and lim.apply_threads_min % 64 == 0 and lim.apply_threads_min <= 1024
    assert 2 * lim.apply_stage * lim.max_tile * 8 <= 160 * 1024                        # a stage of row pairs fits the LDS
    assert lim.apply_stage * lim.max_tile % lim.apply_threads_min == 0                 # ... and whole 16-byte loads per thread
    assert hip.lib().cs3_cplx_updates_limits(None) == hip.CS3_ERR_ARG


# ---- the plan is the real plan ---------------------------------------------------------------------------------------------

def _lists():
    out = [(name, cases, None, tiles) for name, (cases, tiles) in cc.tile_lists().items()]
    out += [(name, cases, env, tiles) for name, (cases, env, tiles) in cc.odd_width_lists().items()]
    return out


def test_the_plan_equals_the_real_plan_on_every_list(hip, monkeypatch):
    n = cc.N_TILES
    B, R = cc.base(n), uc.base(n)
    with hip.ComplexFactorization(n, B.Ap, B.Ai) as F, hip.Factorization(n, n, R.Ap, R.Ai) as FR:
        for name, cases, env, tiles in _lists():
            if env is None:
                monkeypatch.delenv("CS3_UPD_TILE", raising=False)
            else:
                monkeypatch.setenv("CS3_UPD_TILE", str(env))
            rc_lists = [(c[0], c[1]) for c in cases]
            with F.updates_plan(rc_lists) as plan, FR.updates_plan(rc_lists) as real:
                got, want = plan.tiles(), real.tiles()
                assert np.array_equal(got, want), name
                assert [tuple(int(v) for v in row) for row in got] == [tuple(t) for t in tiles], name
                a, b = plan.info, real.info
                assert (a.ncases, a.nrows_unique, a.max_rank, a.ntiles) == (b.ncases, b.nrows_unique, b.max_rank, b.ntiles), name
                cols = cr.tile_columns(cases, got)                                     # the restatement's tile columns agree
                assert [len(c) for c in cols] == [int(w) for w in got[:, 3]], name


# ---- refusals --------------------------------------------------------------------------------------------------------------

def _plan_rc(hip, p, h, ncases, cp, ci, cj, out=True):
    lib = hip.lib()
    u = C.c_void_p()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    cp, ci, cj = arr(cp), arr(ci), arr(cj)
    rc = lib.cs3_cplx_updates_plan(p, h, ncases, hip._pi(cp), hip._pi(ci), hip._pi(cj), C.byref(u) if out else None)
    msg = lib.cs3_last_error().decode()
    if u:
        lib.cs3_cplx_updates_free(u)
    return rc, msg


def test_plan_refusals_in_their_documented_order(hip):
    n, Ap, Ai, _ = csens_cases.ybus40()
    E = hip.CS3_ERR_ARG
    ok = (2, [0, 2, 3], [1, 2, 3], [2, 1, 3])
    seventeen = (2, [0, 1, 18], [0] + list(range(17)), [0] + [5] * 17)
    with hip.ComplexFactorization(n, Ap, Ai) as F, hip.ComplexFactorization(n, Ap, Ai, batch=2) as F2, \
            hip.ComplexFactorization(n, Ap, Ai, schur=csens_cases.BORDER) as FS, hip.Factorization(n, n, Ap, Ai) as R:
        p, h = F.plan._p, F.real._h
        assert _plan_rc(hip, p, h, *ok)[0] == 0
        # each call is wrong in everything that comes later as well
        for pp, hh in ((None, R._h), (p, None)):
            rc, msg = _plan_rc(hip, pp, hh, 0, [1, 0], None, None)
            assert rc == E and "null plan or handle" in msg
        rc, msg = _plan_rc(hip, p, R._h, 0, [1, 0], None, None, out=False)
        assert rc == E and "null output" in msg
        rc, msg = _plan_rc(hip, p, R._h, 0, None, None, None)
        assert rc == E and "null case pointers" in msg
        rc, msg = _plan_rc(hip, p, R._h, 0, [1, 0], None, None)
        assert rc == E and "not 2 n" in msg
        for bad in (0, -3):
            rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, bad, [1, 0], None, None)
            assert rc == E and "ncases must be >= 1" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 2, [1, 1, 2], None, None)
        assert rc == E and "cp[0] != 0" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 2, [0, 2, 1], None, None)
        assert rc == E and "cp not monotone at case 1" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 2, [0, 1, 2], [0, n], None)
        assert rc == E and "null index arrays" in msg
        for ci, cj in (([0, n], [0, 0]), ([0, 0], [0, -1])):       # n is a row of the handle (order 2n), not of the matrix
            rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 2, [0, 1, 2], ci, cj)
            assert rc == E and "index out of range in case 1" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, *seventeen)
        assert rc == E and "case 1 touches 17 rows and 1 columns" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 2, [0, 1, 18], seventeen[3], seventeen[2])
        assert rc == E and "case 1 touches 1 rows and 17 columns" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, *ok)
        assert rc == E and "batch > 1" in msg
        rc, msg = _plan_rc(hip, FS.plan._p, FS.real._h, *ok)
        assert rc == E and "border" in msg
        rc, msg = _plan_rc(hip, p, FS.real._h, *ok)
        assert rc == E and "Schur handle" in msg
        # sixteen of each is the limit, and an empty list of triplets needs no index arrays
        assert _plan_rc(hip, p, h, 1, [0, 16], list(range(16)), list(range(16)))[0] == 0
        assert _plan_rc(hip, p, h, 2, [0, 0, 0], None, None)[0] == 0


def test_solve_refusals_need_no_gpu_either(hip):
    n, Ap, Ai, _ = csens_cases.ybus40()
    lib = hip.lib()
    buf = np.zeros(4 * n, dtype=np.complex128)
    with hip.ComplexFactorization(n, Ap, Ai) as F, hip.ComplexFactorization(n, Ap, Ai) as G:
        with F.updates_plan([([1, 2], [2, 1])]) as plan:
            def rc_of(p, h, u, cz=buf, b=buf, X=buf):
                f64 = lambda a: None if a is None else hip._pc(a)      # noqa: E731
                rc = lib.cs3_cplx_updates_solve(p, h, u, f64(cz), f64(b), 0.0, f64(X), None)
                return rc, lib.cs3_last_error().decode()
            p, h, u = F.plan._p, F.real._h, plan._u
            assert rc_of(None, h, u) == (hip.CS3_ERR_ARG, "cs3_cplx_updates_solve: null complex plan")
            assert rc_of(p, None, u)[0] == hip.CS3_ERR_ARG
            assert rc_of(p, h, None) == (hip.CS3_ERR_ARG, "cs3_cplx_updates_solve: null plan")
            for kw in ({"cz": None}, {"b": None}, {"X": None}):
                assert rc_of(p, h, u, **kw) == (hip.CS3_ERR_ARG, "cs3_cplx_updates_solve: null argument")
            assert rc_of(p, G.real._h, u) == (hip.CS3_ERR_ARG, "cs3_cplx_updates_solve: the plan was made for another handle")
            assert rc_of(G.plan._p, h, u) == (hip.CS3_ERR_ARG, "cs3_cplx_updates_solve: the plan was made for another complex plan")
            assert rc_of(p, h, u) == (hip.CS3_ERR_STATE, "cs3_cplx_updates_solve: no successful factorisation")


# ---- the restatement with an exact Z stays within the bound the GPU is held to --------------------------------------------

def _restated_exact(B, cases, sing_tol=0.0):
    sr, si, solve = cr.exact_inverse_callback(B.A)
    tiles = [(0, len(cases), 0, 0)]
    rows = sorted({int(r) for c in cases for r in c[0]})
    tiles = [(0, len(cases), len(rows), len(rows))]
    return cr.solve_restated(B.n, cases, tiles, B.b, sr, si, solve, sing_tol)


@pytest.mark.parametrize("name", ["ybus40", "ybus40_lossless", "ybus300", "hermitian_pd"])
def test_the_restatement_with_an_exact_inverse_stays_within_the_accuracy_bound(name):
    B, cases = cc.accuracy_lists(name)
    X, rpiv, caps, _ = _restated_exact(B, cases)
    worst, healthy, ranks = 0.0, np.inf, set()
    for c, case in enumerate(cases):
        want, cond1 = cr.x_dense(B.A, case, B.b)
        assert cond1 < 1e5, (name, c, cond1)               # no outage of these networks islands a bus
        ratio = float(np.abs(X[:, c] - want).max()) / cr.accuracy_bound(cond1, want)
        worst, healthy = max(worst, ratio), min(healthy, rpiv[c])
        ranks.add(len(np.unique(case[0])))
    print("%-16s %4d cases  ranks %s  healthy rpiv >= %.2e  worst error / bound %.2e" % (name, len(cases), sorted(ranks), healthy, worst))
    assert worst <= 1.0
    if name.startswith("ybus40"):
        assert len(cc.branches(B.A)) == 60 and {3, 4, 5, 6} & ranks
    if name == "ybus300":
        assert len(cases) == 480


# ---- what each designed case is there for ----------------------------------------------------------------------------------

def test_cdiv_and_cabs1_on_numbers_known_by_hand():
    assert cr.cdiv(1.0, 0.0, 0.0, 2.0) == (0.0, -0.5)                                  # 1 / 2j = -0.5j
    assert cr.cdiv(-1.0, 7.0, 3.0, -4.0) == ((-3.0 - 28.0) / 25.0, (21.0 - 4.0) / 25.0)
    assert cr.cabs1(-0.6, 0.6) == 1.2 and cr.cabs1(np.nan, 0.0) != cr.cabs1(np.nan, 0.0)


def test_designed_cases_deliver_their_pivoting():
    B = cc.base(cc.N_PIVOT)
    designed = cc.pivot_cases()
    cases = [d.case for d in designed]
    X, rpiv, caps, _ = _restated_exact(B, cases)
    seen = {"swaps": 0, "small": 0, "tie": 0, "cabs1": 0, "rect": 0}
    for c, d in enumerate(designed):
        cap = caps[c]
        want, cond1 = cr.x_dense(B.A, d.case, B.b)
        err = float(np.abs(X[:, c] - want).max() / np.abs(want).max())
        r = len(cap.picks)
        swaps = sum(p != k for k, p in enumerate(cap.picks))
        margin = min(cap.margins) if cap.margins else np.inf
        print("%-10s r %2d  swaps %2d  margin %.2e  smallest pivot at step %2d  rpiv %.2e  error %.1e"
              % (d.name, r, swaps, margin, int(np.argmin(cap.pivots)), rpiv[c], err))
        assert err <= 1e-10, d.name
        if not d.tie:
            assert margin >= MARGIN, (d.name, cap.margins)
        if d.swaps is not None:
            assert swaps == r - 1 == d.swaps and all(p != k for k, p in enumerate(cap.picks[:-1])), (d.name, cap.picks)
            assert margin >= 0.1, (d.name, cap.margins)
            seen["swaps"] += 1
        if d.small:
            assert 0 < d.smallest_step < r - 1 and int(np.argmin(cap.pivots)) == d.smallest_step, (d.name, cap.pivots)
            assert 1e-4 <= rpiv[c] <= 1e-2, (d.name, rpiv[c])
            seen["small"] += 1
        if d.tie:
            S0 = cap.Sr[:, 0] + 1j * cap.Si[:, 0]
            assert S0[1] == S0[2] and cr.cabs1(S0[1].real, S0[1].imag) > max(cr.cabs1(S0[k].real, S0[k].imag) for k in (0, 3))
            assert cap.picks[0] == 1 and cap.margins[0] == 0.0 and min(cap.margins[1:]) >= 0.1, (cap.picks, cap.margins)
            seen["tie"] += 1
        if d.name == "cabs1":
            S0 = cap.Sr[:, 0] + 1j * cap.Si[:, 0]
            assert cr.cabs1(S0[1].real, S0[1].imag) > cr.cabs1(S0[0].real, S0[0].imag) and abs(S0[1]) < abs(S0[0])
            assert cap.picks[0] == 1 and abs(rpiv[c] - cc.CABS1_RPIV) <= 1e-9 and abs(rpiv[c] - cc.MODULUS_RPIV) >= 0.05
            seen["cabs1"] += 1
        if d.name.startswith("rect"):
            assert (len(np.unique(d.case[0])), len(np.unique(d.case[1]))) in cc.RECT_SHAPES
            seen["rect"] += 1
    assert seen == {"swaps": len(cc.RANKS) + 4, "small": 4, "tie": 1, "cabs1": 1, "rect": len(cc.RECT_SHAPES)}


def test_the_engineered_matrices_and_the_exact_zero():
    for n in (1, 3, 4, 5, 63, 64, 65, cc.N_PIVOT):
        A = cc.base(n).A
        off = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
        assert np.all(np.abs(np.diag(A)) >= off + 1.0)
        d = np.diag(A)[:4]
        if n >= 4:                                         # the branches of the rotation, in this order
            assert abs(d[0].real) > abs(d[0].imag) and d[0].real > 0 and abs(d[1].imag) > abs(d[1].real)
            assert d[2].real < 0 and d[3].real == d[3].imag
    B = cc.base_exact_zero()
    X, rpiv, caps, _ = _restated_exact(B, [cc.EXACT_ZERO_CASE, cc.EMPTY])
    assert rpiv[0] == 0.0 and caps[0].flag == 1 and np.isnan(X[:, 0]).all() and rpiv[1] == 1.0
    assert np.array_equal(X[:, 1], np.linalg.inv(B.A) @ B.b)
    cases, twin, lanes = cc.flagged_lists()
    X, rpiv, caps, _ = _restated_exact(cc.base(cc.N_PIVOT), cases, 1e-10)
    assert sorted(np.flatnonzero(np.isnan(X).all(axis=0))) == sorted(lanes) and np.all(rpiv[list(lanes)] <= 1e-13)
    assert np.all(np.delete(rpiv, lanes) >= 0.5)
    for lst, bad in cc.nan_lists():
        X, rpiv, caps, _ = _restated_exact(cc.base(cc.N_PIVOT), lst)
        assert np.isnan(rpiv[bad]) and caps[bad].flag == 1 and np.isnan(X[:, bad]).all()
        assert not np.isnan(np.delete(X, bad, axis=1)).any() and not np.isnan(np.delete(rpiv, bad)).any()
