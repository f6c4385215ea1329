"""Sparse right-hand sides (cs3_sens_*), the part that needs no GPU: the plan's argument checks in their documented order,
its info and the limits against the restatement (tests/sens_ref.py), the side choice, the state error of a solve before a
factorisation, and the reference alone -- its two evaluation orders must agree far inside helpers.RTOL before a GPU
result is held against either."""
import ctypes as C

import numpy as np
import pytest

from csparse3_amd import synth
from helpers import RTOL, csc_to_scipy, rel_err
import sens_cases as sc
import sens_ref as sr

SYMBOLS = ("cs3_sens_plan", "cs3_sens_free", "cs3_sens_info", "cs3_sens_limits", "cs3_sens_solve_dev", "cs3_sens_solve")
EDGES = (1, 15, 16, 17, 1023, 1024, 1025)


def test_the_new_symbols_are_exported(hip):
    lib = hip.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libcsparse3_hip.so does not export " + name


def test_limits(hip):
    lim = hip.sens_limits()
    assert lim.max_tile == 1024 and 1 <= lim.pad_width <= lim.max_tile
    assert lim.scatter_rows >= 1 and lim.scatter_threads % 64 == 0
    assert lim.combine_lanes % 64 == 0 and lim.combine_cols >= 1 and lim.tblock >= 1
    assert hip.lib().cs3_sens_limits(None) == hip.CS3_ERR_ARG


# ---- refusals --------------------------------------------------------------------------------------------------------------

def _toy(hip, **kw):
    m, n, Ap, Ai, Ax, b, xt = synth.toy10()
    return n, Ax, hip.Factorization(m, n, Ap, Ai, **kw)


def _plan_rc(hip, h, k, Bp, Bi, p, Ctp, Cti, side=0, trans=0, out=True):
    lib = hip.lib()
    u = C.c_void_p()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    Bp, Bi, Ctp, Cti = arr(Bp), arr(Bi), arr(Ctp), arr(Cti)
    rc = lib.cs3_sens_plan(h, k, hip._pi(Bp), hip._pi(Bi), p, hip._pi(Ctp), hip._pi(Cti), side, trans, C.byref(u) if out else None)
    msg = lib.cs3_last_error().decode()
    if u:
        lib.cs3_sens_free(u)
    return rc, msg


def test_plan_refusals_in_their_documented_order(hip):
    n, Ax, F = _toy(hip)
    B = (2, [0, 1, 3], [4, 0, 9])                    # k, Bp, Bi
    Ct = (3, [0, 2, 2, 3], [1, 2, 7])                # p, Ctp, Cti
    ident = (n, None, None)
    bad_ptr = (2, [0, 2, 1], [4, 0])
    bad_ptr0 = (2, [1, 1, 2], [4, 0])
    bad_idx = (2, [0, 1, 2], [4, n])
    neg_idx = (2, [0, 1, 2], [-1, 4])
    E = hip.CS3_ERR_ARG
    with F:
        h = F._h
        assert _plan_rc(hip, h, *B, *Ct)[0] == 0
        # 1. null handle, null out pointer
        rc, msg = _plan_rc(hip, None, *B, *Ct)
        assert rc == E and "null handle" in msg
        rc, msg = _plan_rc(hip, h, 0, B[1], B[2], *Ct, out=False)              # ... wins over k < 1
        assert rc == E and "null output" in msg
        # 2. k < 1 or p < 1 (before anything is read: the arrays are null here)
        for k, p in ((0, 3), (-1, 3), (2, 0), (2, -5)):
            rc, msg = _plan_rc(hip, h, k, None, None, p, None, None)
            assert rc == E and "k and p" in msg, (k, p, msg)
        # 3. both the identity (wins over 4: k, p != n)
        rc, msg = _plan_rc(hip, h, 3, None, None, 4, None, None)
        assert rc == E and "both the identity" in msg
        # 4. an identity operand with k or p != n (wins over 5: a bad pointer array of the other operand)
        rc, msg = _plan_rc(hip, h, n - 1, None, None, 2, bad_ptr[1], bad_ptr[2])
        assert rc == E and "k != n" in msg
        rc, msg = _plan_rc(hip, h, 2, bad_ptr[1], bad_ptr[2], n + 1, None, None)
        assert rc == E and "p != n" in msg
        # 5. pointers not monotone from 0 (wins over 6: a bad index in B while Ctp is bad)
        rc, msg = _plan_rc(hip, h, *bad_idx, *bad_ptr)
        assert rc == E and "Ctp not monotone" in msg
        rc, msg = _plan_rc(hip, h, *bad_ptr, *Ct)
        assert rc == E and "Bp not monotone" in msg
        rc, msg = _plan_rc(hip, h, *bad_ptr0, *Ct)
        assert rc == E and "Bp[0] != 0" in msg
        rc, msg = _plan_rc(hip, h, *B, *bad_ptr0)
        assert rc == E and "Ctp[0] != 0" in msg
        rc, msg = _plan_rc(hip, h, 2, [0, 1, 2], None, *Ct)
        assert rc == E and "null index array" in msg
        # 6. an index outside [0, n) (wins over 7: a bad side)
        for bad in (bad_idx, neg_idx):
            rc, msg = _plan_rc(hip, h, *bad, *Ct, side=3)
            assert rc == E and "out of range" in msg and " B" in msg
            rc, msg = _plan_rc(hip, h, *B, *bad, side=3)
            assert rc == E and "out of range" in msg and "C'" in msg
        # 7. side outside {0, 1, 2} (wins over 8)
        for side in (-1, 3):
            rc, msg = _plan_rc(hip, h, *ident, *Ct, side=side)
            assert rc == E and "side must be" in msg
        # 8. a side that an identity operand rules out
        rc, msg = _plan_rc(hip, h, *ident, *Ct, side=1)
        assert rc == E and "B is the identity" in msg
        rc, msg = _plan_rc(hip, h, *B, *ident, side=2)
        assert rc == E and "C is the identity" in msg
        assert _plan_rc(hip, h, *ident, *Ct, side=2)[0] == 0 and _plan_rc(hip, h, *B, *ident, side=1)[0] == 0
    # 9. batch > 1 (after 8), 10. a Schur handle (after 9 -- no handle is both -- and after 7)
    n, Ax, F = _toy(hip, batch=2)
    with F:
        rc, msg = _plan_rc(hip, F._h, *B, *Ct)
        assert rc == E and "batch > 1" in msg
        rc, msg = _plan_rc(hip, F._h, *ident, *Ct, side=1)
        assert rc == E and "B is the identity" in msg
    n, Ax, F = _toy(hip, schur=[3, 7])
    with F:
        rc, msg = _plan_rc(hip, F._h, *B, *Ct)
        assert rc == E and "Schur handle" in msg
        rc, msg = _plan_rc(hip, F._h, *B, *Ct, side=5)
        assert rc == E and "side must be" in msg
    n, Ax, F = _toy(hip, schur=[3, 7], batch=2)
    with F:
        rc, msg = _plan_rc(hip, F._h, *B, *Ct)
        assert rc == E and "batch > 1" in msg


# ---- info, tiles, side -----------------------------------------------------------------------------------------------------

def _info_dict(info):
    return {f: int(getattr(info, f)) for f, _ in info._fields_}


@pytest.mark.parametrize("tile", [None, "16", "5", "1000", "4096"])
def test_info_matches_the_restatement_at_the_width_edges(hip, monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    else:
        monkeypatch.setenv("CS3_SENS_TILE", tile)
    lim = hip.sens_limits()
    n, Ax, F = _toy(hip)
    with F:
        for k in EDGES:
            for p in EDGES:
                B, Ct = sc.incidence(n, k, seed=k), sc.incidence(n, p, seed=100 + p)
                for side in ("auto", "right", "left"):
                    for trans in (False, True):
                        with F.sens_plan(B[:3], Ct[:3], side=side, trans=trans) as plan:
                            want = sr.info_ref(n, k, p, int(B.indptr[-1]), int(Ct.indptr[-1]), lim, sr.SIDES[side], trans, tile)
                            assert _info_dict(plan.info) == want, (k, p, side, trans, tile)


def test_side_choice_tie_and_identity_operands(hip, monkeypatch):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    lim = hip.sens_limits()
    n, Ax, F = _toy(hip)
    with F:
        op = lambda c: sc.incidence(n, c, seed=c)[:3]                          # noqa: E731
        side = lambda *a, **kw: F.sens_plan(*a, **kw).info.side                # noqa: E731
        assert side(op(7), op(7)) == sr.RIGHT                                  # a tie goes right
        assert side(op(8), op(7)) == sr.LEFT and side(op(7), op(8)) == sr.RIGHT
        assert side(op(8), op(7), side="right") == sr.RIGHT and side(op(7), op(8), side="left") == sr.LEFT
        assert side(None, op(3)) == sr.LEFT and side(None, op(3), side="left") == sr.LEFT
        assert side(None, op(50)) == sr.LEFT                                   # even with more rows than n
        assert side(op(3), None) == sr.RIGHT and side(op(50), None, side="right") == sr.RIGHT
        with F.sens_plan(None, op(3)) as plan:
            assert _info_dict(plan.info) == sr.info_ref(n, n, 3, None, int(op(3)[1][-1]), lim)
        with F.sens_plan(op(4), None, trans=True) as plan:
            assert _info_dict(plan.info) == sr.info_ref(n, 4, n, int(op(4)[1][-1]), None, lim, trans=True)


def test_restatement_keeps_two_widths_and_covers_every_column(hip):
    lim = hip.sens_limits()
    for tile in (None, 1, 5, 16, 17, 1000):
        for ns in (1, 4, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2048, 2049, 8192):
            tl = sr.tiles(ns, lim, tile)
            assert [c0 for c0, _, _ in tl] == list(np.cumsum([0] + [t for _, t, _ in tl[:-1]]))
            assert sum(t for _, t, _ in tl) == ns and all(t <= w <= lim.max_tile for _, t, w in tl)
            assert len({w for _, _, w in tl}) <= 2


# ---- state and lifetime ----------------------------------------------------------------------------------------------------

def test_solve_before_a_factorisation_is_a_state_error(hip):
    n, Ax, F = _toy(hip)
    B, Ct = sc.incidence(n, 3, seed=1), sc.incidence(n, 2, seed=2)
    with F, F.sens_plan(B[:3], Ct[:3]) as plan:
        with pytest.raises(hip.Cs3Error) as e:
            F.sens_solve(plan, B.values, Ct.values)
        assert e.value.code == hip.CS3_ERR_STATE
        with pytest.raises(hip.Cs3Error) as e:
            F.sens_solve_dev(plan, 8, 8, 8)
        assert e.value.code == hip.CS3_ERR_STATE
        for args in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):                         # null arguments come first
            with pytest.raises(hip.Cs3Error) as e:
                F.sens_solve_dev(plan, *args)
            assert e.value.code == hip.CS3_ERR_ARG
        with F.sens_plan(None, Ct[:3]) as ident:                               # the value pointer of an identity operand is ignored
            with pytest.raises(hip.Cs3Error) as e:
                F.sens_solve_dev(ident, 0, 8, 8)
            assert e.value.code == hip.CS3_ERR_STATE
        n2, Ax2, G = _toy(hip)
        with G:
            with pytest.raises(hip.Cs3Error) as e:                             # another handle's plan
                G.sens_solve_dev(plan, 8, 8, 8)
            assert e.value.code == hip.CS3_ERR_ARG and "another handle" in str(e.value)


def test_plan_and_handle_may_be_freed_in_either_order(hip):
    n, Ax, F = _toy(hip)
    B = sc.incidence(n, 3, seed=1)
    plan = F.sens_plan(B[:3], None)
    F.close()
    assert plan.info.k == 3
    plan.close()
    n, Ax, F = _toy(hip)
    plan = F.sens_plan(B[:3], None)
    plan.close()
    F.close()


# ---- the reference alone ---------------------------------------------------------------------------------------------------

def _spd4000():
    ei, ej = synth.spd_grid_pattern(4000, seed=4000)
    return synth.spd_grid_matrix(4000, ei, ej, seed=4001)


REFERENCE_MATRICES = {
    "toy10": lambda: synth.toy10()[:5],
    "jacobian_like": synth.jacobian_like,
    "grid5000": lambda: synth.grid_jacobian(5000),
    "grid20000": lambda: synth.grid_jacobian(20000),
    "spd4000": _spd4000,
    "spd900": lambda: sc.matrix("spd900")[:5],
    "kkt400": lambda: sc.matrix("kkt400")[:5],
}


@pytest.mark.parametrize("name", list(REFERENCE_MATRICES))
def test_the_two_evaluation_orders_of_the_reference_agree(name):
    """C (A^-1 B) against ((A^-T C')' B) with +-v incidence columns for B and C', plain and transposed: two different
    factorisations and two different orders of summation, so their distance bounds the error of either."""
    m, n, Ap, Ai, Ax = REFERENCE_MATRICES[name]()
    A = csc_to_scipy(m, n, Ap, Ai[:Ap[n]], Ax[:Ap[n]]).tocsc()
    B, Ct = sc.incidence(n, 40, seed=11), sc.incidence(n, 24, seed=13)
    for trans in (False, True):
        yr, yl = sr.y_right(A, B, Ct, trans), sr.y_left(A, B, Ct, trans)
        err = rel_err(yl, yr)
        print("%s trans=%s: right against left %.2e" % (name, trans, err))
        assert yr.shape == (24, 40) and err <= RTOL


def test_reference_adds_duplicates_and_takes_identity_operands():
    m, n, Ap, Ai, Ax = synth.jacobian_like()
    A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()
    dup = sc.from_columns([([5, 9, 5, 5], [0.25, 1.0, 0.5, -0.125]), ([], []), ([3], [2.0])])
    merged = sc.from_columns([([5, 9], [0.625, 1.0]), ([], []), ([3], [2.0])])
    Ct = sc.selection([7, 0, 150])
    assert np.array_equal(sr.y_right(A, dup, Ct), sr.y_right(A, merged, Ct))
    assert not sr.y_right(A, dup, Ct)[:, 1].any()
    inv = np.linalg.inv(A.toarray())
    assert rel_err(sr.y_left(A, None, Ct), inv[[7, 0, 150], :]) <= RTOL
    assert rel_err(sr.y_right(A, dup, None), inv @ sr.dense(dup, n)) <= RTOL
