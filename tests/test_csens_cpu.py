"""Complex sparse right-hand sides (cs3_cplx_sens_*) and complex Schur plans (cs3_cplx_plan_create_schur), the part that
needs no GPU: every plan check in its documented order, the side rule, tiles and info against sens_ref, the p-not-2p
promise of side left, the border of a Schur plan (never rotated, counted, ordered as cs3_analyze_schur orders), the
restatement (tests/csens_ref.py) against dense NumPy -- so that what the GPU tests compare with bit for bit is itself
right --, and that the ctypes mirrors kept their sizes."""
import ctypes as C

import numpy as np
import pytest

import cplx_ref as ref
import csens_cases as cc
import csens_ref as cr
import sens_ref as sr

SYMBOLS = ("cs3_cplx_sens_limits", "cs3_cplx_sens_plan", "cs3_cplx_sens_free", "cs3_cplx_sens_info", "cs3_cplx_sens_solve_dev",
           "cs3_cplx_sens_solve", "cs3_debug_cplx_sens_parts", "cs3_cplx_plan_create_schur", "cs3_cplx_plan_schur_info",
           "cs3_cplx_plan_schur_order", "cs3_cplx_schur_get_dev", "cs3_cplx_schur_get")
OPS = {"N": ref.N, "T": ref.T, "H": ref.H}


def test_the_new_symbols_are_exported(hip):
    for name in SYMBOLS:
        assert hasattr(hip.lib(), name), "libcsparse3_hip.so does not export " + name


def test_limits_and_the_mirrors_kept_their_sizes(hip):
    lim, real = hip.cplx_sens_limits(), hip.sens_limits()
    assert (lim.max_tile, lim.pad_width, lim.scatter_threads, lim.combine_cols, lim.combine_lanes, lim.tblock) == \
        (real.max_tile, real.pad_width, real.scatter_threads, real.combine_cols, real.combine_lanes, real.tblock)
    assert lim.scatter_rows == real.scatter_rows and lim.scatter_rows % 2 == 0       # real rows of the tile: whole pairs
    assert hip.lib().cs3_cplx_sens_limits(None) == hip.CS3_ERR_ARG
    assert C.sizeof(hip.CplxInfo) == 7 * 8 and C.sizeof(hip.SensInfo) == 8 * 8 and C.sizeof(hip.SensLimits) == 7 * 8
    n, Ap, Ai, _ = cc.ybus40()
    with hip.ComplexPlan(n, Ap, Ai) as plan:                                         # a guard behind the struct stays
        buf = (C.c_int64 * 8)(*([-7] * 8))
        assert hip.lib().cs3_cplx_plan_info(plan._p, C.cast(buf, C.POINTER(hip.CplxInfo))) == 0
        assert buf[7] == -7 and buf[0] == n


# ---- refusals ------------------------------------------------------------------------------------------------------------

def _plan_rc(hip, p, h, k, Bp, Bi, pr, Ctp, Cti, side=0, op=0, out=True):
    lib = hip.lib()
    u = C.c_void_p()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    Bp, Bi, Ctp, Cti = arr(Bp), arr(Bi), arr(Ctp), arr(Cti)
    rc = lib.cs3_cplx_sens_plan(p, h, k, hip._pi(Bp), hip._pi(Bi), pr, hip._pi(Ctp), hip._pi(Cti), side, op, C.byref(u) if out else None)
    msg = lib.cs3_last_error().decode()
    if u:
        lib.cs3_cplx_sens_free(u)
    return rc, msg


def test_plan_refusals_in_their_documented_order(hip):
    n, Ap, Ai, _ = cc.ybus40()
    B = (2, [0, 1, 3], [4, 0, 9])
    Ct = (3, [0, 2, 2, 3], [1, 2, 7])
    ident = (n, None, None)
    bad_ptr = (2, [0, 2, 1], [4, 0])
    bad_ptr0 = (2, [1, 1, 2], [4, 0])
    bad_idx = (2, [0, 1, 2], [4, n])                 # n is a valid row of the handle (order 2n), not of the complex matrix
    neg_idx = (2, [0, 1, 2], [-1, 4])
    E = hip.CS3_ERR_ARG
    with hip.ComplexFactorization(n, Ap, Ai) as F, hip.ComplexFactorization(n, Ap, Ai, batch=2) as F2, \
            hip.ComplexFactorization(n, Ap, Ai, schur=cc.BORDER) as FS, hip.Factorization(n, n, Ap, Ai) as R:
        p, h = F.plan._p, F.real._h
        assert _plan_rc(hip, p, h, *B, *Ct)[0] == 0
        # the checks in front of those of cs3_sens_plan: each call is wrong in everything that comes later as well
        for pp, hh in ((None, h), (p, None)):
            rc, msg = _plan_rc(hip, pp, hh, 0, None, None, 0, None, None, side=9, op=9)
            assert rc == E and "null plan or handle" in msg
        rc, msg = _plan_rc(hip, p, R._h, 0, None, None, 0, None, None, out=False)
        assert rc == E and "null output" in msg
        rc, msg = _plan_rc(hip, p, R._h, 0, None, None, 0, None, None, side=9)
        assert rc == E and "not 2 n" in msg
        rc, msg = _plan_rc(hip, F2.plan._p, F2.real._h, 0, None, None, 0, None, None)
        assert rc == E and "batch > 1" in msg
        rc, msg = _plan_rc(hip, FS.plan._p, FS.real._h, 0, None, None, 0, None, None)
        assert rc == E and "Schur handle" in msg
        # ... then cs3_sens_plan's, in its order and wording
        for k, pr in ((0, 3), (-1, 3), (2, 0), (2, -5)):
            rc, msg = _plan_rc(hip, p, h, k, None, None, pr, None, None)
            assert rc == E and "k and p must be >= 1" in msg
        rc, msg = _plan_rc(hip, p, h, 3, None, None, 4, None, None)
        assert rc == E and "both the identity" in msg
        rc, msg = _plan_rc(hip, p, h, n - 1, None, None, 2, bad_ptr[1], bad_ptr[2])
        assert rc == E and "k != n" in msg
        rc, msg = _plan_rc(hip, p, h, 2, bad_ptr[1], bad_ptr[2], n + 1, None, None)
        assert rc == E and "p != n" in msg
        rc, msg = _plan_rc(hip, p, h, 2 * n, None, None, *Ct)                          # the identity has the COMPLEX order
        assert rc == E and "k != n" in msg
        rc, msg = _plan_rc(hip, p, h, *bad_idx, *bad_ptr)
        assert rc == E and "Ctp not monotone at column 1" in msg
        rc, msg = _plan_rc(hip, p, h, *bad_ptr, *Ct)
        assert rc == E and "Bp not monotone at column 1" in msg
        rc, msg = _plan_rc(hip, p, h, *bad_ptr0, *Ct)
        assert rc == E and "Bp[0] != 0" in msg
        rc, msg = _plan_rc(hip, p, h, *B, *bad_ptr0)
        assert rc == E and "Ctp[0] != 0" in msg
        rc, msg = _plan_rc(hip, p, h, 2, [0, 1, 2], None, *Ct)
        assert rc == E and "null index array behind Bp" in msg
        for bad in (bad_idx, neg_idx):
            rc, msg = _plan_rc(hip, p, h, *bad, *Ct, side=3)
            assert rc == E and "index out of range in column" in msg and " of B" in msg
            rc, msg = _plan_rc(hip, p, h, *B, *bad, side=3)
            assert rc == E and "index out of range in column" in msg and "C'" in msg
        for side in (-1, 3):
            rc, msg = _plan_rc(hip, p, h, *ident, *Ct, side=side, op=7)
            assert rc == E and "side must be 0 (auto), 1 (right) or 2 (left)" in msg
        rc, msg = _plan_rc(hip, p, h, *ident, *Ct, side=1, op=7)
        assert rc == E and "B is the identity, side right" in msg
        rc, msg = _plan_rc(hip, p, h, *B, *ident, side=2, op=7)
        assert rc == E and "C is the identity, side left" in msg
        for op in (-1, 3):
            rc, msg = _plan_rc(hip, p, h, *B, *Ct, op=op)
            assert rc == E and "op must be" in msg
        assert all(msg.startswith("cs3_cplx_sens_plan: ") for msg in (_plan_rc(hip, p, h, *bad_ptr, *Ct)[1], _plan_rc(hip, p, h, *B, *Ct, op=3)[1]))
        # a solve before a factorisation: a state error, after the argument checks
        with F.sens_plan(B, Ct) as plan:
            with pytest.raises(hip.Cs3Error) as e:
                F.sens_solve(plan, np.ones(3), np.ones(3))
            assert e.value.code == hip.CS3_ERR_STATE
            with pytest.raises(hip.Cs3Error) as e:                                     # a plan of another handle
                F2.sens_solve(plan, np.ones(3), np.ones(3))
            assert e.value.code == E and "another handle" in str(e.value)


def test_either_party_may_be_freed_first(hip):
    n, Ap, Ai, _ = cc.ybus40()
    F = hip.ComplexFactorization(n, Ap, Ai)
    plan = F.sens_plan((2, [0, 1, 3], [4, 0, 9]), (3, [0, 2, 2, 3], [1, 2, 7]))
    F.close()
    assert plan.info.k == 2                           # the plan outlives its handle: it can be asked, and freed
    plan.close()
    with hip.ComplexFactorization(n, Ap, Ai) as G:
        G.sens_plan((2, [0, 1, 3], [4, 0, 9])).close()


# ---- side, tiles, info -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_env", [None, "5", "16", "4000"])
def test_side_rule_tiles_and_info(hip, monkeypatch, tile_env):
    if tile_env is None:
        monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    else:
        monkeypatch.setenv("CS3_SENS_TILE", tile_env)
    n, Ap, Ai, _ = cc.ybus40()
    lim = hip.cplx_sens_limits()
    with hip.ComplexFactorization(n, Ap, Ai) as F:
        for k, p in ((1, 1), (7, 7), (15, 40), (40, 15), (17, 16), (16, 17), (1030, 33), (33, 1030)):
            B, Ct = cc.incidence(n, k, 1), cc.incidence(n, p, 2)
            for side in ("auto", "right", "left"):
                for name, op in OPS.items():
                    with F.sens_plan((k, B.indptr, B.indices), (p, Ct.indptr, Ct.indices), side=side, trans=name) as plan:
                        inf = plan.info
                        want = sr.info_ref(n, k, p, len(B.indices), len(Ct.indices), lim, sr.SIDES[side], False, tile_env)
                        want["trans"] = op                                           # .trans holds the cs3_cplx_op
                        assert {f: getattr(inf, f) for f in want} == want, (k, p, side, name)
        for B, Ct, side in ((None, cc.incidence(n, 9, 3), "auto"), (cc.incidence(n, 9, 3), None, "auto"), (None, cc.incidence(n, 9, 3), "left")):
            args = [None if o is None else (o.ncols, o.indptr, o.indices) for o in (B, Ct)]
            with F.sens_plan(*args, side=side) as plan:
                inf = plan.info
                want = sr.info_ref(n, n if B is None else 9, n if Ct is None else 9, None if B is None else len(B.indices),
                                   None if Ct is None else len(Ct.indices), lim, sr.SIDES[side], False, tile_env)
                assert {f: getattr(inf, f) for f in want} == want


def test_side_left_plans_p_solved_for_columns_not_2p(hip, monkeypatch):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    n, Ap, Ai, _ = cc.ybus40()
    k, p = 200, 24
    B, Ct = cc.incidence(n, k, 1), cc.incidence(n, p, 2)
    with hip.ComplexFactorization(n, Ap, Ai) as F, F.sens_plan((k, B.indptr, B.indices), (p, Ct.indptr, Ct.indices)) as plan:
        inf = plan.info
        assert (inf.side, inf.ntiles, inf.max_width) == (sr.LEFT, 1, p)             # p real columns of the [2n, w] tile
        # the real path on the real form needs the real and the imaginary row of every row of C: 2p unit rows stand for them
        with F.real.sens_plan((2 * k, np.arange(2 * k + 1), np.arange(2 * k) % (2 * n)),
                              (2 * p, np.arange(2 * p + 1), np.arange(2 * p) % (2 * n))) as real_plan:
            assert (real_plan.info.side, real_plan.info.max_width) == (sr.LEFT, 2 * p)


# ---- plans with a border ---------------------------------------------------------------------------------------------------

def _schur_rc(hip, n, Ap, Ai, ns, idx, batch=1, rotate=1, out=True):
    p = C.c_void_p()
    L = hip.lib()
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    rc = L.cs3_cplx_plan_create_schur(n, hip._pi(Ap), hip._pi(Ai), batch, rotate, ns, hip._pi(idx), C.byref(p) if out else None)
    msg = L.cs3_last_error().decode() if rc else ""
    if p:
        L.cs3_cplx_plan_free(p)
    return rc, msg


def test_create_schur_checks_in_their_order(hip):
    n, Ap, Ai, _ = cc.ybus40()
    E = hip.CS3_ERR_ARG
    assert _schur_rc(hip, n, Ap, Ai, 5, cc.BORDER) == (0, "")
    # the checks of cs3_cplx_plan_create come first, in their order, whatever the set
    rc, msg = _schur_rc(hip, n, Ap, Ai, 0, None, batch=0, out=False)
    assert rc == E and "null output" in msg
    rc, msg = _schur_rc(hip, n, Ap, Ai, 0, None, batch=0, rotate=5)
    assert rc == E and "batch" in msg
    rc, msg = _schur_rc(hip, n, Ap, Ai, 0, None, rotate=5)
    assert rc == E and "rotate" in msg
    rc, msg = _schur_rc(hip, n, Ap, np.full_like(Ai, n), 0, None)
    assert rc == E and "out of range at entry 0" in msg
    # then those of cs3_analyze_schur on the set
    rc, msg = _schur_rc(hip, n, Ap, Ai, 0, None)
    assert rc == E and "null Schur index list" in msg
    for ns in (0, -1, n, n + 1):
        rc, msg = _schur_rc(hip, n, Ap, Ai, ns, [n, n])
        assert rc == E and "at least 1 and fewer than n" in msg and "ns = %d" % ns in msg
    rc, msg = _schur_rc(hip, n, Ap, Ai, 3, [3, n, 3])
    assert rc == E and "Schur index %d (entry 1) is outside" % n in msg
    rc, msg = _schur_rc(hip, n, Ap, Ai, 3, [3, -1, 3])
    assert rc == E and "Schur index -1 (entry 1) is outside" in msg
    rc, msg = _schur_rc(hip, n, Ap, Ai, 4, [3, 7, 5, 7])
    assert rc == E and "Schur index 7 (entry 3) is repeated" in msg
    with hip.ComplexPlan(n, Ap, Ai) as plain:
        for call in (plain.schur_info, plain.schur_order):
            with pytest.raises(hip.Cs3Error) as e:
                call()
            assert e.value.code == hip.CS3_ERR_STATE and "no border" in str(e.value)


@pytest.mark.parametrize("border", [cc.BORDER, [17], list(range(39)), [9, 2, 30, 1]], ids=["five", "one", "n_minus_1", "unsorted"])
def test_the_border_is_never_rotated_and_the_order_is_the_restated_one(hip, border):
    n, Ap, Ai, Az = cc.ybus40()
    with hip.ComplexPlan(n, Ap, Ai, schur=border) as plan, hip.ComplexPlan(n, Ap, Ai) as plain:
        assert np.array_equal(plan.schur_info(), border) and plan.ns == len(border)
        assert plan.info.rows_without_diagonal == plain.info.rows_without_diagonal + len(border)     # (every bus has a diagonal)
        assert C.sizeof(plan.info) == 7 * 8
        interior, A11p, A11i = cr.interior_pattern(n, Ap, Ai, border)
        n1 = len(interior)
        amd = interior[hip.csc_amd_f(hip.ORDER_AMD, n1, n1, A11p, A11i)]
        rev = interior[::-1]
        for got, q in ((plan.schur_order(hip.ORDER_AMD), amd), (plan.schur_order(hip.ORDER_NATURAL), interior),
                       (plan.schur_order(q=rev), rev)):
            want = cr.schur_order(border, q)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for bad in (np.r_[interior[:-1], border[0]], np.r_[interior[:-1], interior[0]])[:2 if n1 > 1 else 1]:
            with pytest.raises(hip.Cs3Error) as e:
                plan.schur_order(q=bad)
            assert e.value.code == hip.CS3_ERR_ARG and "permutation of the interior" in str(e.value)
        # the real Schur handle takes both arrays unchanged
        q2, s2 = plan.schur_order()
        Rp, Ri = plan.pattern()
        with hip.Factorization(2 * n, 2 * n, Rp, Ri, q=q2, schur=s2) as R:
            o = R.ordering()["q_amd"]
            assert np.array_equal(o[:2 * n1], q2) and np.array_equal(o[2 * n1:], s2) and np.array_equal(R.schur_info(), s2)
    # the restated rotation: (1, +0) on the border, cplx_ref's elsewhere
    Azr, Azi = ref.split(Az, (1, -1))
    sr_, si_ = cr.rotation_with_border(n, Ap, Ai, Azr, Azi, True, border)
    full = ref.rotation(n, Ap, Ai, Azr, Azi, True)
    assert np.all(sr_[0, border] == 1.0) and not np.signbit(si_[0, border]).any() and not si_[0, border].any()
    interior = np.setdiff1d(np.arange(n), border)
    assert np.array_equal(sr_[0, interior], full[0][0, interior]) and np.array_equal(si_[0, interior], full[1][0, interior])
    assert np.abs(si_[0, interior]).min() > 0.5                                       # (the rotation does turn the other rows)


def test_the_schur_complement_of_the_rotated_real_form_is_that_of_a(hip):
    """The reason the border stays unrotated: S read from the first column of the 2 x 2 blocks of the real Schur complement
    of diag(s) A, s = 1 on the border, is A22 - A21 A11^-1 A12 with no division."""
    n, Ap, Ai, Az = cc.ybus40()
    border = np.array(cc.BORDER)
    Azr, Azi = ref.split(Az, (1, -1))
    sr_, si_ = cr.rotation_with_border(n, Ap, Ai, Azr, Azi, True, border)
    M = ref.dense_real(n, Ap, Ai, ref.values(n, Ap, Ai, Azr, Azi, sr_, si_)[0])
    interior = np.setdiff1d(np.arange(n), border)
    i2, b2 = ref.doubled_order(interior), ref.doubled_order(border)
    SR = M[np.ix_(b2, b2)] - M[np.ix_(b2, i2)] @ np.linalg.solve(M[np.ix_(i2, i2)], M[np.ix_(i2, b2)])
    S, bound, cond = cr.schur_dense(ref.dense_complex(n, Ap, Ai, Az), border)
    got = SR[0::2, 0::2] + 1j * SR[1::2, 0::2]
    twin = SR[1::2, 1::2] - 1j * SR[0::2, 1::2]
    tol = 1e3 * cond * 2.0 ** -53 * bound
    assert np.all(np.abs(got - S) <= tol) and np.all(np.abs(twin - S) <= tol)


# ---- the restatement against the definition --------------------------------------------------------------------------------

def _operands(n, k, p):
    return cc.incidence(n, k, 5), cc.incidence(n, p, 6)


@pytest.mark.parametrize("name", ["ybus40", "unsorted", "hermitian_pd"])
@pytest.mark.parametrize("side", [sr.RIGHT, sr.LEFT], ids=["right", "left"])
@pytest.mark.parametrize("opname", ["N", "T", "H"])
def test_the_restatement_computes_what_dense_numpy_does(hip, name, side, opname):
    n, Ap, Ai, Az, _, rotate = cc.matrices()[name]
    op = OPS[opname]
    A = ref.dense_complex(n, Ap, Ai, Az)
    sr_, si_, solve = cr.dense_solve_callback(n, Ap, Ai, Az, rotate)
    lim = hip.cplx_sens_limits()
    B, Ct = _operands(n, 9, 7)
    for Bo, Co in ((B, Ct), (cc.awkward(n, 3), cc.selection([n - 1, 0, n - 1])), (None, Ct), (B, None)):
        s = side
        if Bo is None or Co is None:
            s = sr.choose_side(0, 0, 0, Bo is None, Co is None)                       # an identity operand forces the other side
        ns = (n if Bo is None else Bo.ncols) if s == sr.RIGHT else (n if Co is None else Co.ncols)
        for tile_env in (None, 4):
            Y, _ = cr.y_restated(n, Bo, Co, s, op, sr_, si_, sr.tiles(ns, lim, tile_env), solve)
            want = cr.y_dense(A, Bo, Co, op)
            assert Y.shape == want.shape
            assert np.abs(Y - want).max() <= 1e-11 * max(np.abs(want).max(), 1e-300), (name, s, opname, tile_env)


def test_scatter_of_an_operand_without_duplicates_is_pack_of_its_dense_form(hip):
    n, Ap, Ai, Az = cc.ybus40()
    sr_, si_, _ = cr.dense_solve_callback(n, Ap, Ai, Az, True)
    B = cc.incidence(n, 11, 7)
    D = cr.dense_op(B, n)
    for inner in (ref.N, ref.T, ref.H):
        for conj in (False, True):
            Dr, Di = ref.split(np.conj(D) if conj else D, (1, n, -1))
            want = ref.pack(inner, Dr, Di, sr_[None], si_[None])[0]
            got = cr.scatter(n, 16, B, 0, 11, inner, conj, sr_, si_)
            assert np.array_equal(got[:, :11], want) and not got[:, 11:].any()        # (values: -0 + 0 = +0 in the tile, == holds)
