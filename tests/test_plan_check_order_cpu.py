"""The four plan calls on held factors -- cs3_sens_plan, cs3_cplx_sens_plan, cs3_updates_plan, cs3_cplx_updates_plan --
refuse bad arguments in the order include/csparse3_amd.h documents.  Each input below violates two checks that are
neighbours in that order (the label names them), and the call must report the EARLIER one: the error code, a distinctive
piece of its message and the `cs3_..._plan: ` prefix (a null handle of the real calls is the one message without a prefix).
Where two neighbours cannot be violated together without tripping a check in front of both (an identity B with k != n and
an identity C with p != n make both operands the identity; a null index array has no index to be out of range in the same
array), the earlier one is paired with the next check it can meet.  Plan calls are host-only: no GPU.

The patterns have order 6; the pairs around "a case with more than 16 distinct rows" need 17 rows to exist and use order 18,
the smallest that has them."""
import ctypes as C

import numpy as np
import pytest

import csens_cases as cc

N, NBIG = 6, 18
SCHUR = [1, 4]

# operands of the sens plans (ncols, indptr, indices), good and bad in one way each
B = (2, [0, 1, 3], [4, 0, 5])
CT = (3, [0, 2, 2, 3], [1, 2, 3])
IDENT = (N, None, None)
B_PTR = (2, [0, 2, 1], [4, 0])                       # not monotone at column 1
CT_PTR = (3, [0, 2, 1, 3], [1, 2, 3])
B_IDX = (2, [0, 1, 2], [4, N])                       # N: a row of the real form of the complex matrix, not of the matrix
CT_IDX = (3, [0, 1, 2, 3], [1, -1, 3])

# case lists of the updates plans (ncases, cp, ci, cj)
CASES = (2, [0, 2, 3], [0, 5, 3], [0, 5, 2])
ROWS17 = list(range(17))
WIDE = (2, [0, 17, 18], ROWS17 + [3], [0] * 17 + [2])                       # case 0 touches 17 rows
WIDE_AND_RANGE = (2, [0, 17, 18], ROWS17 + [NBIG], [0] * 17 + [2])          # ... and case 1 has an index out of range


def _arr(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _sens(hip, h, B=B, Ct=CT, side=0, trans=0, out=True, p=None, k=None, pr=None):
    """cs3_sens_plan, or with a complex plan `p` cs3_cplx_sens_plan (trans is then op) -> (status, message)."""
    lib = hip.lib()
    u = C.c_void_p()
    Bp, Bi, Ctp, Cti = _arr(B[1]), _arr(B[2]), _arr(Ct[1]), _arr(Ct[2])
    args = (h, B[0] if k is None else k, hip._pi(Bp), hip._pi(Bi), Ct[0] if pr is None else pr, hip._pi(Ctp), hip._pi(Cti),
            side, trans, C.byref(u) if out else None)
    rc = lib.cs3_sens_plan(*args) if p is None else lib.cs3_cplx_sens_plan(p[0], *args)
    msg = lib.cs3_last_error().decode()
    if u:
        (lib.cs3_sens_free if p is None else lib.cs3_cplx_sens_free)(u)
    return rc, msg


def _updates(hip, h, cases=CASES, out=True, p=None, ncases=None):
    """cs3_updates_plan, or with a complex plan `p` cs3_cplx_updates_plan -> (status, message)."""
    lib = hip.lib()
    u = C.c_void_p()
    cp, ci, cj = _arr(cases[1]), _arr(cases[2]), _arr(cases[3])
    args = (h, cases[0] if ncases is None else ncases, hip._pi(cp), hip._pi(ci), hip._pi(cj), C.byref(u) if out else None)
    rc = lib.cs3_updates_plan(*args) if p is None else lib.cs3_cplx_updates_plan(p[0], *args)
    msg = lib.cs3_last_error().decode()
    if u:
        (lib.cs3_updates_free if p is None else lib.cs3_cplx_updates_free)(u)
    return rc, msg


def _walk(hip, who, pairs, prefixed=True):
    for label, (rc, msg), want in pairs:
        assert rc == hip.CS3_ERR_ARG and want in msg, (who, label, rc, msg)
        if prefixed and want != "null handle":
            assert msg.startswith(who + ": "), (who, label, msg)


@pytest.fixture(scope="module")
def real(hip):
    """Handles of order 6: plain, batch 2, Schur, Schur with batch 2; of order 18: plain, batch 2."""
    n, Ap, Ai, _ = cc.banded(N, 1)
    nb, Bp, Bi, _ = cc.banded(NBIG, 2)
    H = {"h": hip.Factorization(n, n, Ap, Ai), "h2": hip.Factorization(n, n, Ap, Ai, batch=2),
         "hs": hip.Factorization(n, n, Ap, Ai, schur=SCHUR), "hs2": hip.Factorization(n, n, Ap, Ai, batch=2, schur=SCHUR),
         "big": hip.Factorization(nb, nb, Bp, Bi), "big2": hip.Factorization(nb, nb, Bp, Bi, batch=2)}
    yield {k: v._h for k, v in H.items()}
    for v in H.values():
        v.close()


@pytest.fixture(scope="module")
def cplx(hip):
    """Complex factorisations (a plan .plan._p and its real-form handle .real._h) of order 6: plain, batch 2, with a border,
    with a border and batch 2; of order 18: plain, batch 2, with a border, with a border and batch 2."""
    n, Ap, Ai, _ = cc.banded(N, 1)
    nb, Bp, Bi, _ = cc.banded(NBIG, 2)
    F = {"f": hip.ComplexFactorization(n, Ap, Ai), "f2": hip.ComplexFactorization(n, Ap, Ai, batch=2),
         "fs": hip.ComplexFactorization(n, Ap, Ai, schur=SCHUR), "fs2": hip.ComplexFactorization(n, Ap, Ai, batch=2, schur=SCHUR),
         "big": hip.ComplexFactorization(nb, Bp, Bi), "big2": hip.ComplexFactorization(nb, Bp, Bi, batch=2),
         "bigs": hip.ComplexFactorization(nb, Bp, Bi, schur=SCHUR), "bigs2": hip.ComplexFactorization(nb, Bp, Bi, batch=2, schur=SCHUR)}
    yield F
    for v in F.values():
        v.close()


def test_the_fixtures_plan_when_nothing_is_wrong(hip, real, cplx):
    f, big = cplx["f"], cplx["big"]
    assert _sens(hip, real["h"])[0] == 0 and _updates(hip, real["h"])[0] == 0
    assert _sens(hip, f.real._h, p=(f.plan._p,))[0] == 0 and _updates(hip, f.real._h, p=(f.plan._p,))[0] == 0
    assert _updates(hip, real["big"])[0] == 0 and _updates(hip, big.real._h, p=(big.plan._p,))[0] == 0


def test_cs3_sens_plan(hip, real):
    h, h2, hs, hs2 = real["h"], real["h2"], real["hs"], real["hs2"]
    _walk(hip, "cs3_sens_plan", [
        ("null handle / null output", _sens(hip, None, out=False), "null handle"),
        ("null output / k < 1", _sens(hip, h, k=0, out=False), "null output"),
        ("k < 1 / both the identity", _sens(hip, h, IDENT, IDENT, k=0), "k and p must be >= 1"),
        ("p < 1 / both the identity", _sens(hip, h, IDENT, IDENT, pr=-2), "k and p must be >= 1"),
        ("both the identity / B = I with k != n", _sens(hip, h, IDENT, IDENT, k=3, pr=3), "both the identity"),
        ("B = I with k != n / Ctp not monotone", _sens(hip, h, IDENT, CT_PTR, k=3), "B is the identity but k != n"),
        ("C = I with p != n / Bp not monotone", _sens(hip, h, B_PTR, IDENT, pr=3), "C is the identity but p != n"),
        ("Bp not monotone / Ctp not monotone", _sens(hip, h, B_PTR, CT_PTR), "Bp not monotone at column 1"),
        ("Ctp not monotone / an index of B out of range", _sens(hip, h, B_IDX, CT_PTR), "Ctp not monotone at column 1"),
        ("an index of B / an index of C'", _sens(hip, h, B_IDX, CT_IDX), "index out of range in column 1 of B"),
        ("an index of C' / side outside 0 .. 2", _sens(hip, h, B, CT_IDX, side=3), "index out of range in column 1 of C'"),
        ("side outside 0 .. 2 / batch > 1", _sens(hip, h2, side=3), "side must be 0 (auto), 1 (right) or 2 (left)"),
        ("side outside 0 .. 2 / a Schur handle", _sens(hip, hs, side=-1), "side must be 0 (auto), 1 (right) or 2 (left)"),
        ("B = I with side right / batch > 1", _sens(hip, h2, IDENT, CT, side=1), "B is the identity, side right"),
        ("C = I with side left / batch > 1", _sens(hip, h2, B, IDENT, side=2), "C is the identity, side left"),
        ("batch > 1 / a Schur handle", _sens(hip, hs2), "handles with batch > 1 are not supported"),
        ("a Schur handle, last", _sens(hip, hs), "not available on a Schur handle (cs3_analyze_schur)"),
    ])


def test_cs3_cplx_sens_plan(hip, real, cplx):
    f, f2, fs, fs2 = cplx["f"], cplx["f2"], cplx["fs"], cplx["fs2"]
    p, h = (f.plan._p,), f.real._h
    _walk(hip, "cs3_cplx_sens_plan", [
        ("null plan / null output", _sens(hip, h, p=(None,), out=False), "null plan or handle"),
        ("null handle / null output", _sens(hip, None, p=p, out=False), "null plan or handle"),
        ("null output / the order is not 2 n", _sens(hip, real["h"], p=p, out=False), "null output"),
        ("the order is not 2 n / batch > 1", _sens(hip, real["h2"], p=p), "not 2 n of the complex plan"),
        ("the order is not 2 n / k < 1", _sens(hip, real["h"], p=p, k=0), "not 2 n of the complex plan"),
        ("batch > 1 / a Schur handle", _sens(hip, fs2.real._h, p=(fs2.plan._p,)), "handles with batch > 1 are not supported"),
        ("batch > 1 / both the identity", _sens(hip, f2.real._h, IDENT, IDENT, p=(f2.plan._p,)), "handles with batch > 1 are not supported"),
        ("a Schur handle / k < 1", _sens(hip, fs.real._h, p=(fs.plan._p,), k=0), "not available on a Schur handle (cs3_analyze_schur)"),
        ("k < 1 / both the identity", _sens(hip, h, IDENT, IDENT, p=p, k=0), "k and p must be >= 1"),
        ("both the identity / B = I with k != n", _sens(hip, h, IDENT, IDENT, p=p, k=3, pr=3), "both the identity"),
        ("B = I with k != n / Ctp not monotone", _sens(hip, h, IDENT, CT_PTR, p=p, k=2 * N), "B is the identity but k != n"),
        ("C = I with p != n / Bp not monotone", _sens(hip, h, B_PTR, IDENT, p=p, pr=2 * N), "C is the identity but p != n"),
        ("Bp not monotone / Ctp not monotone", _sens(hip, h, B_PTR, CT_PTR, p=p), "Bp not monotone at column 1"),
        ("Ctp not monotone / an index of B out of range", _sens(hip, h, B_IDX, CT_PTR, p=p), "Ctp not monotone at column 1"),
        ("an index of B / an index of C'", _sens(hip, h, B_IDX, CT_IDX, p=p), "index out of range in column 1 of B"),
        ("an index of C' / side outside 0 .. 2", _sens(hip, h, B, CT_IDX, p=p, side=3), "index out of range in column 1 of C'"),
        ("side outside 0 .. 2 / op outside the enum", _sens(hip, h, p=p, side=3, trans=7), "side must be 0 (auto), 1 (right) or 2 (left)"),
        ("B = I with side right / op outside the enum", _sens(hip, h, IDENT, CT, p=p, side=1, trans=7), "B is the identity, side right"),
        ("C = I with side left / op outside the enum", _sens(hip, h, B, IDENT, p=p, side=2, trans=-1), "C is the identity, side left"),
        ("op outside the enum, last", _sens(hip, h, p=p, trans=3), "op must be 0 (N), 1 (T) or 2 (H)"),
    ])


def test_cs3_updates_plan(hip, real):
    h, hs, big, big2 = real["h"], real["hs"], real["big"], real["big2"]
    _walk(hip, "cs3_updates_plan", [
        ("null handle / null output", _updates(hip, None, out=False), "null handle"),
        ("null output / a Schur handle", _updates(hip, hs, out=False), "null output"),
        ("a Schur handle / null case pointers", _updates(hip, hs, (2, None, None, None)), "not available on a Schur handle (cs3_analyze_schur)"),
        ("a Schur handle / ncases < 1", _updates(hip, hs, ncases=0), "not available on a Schur handle (cs3_analyze_schur)"),
        ("null case pointers / ncases < 1", _updates(hip, h, (0, None, None, None)), "null case pointers"),
        ("ncases < 1 / cp[0] != 0", _updates(hip, h, (0, [1], None, None)), "ncases must be >= 1"),
        ("cp[0] != 0 / cp not monotone", _updates(hip, h, (1, [1, 0], None, None)), "cp[0] != 0"),
        ("cp not monotone / null index arrays", _updates(hip, h, (2, [0, 2, 1], None, None)), "cp not monotone at case 1"),
        ("null index arrays / an index out of range", _updates(hip, h, (1, [0, 1], [N], None)), "null index arrays"),
        ("an index out of range / a case of 17 rows", _updates(hip, big, WIDE_AND_RANGE), "index out of range in case 1"),
        ("a case of 17 rows / batch > 1", _updates(hip, big2, WIDE), "case 0 touches 17 rows and 1 columns (at most 16 of each)"),
        ("batch > 1, last", _updates(hip, real["h2"]), "handles with batch > 1 are not supported"),
    ])


def test_cs3_cplx_updates_plan(hip, real, cplx):
    f, fs, big, big2, bigs, bigs2 = (cplx[k] for k in ("f", "fs", "big", "big2", "bigs", "bigs2"))
    p, h = (f.plan._p,), f.real._h
    pb, hb = (big.plan._p,), big.real._h
    _walk(hip, "cs3_cplx_updates_plan", [
        ("null plan / null output", _updates(hip, h, p=(None,), out=False), "null plan or handle"),
        ("null handle / null output", _updates(hip, None, p=p, out=False), "null plan or handle"),
        ("null output / null case pointers", _updates(hip, h, (2, None, None, None), p=p, out=False), "null output"),
        ("null case pointers / the order is not 2 n", _updates(hip, real["h"], (2, None, None, None), p=p), "null case pointers"),
        ("the order is not 2 n / ncases < 1", _updates(hip, real["h"], p=p, ncases=0), "not 2 n of the complex plan"),
        ("ncases < 1 / cp[0] != 0", _updates(hip, h, (0, [1], None, None), p=p), "ncases must be >= 1"),
        ("cp[0] != 0 / cp not monotone", _updates(hip, h, (1, [1, 0], None, None), p=p), "cp[0] != 0"),
        ("cp not monotone / null index arrays", _updates(hip, h, (2, [0, 2, 1], None, None), p=p), "cp not monotone at case 1"),
        ("null index arrays / an index out of range", _updates(hip, h, (1, [0, 1], [N], None), p=p), "null index arrays"),
        ("an index out of range / a case of 17 rows", _updates(hip, hb, WIDE_AND_RANGE, p=pb), "index out of range in case 1"),
        ("a case of 17 rows / a plan with batch > 1", _updates(hip, hb, WIDE, p=(big2.plan._p,)),
         "case 0 touches 17 rows and 1 columns (at most 16 of each)"),
        ("a case of 17 rows / a handle with batch > 1", _updates(hip, big2.real._h, WIDE, p=pb),
         "case 0 touches 17 rows and 1 columns (at most 16 of each)"),
        ("a plan with batch > 1 / a plan with a border", _updates(hip, hb, p=(bigs2.plan._p,)), "batch > 1 are not supported"),
        ("a handle with batch > 1 / a plan with a border", _updates(hip, big2.real._h, p=(bigs.plan._p,)), "batch > 1 are not supported"),
        ("a plan with a border / a Schur handle", _updates(hip, fs.real._h, p=(fs.plan._p,)), "a complex plan with a border"),
        ("a Schur handle, last", _updates(hip, fs.real._h, p=p), "not available on a Schur handle (cs3_analyze_schur)"),
    ])
