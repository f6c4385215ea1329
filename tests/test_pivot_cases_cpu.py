"""The engineered pivot cases of tests/pivot_cases.py against the CPU oracle alone (no GPU): the target list that
tests/test_gpu_pivot_threshold.py runs reaches every factor kernel class, has an accept side for (nearly) all targets,
and the oracle decides each target exactly as the construction says it must."""
import collections

import numpy as np
import pytest

import pivot_cases as pc
from helpers import assert_backward_error, backward_error_ratio, permuted

NAMES = list(pc.LU_CASES)


@pytest.mark.parametrize("name", NAMES, ids=["%s-b%d" % nm for nm in NAMES])
def test_target_list_reaches_every_class_with_an_accept_side(hip, orc, name):
    case = pc.lu_case(hip, orc, name)
    per = collections.defaultdict(list)
    for p in case["targets"]:
        assert case["FR"].cls[p.target.front] == p.target.cls
        per[p.target.cls].append(p)
    for cls in pc.LU_CASES[name]:
        got = per[cls]
        assert all(p.weight >= pc.DECISION_WEIGHT for p in got)
        accept = [p for p in got if p.rho is not None and p.weight >= pc.MIN_WEIGHT]       # ... whose factors are compared
        assert len(accept) >= 3, "%s: %d targets with an accept side" % (cls, len(accept))
        reject_only = [p for p in got if p.rho is None]
        assert 5 * len(reject_only) <= len(got), "%s: %d of %d targets are reject-only" % (cls, len(reject_only), len(got))
        # the column maximum sits where it was steered to, and both near the pivot and far from it somewhere
        assert all(p.i_max == p.target.i for p in got if p.target.i is not None)
        assert len(set(p.target.where for p in got) - {"any"}) >= 2, cls
        labels = [lab for lab, *_ in case["pairs"]]
        assert cls in labels, "%s has no two-failure case" % cls
        if cls.startswith("forest"):                          # a leaf front and one on its task's top local level
            assert {"leaf", "top"} <= set(p.target.label.split(" ")[1] for p in got)
    if "il" in pc.LU_CASES[name]:
        assert {"il order", "il rows"} <= set(lab for lab, *_ in case["pairs"])


@pytest.mark.parametrize("name", NAMES, ids=["%s-b%d" % nm for nm in NAMES])
def test_oracle_rejects_exactly_the_engineered_pivot(hip, orc, name):
    case = pc.lu_case(hip, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    for p in case["targets"]:
        rho = pc.reject_rho(p)
        assert pc.first_off_diagonal(orc, n, Ap, Ai, p.Ax, q, rho * (1 + pc.MARGIN)) == p.target.k, p.target.label
        if p.rho is not None:
            assert pc.first_off_diagonal(orc, n, Ap, Ai, p.Ax, q, rho * (1 - pc.MARGIN)) is None, p.target.label
    for label, t1, t2, Ax2, tol in case["pairs"]:
        assert t1.front == t2.front and t1.k < t2.k
        assert pc.first_off_diagonal(orc, n, Ap, Ai, Ax2, q, tol) == t1.k, label
        # ... and both columns hold a multiplier beyond 1 / tol in the factors with every diagonal kept
        Lp, Li, Lx = orc.csc_lu_f(n, n, Ap, Ai, Ax2, q, 0.0)[:3]
        for t in (t1, t2):
            assert np.abs(pc.column_of_l(Lp, Li, Lx, t.k)[1]).max() > 1.0 / tol, label


def test_il_order_pair_fails_where_the_program_order_would_mislead(hip, orc):
    """'il order': column c0 + 2 has its only failing multiplier inside the diagonal 4 x 4 block, column c0 only below it;
    'il rows': column c0 fails in a later 8-row tile than column c0 + 1."""
    case = pc.lu_case(hip, orc, ("grid3000", 130))
    m, n, Ap, Ai, Ax = case["mat"]
    FR = case["FR"]
    for label, t1, t2, Ax2, tol in case["pairs"]:
        if not label.startswith("il "):
            continue
        Lp, Li, Lx = orc.csc_lu_f(n, n, Ap, Ai, Ax2, FR.q, 0.0)[:3]
        c0, w = int(FR.c0[t1.front]), int(FR.w[t1.front])
        ke = c0 + min(4, w)
        bad = {}
        for t in (t1, t2):
            rows, vals = pc.column_of_l(Lp, Li, Lx, t.k)
            bad[t.k] = rows[np.abs(vals) > 1.0 / tol]
            assert len(bad[t.k]) > 0
        if label == "il order":
            assert (bad[t1.k] >= ke).all() and (bad[t2.k] < ke).all()
        else:
            pos = lambda i: (np.searchsorted(FR.rows[t1.front], i) - (ke - c0)) // 8          # noqa: E731
            assert (bad[t1.k] >= ke).all() and (bad[t2.k] >= ke).all()
            assert min(pos(i) for i in bad[t1.k]) > max(pos(i) for i in bad[t2.k])


@pytest.mark.parametrize("name", NAMES, ids=["%s-b%d" % nm for nm in NAMES])
def test_oracle_factors_meet_the_componentwise_bound(hip, orc, name):
    """Higham's bound holds for cs_lu's own factors of every engineered matrix (multipliers up to 1 / rho)."""
    case = pc.lu_case(hip, orc, name)
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    worst = 0.0
    for p in case["targets"]:
        if p.rho is None or p.weight < pc.MIN_WEIGHT:
            continue
        oL = orc.csc_lu_f(n, n, Ap, Ai, p.Ax, q, p.rho * (1 - pc.MARGIN))
        worst = max(worst, assert_backward_error(n, permuted(n, Ap, Ai, p.Ax, q), oL[0:3], oL[3:6], p.target.label))
    print("%s: oracle max |PAQ - LU| / (u |L||U|) = %.2f" % (name, worst))


def test_backward_error_check_sees_one_wrong_small_entry(orc):
    """The componentwise check fails on an error that the norm-wise 1e-10 of assert_factor_equal cannot see."""
    m, n, Ap, Ai, Ax = pc.matrix("db100")
    q = orc.csc_amd_f(1, n, n, Ap, Ai)
    Lp, Li, Lx, Up, Ui, Ux, _ = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, 1e-3)
    A = permuted(n, Ap, Ai, Ax, q)
    assert backward_error_ratio(n, A, (Lp, Li, Lx), (Up, Ui, Ux)) [0] <= 2 * n
    small = np.argmin(np.where(Lx != 0, np.abs(Lx), np.inf))
    Lx2 = Lx.copy()
    Lx2[small] *= 1 + 1e-9                                    # 1e-9 relative on the smallest entry of L
    assert np.abs(Lx2 - Lx).max() / np.abs(Lx).max() < 1e-10
    with pytest.raises(AssertionError):
        assert_backward_error(n, A, (Lp, Li, Lx2), (Up, Ui, Ux), "perturbed")
