"""The cases of tests/big_step_flag_cases.py against the host analysis and the CPU oracle alone (no GPU): every target of
tests/test_gpu_big_step_flags.py lies in the tile, half and block its case names, fails in that place and nowhere else
in its column, and the oracle decides it as the construction says."""
import numpy as np
import pytest

import big_step_flag_cases as bc
import pivot_cases as pc


def _want(site):
    block, col, rows = site
    tile, part = (0, None) if rows == "diag" else rows
    return block, "lo" if col < 16 else "hi", tile, part


def _assert_place(FR, s, k, i, site, what):
    got = bc.place(FR, s, k, i)
    assert (got.block, got.half, got.tile, got.rows) == _want(site), "%s: row %d of column %d lies at %r" % (what, i, k, got)
    return got


def test_the_front_is_the_one_the_cases_assume(hip):
    for name, batch in ((bc.LU, 1), (bc.CHOL, 1), (bc.LU, 2)):
        mat, FR, s = bc.analysis(hip, name, batch)
        assert FR.cls[s] == "big_step" and FR.batch == batch
        # a root of 7 blocks, the last one partial with columns in both halves; three block-column tiles behind block 0
        assert FR.r[s] == FR.w[s] == 210 and FR.w[s] % bc.BIG_NB == 18 and FR.c0[s] + FR.w[s] == FR.n
        assert np.array_equal(FR.rows[s], np.arange(FR.c0[s], FR.n))


def test_multiplier_targets_lie_where_their_names_say(hip, orc):
    (m, n, Ap, Ai, Ax), FR, s = bc.analysis(hip)
    cases = bc.multiplier_cases(hip, orc)
    assert list(cases) == list(bc.MULTIPLIER_SITES)
    for label, p in cases.items():
        site = bc.MULTIPLIER_SITES[label]
        got = _assert_place(FR, s, p.target.k, p.target.i, site, label)
        assert got.partial == ("partial" in label)
        # pivot_cases keeps the target (its 1e-6 rule), both sides exist, the factors can be compared
        assert p.weight >= pc.MIN_WEIGHT and p.rho is not None and p.i_max == p.target.i, label
        lo, hi = p.rho * (1 - pc.MARGIN), p.rho * (1 + pc.MARGIN)
        assert pc.first_off_diagonal(orc, n, Ap, Ai, p.Ax, FR.q, lo) is None, label
        assert pc.first_off_diagonal(orc, n, Ap, Ai, p.Ax, FR.q, hi) == p.target.k, label
        # the column fails in the steered row alone: no other check of the launch sees it
        bad, rest = bc.failing_rows(orc, n, Ap, Ai, p.Ax, FR.q, p.target.k, hi)
        assert list(bad) == [p.target.i] and rest < 0.7, (label, bad, rest)
    # 'col last tile': the rows are those of a partial tile (fewer than 64 rows, fewer than 32 in its lower part)
    t = cases["col last tile"].target
    assert FR.r[s] - (32 + 128) == 50 and bc.place(FR, s, t.k, t.i).tile == 3


@pytest.mark.parametrize("which", ["pair", "lane"])
def test_two_failures_lie_where_their_names_say(hip, orc, which):
    (m, n, Ap, Ai, Ax), FR, s = bc.analysis(hip)
    cases = bc.pair_cases(hip, orc) if which == "pair" else bc.one_lane_cases(hip, orc)
    for label, (t1, t2, Ax2, tol) in cases.items():
        assert t1.k < t2.k and (t1.k - FR.c0[s]) // bc.BIG_NB == (t2.k - FR.c0[s]) // bc.BIG_NB, "one launch"
        assert pc.first_off_diagonal(orc, n, Ap, Ai, Ax2, FR.q, tol) == t1.k, label
        assert pc.first_off_diagonal(orc, n, Ap, Ai, Ax2, FR.q, pc.RHOS[0] * (1 - pc.MARGIN)) is None, label
        bad1, rest1 = bc.failing_rows(orc, n, Ap, Ai, Ax2, FR.q, t1.k, tol)
        bad2, rest2 = bc.failing_rows(orc, n, Ap, Ai, Ax2, FR.q, t2.k, tol)
        assert list(bad1) == [t1.i] and list(bad2) == [t2.i] and max(rest1, rest2) < 0.7, (label, bad1, bad2)
        if which == "pair":
            s1, s2 = bc.PAIR_SITES[label]
            p1, p2 = _assert_place(FR, s, t1.k, t1.i, s1, label), _assert_place(FR, s, t2.k, t2.i, s2, label)
            assert (p1.tile == 0) != (p2.tile == 0), "one failure in the diagonal tile, one in a block-column tile"
        else:
            block, j1, j2, rows = bc.ONE_LANE_SITES[label]
            assert t1.i == t2.i and (j1 < 16) == (j2 < 16), "one lane: the same row, both columns on one wave"
            _assert_place(FR, s, t1.k, t1.i, (block, j1, rows), label)
            _assert_place(FR, s, t2.k, t2.i, (block, j2, rows), label)


def test_diagonal_targets(hip, orc):
    """The pivot itself: the columns sit in both halves of a full and of the partial block; the oracle finds no pivot in a
    zero column, keeps a pivot of 1e301 (the kernels' overflow guard has no counterpart in cs_lu), and decides the
    Cholesky pivots of -+ 1e-6 a as tests/test_gpu_pivot_threshold.py describes."""
    (m, n, Ap, Ai, Ax), FR, s = bc.analysis(hip)
    cols = bc.diagonal_columns(FR, s)
    got = [bc.place(FR, s, k, k) for k in cols]
    assert [(g.block, g.half, g.partial, g.tile) for g in got] == [(1, "lo", False, 0), (1, "hi", False, 0), (6, "lo", True, 0), (6, "hi", True, 0)]
    assert cols[-1] == n - 1
    for k in cols:
        with pytest.raises(orc.SingularMatrix, match="no pivot at step %d$" % k):
            orc.csc_lu_f(n, n, Ap, Ai, bc.with_zero_column(Ap, Ai, Ax, FR.q, k), FR.q, 1e-3)
        assert pc.first_off_diagonal(orc, n, Ap, Ai, bc.with_entry(Ap, Ai, Ax, FR.q, k, k, 1e301), FR.q, 1e-3) is None
    (m, n, Ap, Ai, Ax), FR, s = bc.analysis(hip, bc.CHOL)
    assert bc.diagonal_columns(FR, s) == cols
    for k in cols:
        assert pc.chol_fail_step(orc, n, Ap, Ai, pc.engineer_chol(orc, n, Ap, Ai, Ax, FR.q, k, -1.0), FR.q) == k
        later = pc.chol_fail_step(orc, n, Ap, Ai, pc.engineer_chol(orc, n, Ap, Ai, Ax, FR.q, k, +1.0), FR.q)
        assert later == (k + 1 if k < n - 1 else None)


def test_nan_targets(hip):
    """A has the entries that the NaN cases overwrite: the pivot, a row of the diagonal tile, a row of a block-column tile."""
    (m, n, Ap, Ai, Ax), FR, s = bc.analysis(hip)
    for label, (k, i) in bc.nan_entries(FR, Ap, Ai, s).items():
        got = bc.place(FR, s, k, i)
        assert (got.block, got.half) == (1, "lo") and (got.tile == 0) == (label != "col") and (i == k) == (label == "pivot")
