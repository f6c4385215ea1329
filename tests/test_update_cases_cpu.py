"""The engineered cases of the low-rank-modified solves (tests/update_cases.py), the part that needs no GPU: from the
NumPy reference alone (tests/updates_ref.py) every designed case delivers what it is there for -- a swap at every step,
with a wide margin; the smallest pivot at an interior step; two candidates that are the same bits -- and the reference
solves it within RTOL of a factorisation of the modified matrix; and the plan of a host-only handle cuts every structural
list into the tiles it was built to give."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import RTOL, rel_err
import update_cases as uc
import updates_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pivot_trace_on_matrices_known_by_hand():
    t = uc.pivot_trace(np.array([[1.0, 2.0], [4.0, 3.0]]))                # 4 is taken, then 2 - 3/4 = 1.25
    assert (t.picks, t.swaps, t.pivots, t.smallest_step) == ([1, 1], 1, [4.0, 1.25], 1) and t.margin == 0.75
    t = uc.pivot_trace(np.array([[2.0, 0.0, 0.0], [-2.0, 1.0, 0.0], [2.0, 0.0, 0.5]]))
    assert (t.picks, t.swaps, t.margins[0]) == ([0, 1, 2], 0, 0.0)         # equal candidates: the lowest row
    assert uc.pivot_trace(np.zeros((2, 2))).pivots == [0.0]
    for n in uc.ROW_ORDERS:                                                # the small matrices: any order, dominant
        for spd in (False, True):
            A = uc.base(n, spd).A.toarray()
            off = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
            assert A.shape == (n, n) and np.all(np.diag(A) >= off + 1.0)
            assert (np.array_equal(A, A.T)) == (spd or n == 1)


@pytest.mark.parametrize("n,spd", [(uc.N_PIVOT, False), (uc.N_PIVOT, True), (uc.N_TILES, False)])
def test_designed_cases_deliver_their_pivoting(n, spd):
    B = uc.base(n, spd)
    designed = uc.pivot_cases(n, spd)
    cases = [d.case for d in designed]
    X, rpiv, cond = ur.solve_updates_ref(B.A, B.b, cases)
    seen = {"swaps": 0, "small": 0, "tie": 0, "rect": 0}
    for c, d in enumerate(designed):
        S = uc.reference_S(B, d.case)
        t = uc.pivot_trace(S)
        assert abs(min(t.pivots) / max(1.0, np.abs(S).max()) - rpiv[c]) <= 1e-14, d.name      # the counter is the reference's LU
        err = rel_err(X[:, c], ur.direct_solve(B.A, d.case, B.b))
        print("%-12s %2d x %2d  swaps %2d  margin %.2f  smallest pivot at step %2d  rpiv %.2e  cond(S) %8.1f  error %.1e"
              % (d.name, S.shape[0], len(np.unique(d.case[1])), t.swaps, t.margin, t.smallest_step, rpiv[c], cond[c], err))
        assert err <= RTOL, "%s: the reference is %.3e from the direct solve" % (d.name, err)
        if d.swaps is not None:
            r = S.shape[0]
            assert d.swaps == r - 1 and t.swaps == r - 1 and all(p != k for k, p in enumerate(t.picks[:-1])), (d.name, t.picks)
            assert t.margin >= 0.1, (d.name, t.margins)
            seen["swaps"] += 1
        if d.small:
            assert 0 < d.smallest_step < S.shape[0] - 1 and t.smallest_step == d.smallest_step, (d.name, t.pivots)
            assert 1e-4 <= rpiv[c] <= 1e-2, (d.name, rpiv[c])
            seen["small"] += 1
        elif d.swaps is not None:
            assert rpiv[c] >= 0.5 and cond[c] <= 2.0, (d.name, rpiv[c], cond[c])
        if d.tie:
            assert S[1, 0] == S[2, 0] and abs(S[1, 0]) > max(abs(S[0, 0]), abs(S[3, 0])), S[:, 0]
            assert t.picks[0] == 1 and t.margins[0] == 0.0 and min(t.margins[1:]) >= 0.1, (t.picks, t.margins)
            seen["tie"] += 1
        if d.name.startswith("rect"):
            shape = (len(np.unique(d.case[0])), len(np.unique(d.case[1])))
            assert shape in uc.RECT_SHAPES
            seen["rect"] += 1
    assert seen == {"swaps": len(uc.RANKS) + 3 + 4 + 1, "small": 4, "tie": 1, "rect": len(uc.RECT_SHAPES)}
    ranks = sorted(len(np.unique(d.case[0])) for d in designed if d.name.startswith("cyclic") and "up" not in d.name)
    assert ranks == list(uc.RANKS)
    wide = [d for d in designed if d.name == "wide5x9"][0]
    assert (len(np.unique(wide.case[0])), len(np.unique(wide.case[1]))) == (5, 9)


def test_the_exact_zero_case_is_exact_in_the_reference_too():
    B = uc.base_exact_zero()
    i = uc.ZERO_ROW
    e = np.zeros(B.n)
    e[i] = 1.0
    assert B.lu.solve(e)[i] == 0.5 and B.A[i, i] == 2.0
    _, rpiv, _ = ur.solve_updates_ref(B.A, B.b, [(np.array([i]), np.array([i]), np.array([-2.0]))])
    assert rpiv[0] == 0.0


def _handle(hip, B):
    return hip.Factorization(B.m, B.n, B.Ap, B.Ai)


@pytest.mark.parametrize("name", list(uc.tile_lists()))
def test_structural_lists_give_their_tiles(hip, name):
    cases, tiles = uc.tile_lists()[name]
    B = uc.base(uc.N_TILES)
    with _handle(hip, B) as F, F.updates_plan([(c[0], c[1]) for c in cases]) as plan:
        got = plan.tiles()
        assert got.tolist() == [list(t) for t in tiles], name
        info = plan.info
        assert info.ncases == len(cases) == sum(t[1] for t in tiles) and info.ntiles == len(tiles)
    for first, nc, rows, w in tiles:
        assert nc <= uc.MAX_TILE_CASES and rows <= uc.MAX_TILE and w == uc.width(rows)
        touched = np.unique(np.concatenate([np.asarray(c[0], dtype=np.int64) for c in cases[first:first + nc]]))
        assert len(touched) == rows


def test_the_lists_reach_the_edges_they_are_named_for():
    L = uc.tile_lists()
    assert {1, 64, 512, 513, 1024} <= {t[0][1] for _, t in L.values() if len(t) == 1}       # cases of a single tile
    assert [t[1] for t in L["cases1025"][1]] == [1024, 1]
    last = L["cases64_rows1024"][0][-1]
    assert np.unique(last[0]).tolist() == list(range(1008, 1024))          # first-use order = row order: positions 1008 ..
    assert sorted({len(np.unique(c[0])) for c in L["ranks_0_1_16"][0]}) == [0, 1, 16]
    boundary = L["rows1024_fits"][0][64]                                   # arrives at 1023 rows: one old row, one fresh
    head = np.unique(np.concatenate([c[0] for c in L["rows1024_fits"][0][:64]]))
    assert len(head) == 1023 and np.isin(np.unique(boundary[0]), head).tolist() == [True, False]
    cases, twin, lanes = uc.flagged_lists()
    assert lanes == (0, 63, 64, len(cases) - 1) and len(cases) == len(twin) == uc.FLAGGED_NC
    B = uc.base(uc.N_PIVOT)
    _, rpiv, _ = ur.solve_updates_ref(B.A, B.b, cases, 1e-10)
    assert [c for c in range(len(cases)) if rpiv[c] <= 1e-13] == list(lanes) and np.delete(rpiv, lanes).min() >= 0.5
    assert all(len(twin[c][0]) == 0 for c in lanes)


def test_flagged_list_is_one_tile(hip):
    cases, twin, lanes = uc.flagged_lists()
    with _handle(hip, uc.base(uc.N_PIVOT)) as F:
        for lst in (cases, twin):
            with F.updates_plan([(c[0], c[1]) for c in lst]) as plan:
                t = plan.tiles()
                assert t.shape == (1, 4) and t[0, 1] == uc.FLAGGED_NC


@pytest.mark.parametrize("n", uc.ROW_ORDERS)
def test_row_lists_have_their_ranks_and_the_odd_tail_is_read(hip, n):
    cases = uc.row_list(n)
    assert [len(np.unique(c[0])) for c in cases] == [min(n, 16), 1, 2][:len(cases)] and len(cases) == (3 if n > 1 else 2)
    assert cases[1][0].tolist() == [n - 1]
    with _handle(hip, uc.base(n)) as F, F.updates_plan([(c[0], c[1]) for c in cases]) as plan:
        assert plan.tiles()[:, 3].tolist() == [64]                         # default width: one tile
    if n > 16:
        assert n - 1 not in cases[0][0]                                    # ... so the last row is the tile's 17th


_CHILD = ("import json, sys\n"
          "sys.path.insert(0, 'tests')\n"
          "from csparse3_amd import csc_hip as hip\n"
          "import update_cases as uc\n"
          "name = sys.argv[1]\n"
          "if name.startswith('rows'):\n"
          "    n = int(name[4:]); cases = uc.row_list(n); B = uc.base(n)\n"
          "elif name.startswith('pivot'):\n"
          "    spd = name == 'pivot_spd'; cases = [d.case for d in uc.pivot_cases(uc.N_PIVOT, spd)]; B = uc.base(uc.N_PIVOT, spd)\n"
          "else:\n"
          "    cases = uc.odd_width_lists()[name][0]; B = uc.base(uc.N_PIVOT)\n"
          "with hip.Factorization(B.m, B.n, B.Ap, B.Ai) as F, F.updates_plan([(c[0], c[1]) for c in cases]) as p:\n"
          "    print(json.dumps(p.tiles().tolist()))\n")


def _tiles_in_a_child(name, tile):
    import json
    out = subprocess.run([sys.executable, "-c", _CHILD, name], cwd=ROOT, env=dict(os.environ, CS3_UPD_TILE=str(tile)),
                         capture_output=True, text=True, check=True).stdout
    return [tuple(t) for t in json.loads(out)]


def test_odd_widths():
    """CS3_UPD_TILE = 9 with ranks up to 9, and 1 and 9 with a rank-15 list (a tile is never narrower than the list's
    largest rank: 15): odd solve widths, the ones whose stages of Z have an odd last entry.  (A child process per width:
    the switch must not leak into this one.)"""
    for name, (cases, tile, tiles) in uc.odd_width_lists().items():
        got = _tiles_in_a_child(name, tile)
        assert got == tiles, (name, got)
        assert all(t[3] % 2 == 1 for t in got)
    # the row lists at the widths the GPU test runs them at: 9 is odd only while the largest rank is <= 9, hence 17
    assert _tiles_in_a_child("rows9", 9) == [(0, 3, 9, 9)]
    assert _tiles_in_a_child("rows137", 9)[0] == (0, 1, 16, 16)
    t = _tiles_in_a_child("rows137", 17)
    assert t[0] == (0, 2, 17, 17) and all(x[3] == 17 for x in t)
    assert _tiles_in_a_child("rows7", 17) == [(0, 3, 7, 17)]


def test_at_width_16_every_rank_16_case_fills_a_tile_of_its_own():
    for name, spd in (("pivot", False), ("pivot_spd", True)):
        tiles = _tiles_in_a_child(name, 16)
        full = [c for c, d in enumerate(uc.pivot_cases(uc.N_PIVOT, spd)) if len(np.unique(d.case[0])) == 16]
        assert len(full) == 5 and all((c, 1, 16, 16) in tiles for c in full), tiles
