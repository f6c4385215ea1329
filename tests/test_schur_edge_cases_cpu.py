"""The matrices of tests/schur_edge_cases.py against the host analysis alone (no GPU): every case, for LU and Cholesky and
every batch, has the fronts that tests/test_gpu_schur_edges.py is written for -- one interior front (d + s, d) per block
with the factor class of the table, below a last supernode (s, s) that is parentless and alone on the last level -- the
Schur front's restated sweep kind is the table's, and the (batch, right-hand sides) pairs of the GPU tests take the
paths they are meant to take.  If the analysis reshapes a case, this fails instead of leaving a kernel silently untested.
The reference is checked against a second float64 route and printed with its margin."""
import numpy as np
import pytest

import pivot_cases as pc
import schur_edge_cases as se
import sweep_cases as sc
from helpers import RTOL, rel_err

KINDS = ("lu", "chol")

# the Schur front's sweep kind per case: (batch < 16, batch >= 16)
KIND_TABLE = {"s5": ("small", "small"), "s16": ("small", "small"), "s17": ("small", "small"), "s31": ("small", "small"),
              "s32": ("small", "small"), "s33": ("wave", "wave"), "s64": ("wave", "wave"), "s65": ("block", "block"),
              "s96": ("block", "block"), "s129": ("block", "block"), "s136": ("block", "block"), "s137": ("big", "block"),
              "s256": ("big", "block"), "s257": ("big", "block"), "s288mix": ("big", "block")}


@pytest.mark.parametrize("batch", se.BATCHES_CPU)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(se.CASES))
def test_fronts_of_the_cases(hip, name, kind, batch):
    m, n, Ap, Ai = se.pattern(name, symmetric=kind == "chol")
    idx = se.schur_set(name)
    ns = se.NS[name]
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU, batch=batch, schur=idx) as F:
        assert F.n == se.ORDER[name] <= 600
        assert np.array_equal(F.schur_info(), idx) and np.array_equal(F.ordering()["q"][n - ns:], idx)
        K = sc.solve_kinds(hip, F)
        sn_ptr, _, level = F.supernodes()
    last = len(K.w) - 1
    print("%s %s batch %d: %s" % (name, kind, batch, [(int(r), int(w), c, k) for r, w, c, k in zip(K.r, K.w, K.cls, K.kind)]))
    # the Schur front: (s, s), the last columns, parentless, alone on the last level, never matrix-interleaved
    assert (int(K.r[last]), int(K.w[last])) == (ns, ns) and sn_ptr[last] == n - ns
    assert K.parent[last] == -1 and K.cls[last] == "schur"
    assert [s for s in range(last + 1) if level[s] == level[last]] == [last] and level[last] == max(level)
    assert K.kind[last] == se.schur_kind(ns, batch) == KIND_TABLE[name][batch > sc.BIG_BATCH_MAX]
    # the interior: one front per block, every one a child of the Schur front, on one level
    assert sorted((int(K.r[s]), int(K.w[s])) for s in range(last)) == sorted(se.INTERIOR[name])
    assert all(K.parent[s] == last for s in range(last)) and len({int(level[s]) for s in range(last)}) == 1
    for s in range(last):
        r, w = int(K.r[s]), int(K.w[s])
        want = se.INTERIOR_CLASS.get(name, pc._front_class(r, w, batch >= 8, batch >= 128))
        assert se.CLASS_OF_KERNEL[K.cls[s]] == want == pc._front_class(r, w, batch >= 8, batch >= 128), (s, K.cls[s])
    if name == "s5":                                                       # the one-variable interior changes class with the batch
        assert K.cls[0] == {1: "mix_wave", 2: "mix_wave", 7: "mix_wave", 16: "wave", 130: "il"}[batch]
    if se.INTERIOR_CLASS.get(name) == "big":                               # wide interior fronts: SK_BIG below a batch of 16
        wide = [s for s in range(last) if K.w[s] > sc.WAVE_WMAX]
        assert wide and {K.kind[s] for s in wide} == {"big" if batch <= sc.BIG_BATCH_MAX else "block"}


def test_the_sweep_kind_edges_come_from_the_restated_rule():
    """The cases sit on both sides of every bound of sweep_cases.kind_of for a front with r = w."""
    ns = set(se.NS.values())
    assert {sc.SMALL_RMAX, sc.SMALL_RMAX + 1} <= ns                        # SK_SMALL | SK_WAVE
    assert {sc.WAVE_WMAX, sc.WAVE_WMAX + 1} <= ns                          # SK_WAVE | SK_BLOCK
    assert {sc.BIG_RMIN - 1, sc.BIG_RMIN} <= ns                            # SK_BLOCK | SK_BIG
    assert {16, 17} <= ns                                                  # the order of matrix-interleaved fronts (FC_IL)
    for batch in (sc.BIG_BATCH_MAX, sc.BIG_BATCH_MAX + 1):
        assert se.schur_kind(sc.BIG_RMIN, batch) == ("big" if batch <= sc.BIG_BATCH_MAX else "block")
    assert {b for b, _ in se.HALF_PAIRS} >= {sc.BIG_BATCH_MAX, sc.BIG_BATCH_MAX + 1}


def test_the_pairs_take_the_paths_they_are_there_for():
    for name in se.HALF_CASES:
        ns = se.NS[name]
        for batch, k in se.half_pairs(name):
            pl = se.sweep_plan(ns, batch, k)
            print("%s ns %d batch %d k %d: %s" % (name, ns, batch, k, pl))
            assert pl.kind == KIND_TABLE[name][batch > sc.BIG_BATCH_MAX]
            if k >= se.GEMM_MIN:
                assert pl.path == ("rhs" if ns <= sc.SMALL_RMAX else "gemm")
            elif pl.kind == "big":
                wide = batch * k < 8
                assert pl.cw == ((256 if ns > 128 else 128) if wide else 64)
                assert pl.no_init == (wide and ns > 128) and pl.nchunk == -(-ns // pl.cw)
            else:
                assert pl.path == {"small": "wave", "wave": "wave", "block": "block"}[pl.kind]
    plans = {(name, p): se.sweep_plan(se.NS[name], *p) for name in se.HALF_CASES for p in se.half_pairs(name)}
    # the 256-column path: one chunk and two (the second of one column), without an init launch, alone and in a batch of 2 and 7
    assert {(pl.cw, pl.nchunk, pl.no_init) for (name, _), pl in plans.items() if name == "s257" and pl.cw == 256} == {(256, 2, True)}
    assert {p for (name, p), pl in plans.items() if name == "s257" and pl.cw == 256} == {(1, 1), (1, 7), (2, 3), (7, 1)}
    assert {p for (name, p), pl in plans.items() if name == "s257" and pl.cw == 64} == {(1, 8), (2, 4), (15, 1)}
    assert plans["s137", (1, 1)][2:] == (256, 1, True) and plans["s288mix", (1, 7)][2:] == (256, 2, True)
    # SK_BIG Schur fronts in batches of 2 to 15, and the block kernel from 16 on
    assert {p[0] for (name, p), pl in plans.items() if pl.path == "big"} == {1, 2, 7, 15}
    assert plans["s137", (16, 1)].path == plans["s137", (130, 1)].path == "block"
    # every path of every kind
    assert {(pl.kind, pl.path) for pl in plans.values()} == {("small", "wave"), ("small", "rhs"), ("wave", "wave"), ("wave", "gemm"),
                                                            ("block", "block"), ("block", "gemm"), ("big", "big"), ("big", "gemm")}


def test_the_cases_cover_the_tiles_kinds_and_chunks():
    ns = sorted(se.NS.values())
    assert {0, 1, se.ST - 1} <= {v % se.ST for v in ns}
    assert {1, 2, 3, 5, 9} <= {-(-v // se.ST) for v in ns}                 # tiles per side
    assert {se.schur_kind(v, 1) for v in ns} == {"small", "wave", "block", "big"}
    assert {se.sweep_plan(v, 1, 1).nchunk for v in ns if se.schur_kind(v, 1) == "big"} == {1, 2}
    assert {v for v in ns if v % se.ST == 0} >= {32, 64, 96, 256}          # Cholesky mirror without a partial tile
    # S in batches: more than one tile column, every sweep kind's order, 64 and more matrices and 16 and more
    assert all(max(b) >= 7 for b in se.S_BATCHES.values()) and {33, 65, 137, 257} == {se.NS[c] for c in se.S_BATCHES}
    assert all({16, 130} <= set(se.S_BATCHES[c]) for c in ("s33", "s65", "s137"))
    assert set(se.HALF_CASES) <= set(se.CASES) and set(se.HALF_CASES_130) <= set(se.HALF_CASES)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(se.CASES))
def test_reference_against_a_second_route(name, kind):
    """cond(A11) < 10 (with a fringe: of A11 with its diagonal scaled to one); W > 0 everywhere; the dense reference and a
    sparse LU of A11 agree within RTOL / 100 W entry-wise (measured: at most 9.2e-16 W), so the bound of the GPU tests has
    five orders of margin over the reference itself.  LU cases: no 32 x 32 tile of S equals its transposed counterpart
    to better than 1e-2 W, so a transposed tile cannot pass an entry-wise bound of 1e-10 W."""
    sym = kind == "chol"
    worst = 0.0
    for variant in (0, 1):
        A = se.scipy_matrix(name, 0, sym, variant)
        idx = se.schur_set(name)
        cond, cond_scaled = se.cond_interior(A, idx)
        S, W = se.reference(name, 0, sym, variant)
        assert S.shape == W.shape == (se.NS[name],) * 2
        # (the chain nodes of a fringe have a diagonal of about 3 beside the blocks' hundreds: cond 129 .. 171 by scaling alone)
        assert cond_scaled < 10 and (cond < 10 or se.CASES[name][2] > 0), (cond, cond_scaled)
        assert W.min() > 0
        ratio = float((np.abs(S - se.second_route(A, idx)) / W).max())
        worst = max(worst, ratio)
        print("%s %s variant %d: cond(A11) %.2f (diagonal scaled to one: %.2f), min W %.3g, |S_ref - S_splu| / W <= %.2e" % (name, kind, variant, cond, cond_scaled, W.min(), ratio))
        assert ratio <= RTOL / 100
        if sym:
            assert (np.abs(S - S.T) <= 1e-14 * W).all()
        else:                                              # an LU case: no tile of S survives a transposition
            margin = se.transposed_tile_margin(S, W)
            print("%s variant %d: a transposed tile misses by at least %.2f W (norm-wise %.1e)" % (name, variant, margin, rel_err(S, S.T)))
            assert margin > 1e-2
    assert worst <= RTOL / 100
