"""The matrices of tests/big_step_tile_cases.py against the host analysis alone (no GPU): every case has the fronts that
tests/test_gpu_big_step_tiles.py is written for -- two (129 + s, 129) fronts on one level under a dense parentless root of
order 258 + s -- with BIG_BLOCK steps in its factor and fused plans, as LU and as Cholesky; and those fronts, with the three
shapes of tests/big_step_bits_cases.py, reach every bucket of the last block's width and of the ragged last tile's extent.
If the analysis reshapes a case, or a case stops reaching k_big_step, this fails instead of leaving a tile path untested."""
import numpy as np
import pytest

import big_step_bits_cases as bb
import big_step_tile_cases as tc
import launch_plan_cases as lp
import sweep_cases as sc
import wide_chunk_cases as wc


@pytest.mark.parametrize("batch", tc.BATCHES)
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("name", tc.NAMES)
def test_fronts_and_plans_of_the_cases(hip, name, kind, batch):
    sym = kind == "chol"
    m, n, Ap, Ai, _ = tc.case_matrix(name, symmetric=sym)
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if sym else hip.CS3_LU, batch=batch) as F:
        K = sc.solve_kinds(hip, F)
        wide = sc.wide_fronts(K)
        assert tuple((int(K.r[s]), int(K.w[s])) for s in wide) == tc.FRONTS[name]
        root = wide[-1]
        assert K.parent[root] == -1 and [int(K.parent[s]) for s in wide[:-1]] == [root, root]
        for op in ("factor", "fused"):
            rows = lp.plan(hip, F, op, 1)
            # the two launch groups (the fronts below the root; the root) go block step by block step, each with a closing launch
            assert int(np.sum(rows[:, lp.KIND] == lp.BIG_BLOCK)) == sum(-(-w // tc.BIG_NB) + 1 for _, w in tc.FRONTS[name][1:])


def test_the_recorded_fronts_of_the_bits_cases():
    assert {name: wc.FRONTS[name] for name in bb.NAMES} == tc.BITS_FRONTS


def test_the_shapes_reach_every_bucket():
    widths, extents, rows = set(), set(), set()
    for fronts in list(tc.FRONTS.values()) + list(tc.BITS_FRONTS.values()):
        for r, w in fronts:
            a, b, c = tc.reach(r, w)
            widths |= a
            extents |= b
            rows |= c
    assert widths == set(tc.WIDTH_BUCKETS)
    assert extents == set(tc.EXTENT_BUCKETS)
    assert rows >= {1, 2, 3, 4, 5}


def test_the_buckets():
    assert [tc.bucket(x) for x in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)] == [
        "1", "2-15", "2-15", "16", "17-31", "17-31", "32", "33-47", "33-47", "48", "49-63", "49-63", "64"]


def test_twenty_cases():
    assert len(tc.CASES) == len({tc.case_id(c) for c in tc.CASES}) == 20
