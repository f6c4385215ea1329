"""The matrices of tests/big_step_slice_cases.py against the host analysis alone (no GPU): every case has the fronts that
tests/test_gpu_big_step_slices.py is written for -- two (D + s, D) fronts on one level under a dense parentless root of
order 2 D + s -- with BIG_BLOCK steps in its factor and fused plans, as LU and as Cholesky; and those fronts, with the eight
shapes of tests/big_step_tile_cases.py and tests/big_step_bits_cases.py, reach every bucket of the last block's width twice:
in a front with rows and columns behind its last block (block-column and block-row tiles) and in a parentless root (the
diagonal tile alone).  If the analysis reshapes a case, or a case stops reaching k_big_step, this fails instead of leaving a
slice of the elimination untested."""
import numpy as np
import pytest

import big_step_slice_cases as ss
import big_step_tile_cases as tc
import launch_plan_cases as lp
import sweep_cases as sc

_SEEN = {}          # name -> the wide fronts (r, w, parent is the root / -1) that the analysis returned, LU


@pytest.mark.parametrize("batch", ss.BATCHES)
@pytest.mark.parametrize("kind", ss.KINDS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_fronts_and_plans_of_the_cases(hip, name, kind, batch):
    sym = kind == "chol"
    m, n, Ap, Ai, _ = ss.case_matrix(name, symmetric=sym)
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if sym else hip.CS3_LU, batch=batch) as F:
        K = sc.solve_kinds(hip, F)
        wide = sc.wide_fronts(K)
        fronts = tuple((int(K.r[s]), int(K.w[s])) for s in wide)
        assert fronts == ss.FRONTS[name]
        root = wide[-1]
        assert K.parent[root] == -1 and [int(K.parent[s]) for s in wide[:-1]] == [root, root]
        _SEEN.setdefault(name, fronts)
        for op in ("factor", "fused"):
            rows = lp.plan(hip, F, op, 1)
            # the two launch groups (the fronts below the root; the root) go block step by block step, each with a closing launch
            assert int(np.sum(rows[:, lp.KIND] == lp.BIG_BLOCK)) == sum(-(-w // ss.BIG_NB) + 1 for _, w in ss.FRONTS[name][1:])


def _reached(all_fronts):
    """-> (buckets of the last block's width in fronts with trailing tiles, ... in parentless roots); in every shape the
    last front is the parentless root (asserted above and in test_big_step_tile_cases_cpu.py), the others lie below it."""
    below, roots = set(), set()
    for fronts in all_fronts:
        for r, w in fronts[:-1]:
            assert r > w
            below.add(ss.bucket(ss.last_width(w)))
        r, w = fronts[-1]
        assert r == w
        roots.add(ss.bucket(ss.last_width(w)))
    return below, roots


def test_the_shapes_reach_every_bucket_twice(hip):
    seen = []
    for name in ss.NAMES:                           # from the analysis itself, not from the table
        if name not in _SEEN:
            m, n, Ap, Ai, _ = ss.case_matrix(name)
            with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_LU, batch=1) as F:
                K = sc.solve_kinds(hip, F)
                _SEEN[name] = tuple((int(K.r[s]), int(K.w[s])) for s in sc.wide_fronts(K))
        seen.append(_SEEN[name])
    below, roots = _reached(seen + list(tc.FRONTS.values()) + list(tc.BITS_FRONTS.values()))
    assert below == set(ss.WIDTH_BUCKETS)
    assert roots == set(ss.WIDTH_BUCKETS)


def test_the_new_shapes_alone_stand_beside_the_multiples_of_eight():
    below, roots = _reached(list(ss.FRONTS.values()))
    assert below == {"1", "2-7", "8", "9-15", "16", "17-23", "24", "25-31"}     # ("1": the (129 + s, 129) fronts of the root group)
    assert roots >= {"2-7", "8", "9-15", "17-23", "24", "25-31"}
    assert [ss.last_width(d) for d, _ in ss.BELOW] == [7, 8, 9, 16, 23, 24, 25]
    assert [ss.last_width(2 * d + s) for d, s in ss.ROOT] == [7, 8, 9, 23, 24, 25]


def test_the_buckets():
    assert [ss.bucket(x) for x in (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32)] == [
        "1", "2-7", "2-7", "8", "9-15", "9-15", "16", "17-23", "17-23", "24", "25-31", "25-31", "32"]
    assert [ss.last_width(w) for w in (1, 31, 32, 33, 64, 129, 160)] == [1, 31, 32, 1, 32, 1, 32]


def test_the_cases():
    assert len(ss.CASES) == len({ss.case_id(c) for c in ss.CASES}) == 4 * len(ss.NAMES) + 2 == 54
    assert [c for c in ss.CASES if c[3]] == [("d136s30", "lu", 1, True), ("d129s54", "lu", 1, True)]
