"""The matrices of tests/wide_chunk_cases.py against the host analysis alone (no GPU): every case has the fronts that
tests/test_gpu_wide_chunks.py is written for -- two (d + s, d) fronts on one level under a parentless (2 d + s, 2 d + s)
root, all swept as SK_BIG -- and the restated plan sends them down the 256-column path for the pairs that are meant to
take it.  If the analysis reshapes a case, this fails instead of leaving k_fwd_big_step4 / k_bwd_big_step4 untested."""
import pytest

import sweep_cases as sc
import wide_chunk_cases as wc

KINDS = ("lu", "chol")


@pytest.mark.parametrize("batch", wc.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(wc.CASES))
def test_fronts_of_the_cases(hip, name, kind, batch):
    m, n, Ap, Ai, _ = wc.case_matrix(name, symmetric=kind == "chol")
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU, batch=batch) as F:
        assert F.n == wc.ORDER[name] <= 1058
        K = sc.solve_kinds(hip, F)
        level = F.supernodes()[2]
    wide = sc.wide_fronts(K)
    assert tuple((int(K.r[s]), int(K.w[s])) for s in wide) == wc.FRONTS[name]
    root = wide[-1]
    assert K.parent[root] == -1 and [int(K.parent[s]) for s in wide[:-1]] == [root, root]
    assert [K.kind[s] for s in wide] == ["big"] * 3
    # the two non-root fronts share a level (one launch group of two), the root is alone on the last one
    assert level[wide[0]] == level[wide[1]] < level[root]
    assert [s for s in range(len(K.w)) if level[s] == level[root]] == [root]
    assert [s for s in range(len(K.w)) if level[s] == level[wide[0]] and K.kind[s] == "big"] == wide[:-1]


def test_the_pairs_take_the_chunk_widths_they_are_there_for():
    for name in wc.CASES:
        below, root = wc.FRONTS[name][:2], wc.FRONTS[name][2:]
        for pair in wc.PAIRS_NEW:
            assert wc.chunk_width(*pair, below[0][1]) == wc.chunk_width(*pair, root[0][1]) == 256
            assert wc.skips_init(*pair, root) and not wc.skips_init(*pair, below)
        for pair in wc.PAIRS_OLD:
            assert wc.chunk_width(*pair, root[0][1]) == 64 and not wc.skips_init(*pair, root)
    assert {b for b, _ in wc.PAIRS_NEW + wc.PAIRS_OLD} == set(wc.BATCHES)
    # fronts of at most 128 pivots keep the two-block launches
    assert wc.chunk_width(1, 1, 128) == 128 and wc.chunk_width(1, 1, 129) == 256


def test_the_cases_cover_the_widths_where_the_kernels_change_path():
    widths = sorted({w for name in wc.CASES for _, w in wc.FRONTS[name]})
    nblocks = {-(-min(256, w - 256 * c) // 64) for w in widths for c in range(-(-w // 256))}
    assert nblocks == {1, 2, 3, 4}                                         # 64-blocks in a chunk
    last = {w - 256 * (-(-w // 256) - 1) for w in widths}
    assert {1, 30, 32, 256} <= last                                        # columns of the last chunk
    assert {-(-w // 256) for w in widths} == {1, 2, 3}                     # chunks per front
    assert {r - w for name in wc.CASES for r, w in wc.FRONTS[name]} == {0, 30, 200}
