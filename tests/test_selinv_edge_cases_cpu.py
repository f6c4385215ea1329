"""The matrices of tests/selinv_edge_cases.py against the host analysis alone (no GPU): every case, by every kind the GPU
test runs it with, has the fronts, parents and launch groups that selinv_edge_cases.TABLE states, so that
tests/test_gpu_selinv_edges.py cannot silently test something else when the analysis changes; every edge of
selinv_edge_cases.edges() is met by a case; and the inputs are benign -- cond_1 <= COND_MAX, and the float64 restatement
of the recurrence stays within 1e-12 PER BLOCK of the dense inverse -- so that the GPU bound is about the kernels."""
import collections

import numpy as np
import pytest

import selinv_cases as sc
import selinv_edge_cases as se
import selinv_ref as ref

RESTATEMENT_BOUND = 1e-12     # per block; measured: at most 1.1e-14, cond_1 at most 6.5e2


def _orders(name, kind, hip):
    case = se.matrix(name, 0, kind == "chol")
    return sc._front_orders(case[1], case[2], case[3], hip.CS3_CHOLESKY if kind == "chol" else hip.CS3_LU)


@pytest.mark.parametrize("name,kind", se.GPU_CASES)
def test_fronts_and_groups_of_the_cases(hip, name, kind):
    want = se.TABLE[name]
    with se.analysed(name, kind) as F:
        assert F.n <= 800
        P = se.plan_fronts(F)
        info = F.selinv_info()
    print("%s %s: n = %d, %s, groups %s" % (name, kind, F.n, sorted(collections.Counter((f.r, f.w) for f in P).items()),
                                         [(g[0].cls, len(g)) for g in se.groups(P)]))
    # (r, w, parent) as the analysis schedules them are the plan's
    order_of = {f.s: f.r for f in P}
    assert sorted((r, w, parent) for r, w, parent in _orders(name, kind, hip)) == sorted((f.r, f.w, f.parent) for f in P)
    # the roots, the fronts the case is there for, and nothing else beyond the wave class
    assert sorted(f.r for f in P if f.parent < 0) == sorted(want.roots) and all(f.c == 0 for f in P if f.parent < 0)
    below = [(f.r, f.w, order_of[f.parent]) for f in P if f.parent >= 0]
    named = [b for b in below if se.class_of(b[0]) != "wave"] if want.rest else below
    assert sorted(named) == sorted(want.fronts)
    rest = [b for b in below if se.class_of(b[0]) == "wave"] if want.rest else []
    assert len(rest) == want.rest
    assert all(f.c > 0 and f.r > f.w for f in P if f.parent >= 0)
    # the launch groups: which fronts share a launch, the class of each group from r, parents in earlier launches
    G = se.groups(P)
    assert [(g[0].cls, len(g)) for g in G] == want.groups
    assert all(len({f.cls for f in g}) == 1 for g in G)
    launches = [g[0].launch for g in G]
    assert launches == list(np.cumsum([0] + [3 if g[0].cls == "big" else 1 for g in G[:-1]]))
    launch_of = {f.s: f.launch for f in P}
    assert all(launch_of[f.parent] < f.launch for f in P if f.parent >= 0)
    assert info.nfronts_big == sum(f.cls == "big" for f in P) and info.nfronts_small == len(P) - info.nfronts_big
    assert info.nlaunches == launches[-1] + (3 if G[-1][0].cls == "big" else 1)
    assert info.zpool_doubles == sum(f.r * f.r for f in P)


def test_two_trees_plan(hip):
    """Two launch groups, the roots first: both roots in one big group, then the four fronts below them -- two shapes,
    two parents -- in another."""
    with se.analysed("two_trees") as F:
        P = se.plan_fronts(F)
    G = se.groups(P)
    assert len(G) == 2
    assert sorted((f.r, f.w, f.parent) for f in G[0]) == [(214, 214, -1), (237, 237, -1)]
    root = {f.r: f.s for f in G[0]}
    assert sorted((f.r, f.w, f.parent) for f in G[1]) == sorted([(142, 72, root[214])] * 2 + [(137, 100, root[237])] * 2)
    assert [g[0].launch for g in G] == [0, 3]
    # the work buffer advances by 2 c w per big front: unequal strides inside the second group
    assert len({2 * f.c * f.w for f in G[1]}) == 2
    # the grids are the maxima over the group: each shape is the smaller one in at least one of them
    grids = [se.big_grids(f) for f in G[1]]
    assert all(len({g[k] for g in grids}) == 2 for k in range(3))


def test_every_edge_is_met_by_a_case(hip):
    plans = {}
    for name in se.CASES:
        with se.analysed(name) as F:
            plans[name] = se.plan_fronts(F)
    missing = []
    for edge, met in se.edges().items():
        hits = [name for name in se.CASES if met(plans[name])]
        print("%-60s %s" % (edge, " ".join(hits)))
        if not hits:
            missing.append(edge)
    assert not missing


def test_the_sizes_at_a_limit_come_from_the_limits():
    lim = se.LIMITS
    first = {name: (spec[0][0], spec[1]) for name, spec in se.SPEC.items()}
    assert first["w64"][0] == lim.diag_block and first["w65"][0] == lim.diag_block + 1
    assert first["w128"] == (2 * lim.diag_block, lim.gemm_tile) and first["w129"] == (2 * lim.diag_block + 1, lim.gemm_tile + 1)
    assert first["w64"][1] % lim.gemm_tile == 0 and first["c1"][1] == 1 and first["c15"][1] == lim.gemm_tile - 1
    assert sum(first["r137"]) == lim.lds_max_order + 1 and sum(first["l136"]) == lim.lds_max_order
    assert sum(first["l33"]) == lim.wave_max_order + 1
    assert sum(first["v32x3"]) == sum(first["v32x5"]) == sum(first["v32c1"]) == lim.wave_max_order == sum(first["v31"]) + 1
    assert first["w8"][0] < lim.gemm_tile and first["w8"][1] == lim.lds_max_order and first["w40"][0] < lim.diag_block


@pytest.mark.parametrize("name,kind", [(name, "lu") for name in se.CASES] + [(name, "chol") for name in se.RESTATED_CHOLESKY])
def test_inputs_are_benign(hip, name, kind):
    """cond_1 <= COND_MAX, and the float64 restatement of the recurrence on host factors is within 1e-12 of the dense
    inverse in every block of every front, by the measure the GPU test uses."""
    case = se.matrix(name, 0, kind == "chol")
    n = case[1]
    A = ref.dense(n, case[2], case[3], case[4])
    Zref, cond = ref.dense_inverse(n, case[2], case[3], case[4])
    assert cond <= ref.COND_MAX, cond
    if kind == "chol":
        assert np.array_equal(A, A.T)
    else:
        assert np.abs(A - A.T).max() > 0.1
    with se.analysed(name, kind) as F:
        Lh, Uh = ref.host_factors(F, A, cholesky=kind == "chol")
        Z = ref.restated_inverse(hip, F, Lh, Uh)
        Lp, Li, _, Up, Ui, _ = F.factors(values=False)
        Zl = ref.entries_of(Z, n, Lp, Li)
        Zu = ref.entries_of(Z, n, Up, Ui) if kind == "lu" else None
        blocks = ref.front_block_errors(hip, F, Zl, Zu, Zref)
        nfronts = int(F.info.nsuper)
    print("%s %s: cond_1 %.3g, restatement: worst block %s" % (name, kind, cond, ref.worst_block(blocks)))
    # every front has its PP block, every front below a root its CP block (and PC for LU)
    assert len({s for s, _, _, b, _ in blocks if b == "PP"}) == nfronts
    assert {b for _, _, _, b, _ in blocks} == ({"PP", "CP", "PC"} if kind == "lu" else {"PP", "CP"})
    assert sum(b == "CP" for _, _, _, b, _ in blocks) == sum(r > w for _, r, w, b, _ in blocks if b == "PP")
    assert all(err <= RESTATEMENT_BOUND for _, _, _, _, err in blocks), ref.worst_block(blocks)


def test_block_measure_names_the_block():
    """front_block_errors on a doctored Z: an error in one entry shows in its block alone, relative to that block's largest
    entry, and a NaN counts as inf."""
    from csparse3_amd import csc_hip as hip
    name = "l33f"
    case = se.matrix(name)
    n = case[1]
    Zref, _ = ref.dense_inverse(n, case[2], case[3], case[4])
    with se.analysed(name) as F:
        q = F.ordering()["q"]
        Zp = Zref[np.ix_(q, q)]
        Lp, Li, _, Up, Ui, _ = F.factors(values=False)
        sn_ptr, _, _, st = ref.fronts(hip, F)
        Zl, Zu = ref.entries_of(Zp, n, Lp, Li), ref.entries_of(Zp, n, Up, Ui)
        assert all(err == 0.0 for _, _, _, _, err in ref.front_block_errors(hip, F, Zl, Zu, Zref))
        s = next(s for s in range(len(st)) if len(st[s]) == se.WV + 1)          # a front (33, 16)
        w = int(sn_ptr[s + 1] - sn_ptr[s])
        j = int(sn_ptr[s + 1]) - 1                                             # the last pivot: its column of L is the front's
        col = np.arange(Lp[j], Lp[j + 1])
        p = int(col[Li[col] == st[s][-1]][0])                                  # Z(last update row, last pivot): in Z_CP
        cp_max = np.abs(Zp[np.ix_(st[s][w:], st[s][:w])]).max()
        bad = Zl.copy()
        bad[p] += 1e-9 * cp_max
        blocks = ref.front_block_errors(hip, F, bad, Zu, Zref)
        wrong = [(t, b) for t, _, _, b, err in blocks if err > 0.0]
        assert wrong == [(s, "CP")]
        err = [e for t, _, _, b, e in blocks if (t, b) == (s, "CP")][0]
        assert abs(err - 1e-9) <= 1e-12
        assert 1e-9 * cp_max < ref.BOUND * np.abs(Zref).max()                  # the measure over all entries would let it pass
        bad = Zu.copy()
        bad[int(Up[j + 1]) - 1] = np.nan                                       # U(j, j): in Z_PP
        blocks = ref.front_block_errors(hip, F, Zl, bad, Zref)
        assert [(t, b) for t, _, _, b, err in blocks if err > 0.0] == [(s, "PP")]
        assert [e for t, _, _, b, e in blocks if (t, b) == (s, "PP")] == [np.inf]
