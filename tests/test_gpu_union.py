"""Union plans on the GPU: the embedding kernel bit for bit against the NumPy restatement (tests/union_ref.py) at the
edges of its launch shape (sizes from cs3_union_limits), and csparse3_amd.streams.UnionBatch end to end on the family that
tests/test_union_cpu.py checks with the oracle."""
import gc

import numpy as np
import pytest

import helpers
import union_cases as cases
import union_ref as ref

pytestmark = pytest.mark.gpu


def embed_three_ways(hip, n, patterns, vals, want=None):
    """values_dev into a NaN-filled buffer and values(), both against the restatement.  -> the plan's info."""
    import torch
    if want is None:
        want = ref.embed(n, patterns, vals)
    dev = torch.device("cuda:0")
    cat = np.concatenate([np.asarray(v, dtype=np.float64) for v in vals] + [np.empty(0)])
    with hip.UnionPlan(n, patterns) as plan:
        assert want.shape == (plan.nmat, plan.nnz)
        d_cat = torch.from_numpy(cat.copy()).to(dev)
        d_out = torch.full((plan.nmat * plan.nnz + 1,), float("nan"), dtype=torch.float64, device=dev)
        plan.values_dev(d_cat.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.isnan(got[-1])                                             # nothing written past the end
        assert np.array_equal(ref.bits(got[:-1]), ref.bits(want)), "values_dev differs from the restatement"
        assert np.array_equal(ref.bits(plan.values(vals)), ref.bits(want)), "values differs from values_dev"
        assert np.array_equal(ref.bits(plan.values(cat)), ref.bits(want))
        return plan.info


@pytest.fixture(scope="module")
def lim(gpu):
    lim = gpu.union_limits()
    return int(lim.block * lim.entries_per_lane), int(lim.grid_cap)


@pytest.mark.parametrize("which", ["1", "B-1", "B", "B+1", "GB", "GB+1"])
def test_sizes_at_the_block_and_grid_edges(gpu, lim, which):
    B, G = lim
    total = {"1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "GB": G * B, "GB+1": G * B + 1}[which]
    n, patterns, vals = cases.diagonal_family(total, np.random.default_rng(total % 1000))
    inf = embed_three_ways(gpu, n, patterns, vals)
    assert inf.nmat * inf.nnz_union == total


def test_odd_union_puts_member_boundaries_at_odd_indices(gpu):
    n, patterns, vals = cases.banded_odd_family(np.random.default_rng(1))
    inf = embed_three_ways(gpu, n, patterns, vals)
    assert inf.nnz_union % 2 == 1 and inf.nmat == 3 and inf.padded > 0


def test_an_output_that_is_only_8_byte_aligned(gpu):
    import torch
    n, patterns, vals = cases.banded_odd_family(np.random.default_rng(2))
    want = ref.embed(n, patterns, vals)
    dev = torch.device("cuda:0")
    with gpu.UnionPlan(n, patterns) as plan:
        d_cat = torch.from_numpy(np.concatenate(vals)).to(dev)
        d_out = torch.full((want.size + 2,), float("nan"), dtype=torch.float64, device=dev)
        assert d_out.data_ptr() % 16 == 0
        plan.values_dev(d_cat.data_ptr(), d_out.data_ptr() + 8, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.isnan(got[0]) and np.isnan(got[-1])
        assert np.array_equal(ref.bits(got[1:-1]), ref.bits(want))
        with pytest.raises(gpu.Cs3Error) as e:
            plan.values_dev(d_cat.data_ptr(), d_out.data_ptr() + 4)
        assert e.value.code == gpu.CS3_ERR_ARG


def test_a_member_equal_to_the_union_and_an_empty_member(gpu):
    n, patterns = cases.structural_cases()["empty_member"]
    Up, Ui, key = ref.union_pattern(n, patterns)
    patterns = [(Up, Ui)] + list(patterns)
    vals = cases.values_for(np.random.default_rng(4), patterns)
    want = ref.embed_loop(n, patterns, vals)
    assert np.array_equal(ref.bits(want[0]), ref.bits(vals[0]))             # the union itself: a plain copy
    assert not want[2].any() and not np.signbit(want[2]).any()              # the empty member: a row of +0.0
    embed_three_ways(gpu, n, patterns, vals, want)


def test_special_values_are_copied_bit_for_bit(gpu):
    n, patterns = cases.structural_cases()["disjoint"]
    special = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF4000000ABCDEF,
                        0xFFF8000000000123, 0x0000000000000001, 0x800FFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    vals = [special[:4].copy(), np.concatenate([special[4:], special[:2]])]
    assert [len(v) for v in vals] == [int(Ap[-1]) for Ap, Ai in patterns]
    want = ref.embed_loop(n, patterns, vals)
    assert set(ref.bits(want)) >= set(ref.bits(special))
    embed_three_ways(gpu, n, patterns, vals, want)


def test_duplicates_are_added_left_to_right_starting_from_the_first(gpu):
    cs = cases.structural_cases()
    n, patterns = cs["dup5"]
    vals = [np.array([5.0, 1e16, 7.0, 1.0, -1e16, 9.0, 0.0, 0.0, -0.0, 0.0]), np.array([-0.0, 0.0])]
    want = ref.embed_loop(n, patterns, vals)
    Up, Ui, key = ref.union_pattern(n, patterns)
    s = int(ref.slots(n, key, *patterns[0])[1])
    assert want[0, s] == 0.0                                                # ((1e16 + 1) - 1e16) + 0 + 0; any other order: 1
    assert want[1, s] == 0.0 and not np.signbit(want[1, s])                 # -0.0 + +0.0 = +0.0
    assert embed_three_ways(gpu, n, patterns, vals, want).dup_slots == 3
    n, patterns = cs["dup2"]
    vals = [np.array([1e16, 3.0, 1.0, 4.0]), np.array([2.0, -0.0])]
    want = ref.embed_loop(n, patterns, vals)
    embed_three_ways(gpu, n, patterns, vals, want)
    three = cases._csc(2, [(0, [1, 1, 1])])                                 # exactly the triple of the header's example
    want = ref.embed_loop(2, [three], [np.array([1e16, 1.0, -1e16])])
    assert want.tolist() == [[0.0]]
    embed_three_ways(gpu, 2, [three], [np.array([1e16, 1.0, -1e16])], want)


@pytest.mark.parametrize("name", ["unsorted", "many_over_three_patterns", "six_members_three_identical", "n1", "column_empty_everywhere"])
def test_structural_cases(gpu, name):
    n, patterns = cases.structural_cases()[name]
    vals = cases.values_for(np.random.default_rng(9), patterns)
    inf = embed_three_ways(gpu, n, patterns, vals, ref.embed_loop(n, patterns, vals))
    if name == "many_over_three_patterns":
        assert inf.nmat == 130 and inf.distinct_patterns == 3


def test_capture_in_a_graph_and_replay_with_new_values(gpu):
    import torch
    n, patterns, vals = cases.contingency_family()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    with gpu.UnionPlan(n, patterns) as plan:
        plan.upload()                                                       # the tables go up before the capture
        d_cat = torch.from_numpy(np.concatenate(vals)).to(dev)
        d_out = torch.full((plan.nmat, plan.nnz), float("nan"), dtype=torch.float64, device=dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            plan.values_dev(d_cat.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            new = cases.values_for(rng, patterns)
            d_cat.copy_(torch.from_numpy(np.concatenate(new)))
            d_out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(ref.bits(d_out.cpu().numpy()), ref.bits(ref.embed(n, patterns, new)))
        del graph


# ---- end to end ------------------------------------------------------------------------------------------------------

def _own_solutions(hip, n, patterns, vals, rhs, kind, tol):
    out = []
    for (Ap, Ai), Ax, b in zip(patterns, vals, rhs):
        with hip.Factorization(n, n, Ap, Ai, kind=kind) as F:
            out.append(F.factor(Ax, tol).solve(b))
    return np.stack(out)


@pytest.fixture(scope="module")
def families():
    """(kind, members, k) -> (n, patterns, values, right-hand sides, own-pattern solutions): built once, shared, read-only."""
    return {}


def _family(families, hip, kind, members, k):
    key = (kind, members, k)
    if key not in families:
        n, patterns, vals = cases.contingency_family(members=members, symmetric_values=kind == hip.CS3_CHOLESKY)
        shape = (members, n) if k == 1 else (members, n, k)
        rhs = np.random.default_rng(40 + k).standard_normal(shape)
        own = _own_solutions(hip, n, patterns, vals, rhs, kind, 1e-3)
        own.setflags(write=False)
        families[key] = (n, patterns, vals, rhs, own)
    return families[key]


@pytest.mark.parametrize("kind_name,members,k", [("lu", 9, 1), ("lu", 9, 3), ("chol", 9, 1), ("chol", 9, 3), ("lu", 130, 1), ("lu", 130, 3),
                                                 ("chol", 130, 1), ("chol", 130, 3)])
def test_union_batch_against_the_plain_batched_handle_and_own_patterns(gpu, families, kind_name, members, k):
    import torch
    from csparse3_amd.streams import UnionBatch
    kind = gpu.CS3_LU if kind_name == "lu" else gpu.CS3_CHOLESKY
    n, patterns, vals, rhs, own = _family(families, gpu, kind, members, k)
    dev = torch.device("cuda:0")
    padded = ref.embed(n, patterns, vals)
    Up, Ui, key = ref.union_pattern(n, patterns)
    with UnionBatch([(n, n, Ap, Ai) for Ap, Ai in patterns], kind=kind) as U:
        assert U.factorization.batch == members and U.nnz == len(key)
        x = torch.from_numpy(rhs.copy()).to(dev)
        U.factor_solve([torch.from_numpy(v).to(dev) for v in vals], x, 1e-3)          # a list of per-member tensors
        U.status()
        got = x.cpu().numpy()
        assert np.array_equal(ref.bits(U.union_values.cpu().numpy()), ref.bits(padded))
        x2 = torch.from_numpy(rhs.copy()).to(dev)
        U.factor_solve(torch.from_numpy(np.concatenate(vals)).to(dev), x2, 1e-3)       # one concatenated tensor
        U.status()
        assert torch.equal(x, x2)
    with gpu.Factorization(n, n, Up, Ui, kind=kind, batch=members) as F:
        d_ax = torch.from_numpy(padded).to(dev)
        xp = torch.from_numpy(rhs.copy()).to(dev)
        F.factor_solve_dev(d_ax.data_ptr(), xp.data_ptr(), k, 1e-3, torch.cuda.current_stream().cuda_stream)
        F.factor_status(torch.cuda.current_stream().cuda_stream)
        plain = xp.cpu().numpy()
    assert np.array_equal(ref.bits(got), ref.bits(plain)), "UnionBatch differs from the batched handle on host-padded values"
    worst = max(helpers.rel_err(got[c], own[c]) for c in range(members))
    print("%s, %d members, k = %d: worst relative difference to the own-pattern handles %.2e" % (kind_name, members, k, worst))
    assert worst <= helpers.RTOL


def test_union_batch_with_matching(gpu, families):
    import torch
    from csparse3_amd.streams import UnionBatch
    n, patterns, vals, rhs, own = _family(families, gpu, gpu.CS3_LU, 9, 1)
    dev = torch.device("cuda:0")
    padded = ref.embed(n, patterns, vals)
    Up, Ui, key = ref.union_pattern(n, patterns)
    with UnionBatch([(n, n, Ap, Ai) for Ap, Ai in patterns], match_values=(3, vals[3])) as U:
        assert U.factorization.matched
        x = torch.from_numpy(rhs.copy()).to(dev)
        U.factor_solve(torch.from_numpy(np.concatenate(vals)).to(dev), x, 1e-3)
        U.status()
        got = x.cpu().numpy()
    with gpu.Factorization(n, n, Up, Ui, batch=9, match_values=padded[3]) as F:
        plain = F.factor(padded, 1e-3).solve(rhs.reshape(9, n, 1)).reshape(9, n)
    assert np.array_equal(ref.bits(got), ref.bits(plain))
    assert max(helpers.rel_err(got[c], own[c]) for c in range(9)) <= helpers.RTOL


def test_a_singular_member_is_reported_at_its_own_index(gpu, families):
    import torch
    from csparse3_amd.streams import UnionBatch
    n, patterns, vals, rhs, own = _family(families, gpu, gpu.CS3_LU, 9, 1)
    dev = torch.device("cuda:0")
    bad, row = 4, 77
    vals = [v.copy() for v in vals]
    vals[bad][patterns[bad][1] == row] = 0.0                                # an islanded bus: its whole row is zero
    with UnionBatch([(n, n, Ap, Ai) for Ap, Ai in patterns]) as U:
        x = torch.from_numpy(rhs.copy()).to(dev)
        U.factor_solve(torch.from_numpy(np.concatenate(vals)).to(dev), x, 0.0)
        with pytest.raises(gpu.SingularMatrix):                             # one status word per batch: the whole call fails
            U.status()
        U.factorization.set_perturbation(1e-8)
        x = torch.from_numpy(rhs.copy()).to(dev)
        U.factor_solve(torch.from_numpy(np.concatenate(vals)).to(dev), x, 0.0)
        U.status()
        count = U.factorization.perturbed(torch.cuda.current_stream().cuda_stream)
        assert count[bad] >= 1 and not np.delete(count, bad).any()
        got = x.cpu().numpy()
    ok = [c for c in range(9) if c != bad]
    # the others are not disturbed (tol 0 here, so their own-pattern solutions are taken again)
    own0 =_own_solutions(gpu, n, [patterns[c] for c in ok], [vals[c] for c in ok], [rhs[c] for c in ok], gpu.CS3_LU, 0.0)
    assert max(helpers.rel_err(got[c], own0[i]) for i, c in enumerate(ok)) <= helpers.RTOL


def test_a_freed_plan_leaves_no_device_block(gpu):
    import torch
    from csparse3_amd.streams import UnionBatch
    gc.collect()
    start = gpu.debug_live_device_buffers()
    n, patterns, vals = cases.contingency_family()
    with gpu.UnionPlan(n, patterns) as plan:
        plan.values(vals)
        assert gpu.debug_live_device_buffers() == start + 5                 # the five tables; the value buffers of values() are gone
    assert gpu.debug_live_device_buffers() == start
    U = UnionBatch([(n, n, Ap, Ai) for Ap, Ai in patterns])
    x = torch.zeros((9, n), dtype=torch.float64, device="cuda:0")
    U.factor_solve(torch.from_numpy(np.concatenate(vals)).to("cuda:0"), x, 1e-3)
    U.status()
    assert gpu.debug_live_device_buffers() > start + 5
    U.close()
    assert gpu.debug_live_device_buffers() == start
