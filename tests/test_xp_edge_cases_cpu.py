"""What the CPU can say about the edge cases of the extra-precise refinement (tests/xp_edge_cases.py): the batched
restatement xp_ref.refine_xp_all equals xp_ref.refine_xp bit for bit, a column does not feel its neighbours, every case
meets the conditions it is there for with SuperLU as the inner solver (one matrix and one column at a time), and the sizes
derived from the library's limits land where intended.  tests/test_gpu_refine_xp_edges.py re-asserts the conditions from
the trace of the handle's own solves."""
import numpy as np
import pytest

import xp_cases as xc
import xp_edge_cases as xe
import xp_ref


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def lim():
    return xe.limits()


def _run(case, inp, max_iters=10):
    return xp_ref.refine_xp_all(xe.cpu_solve_all(case, inp["AX0"]), case.n, case.Ap, case.Ai, inp["AX"], inp["B"], inp["X0"],
                                max_iters, case.trans)


@pytest.fixture(scope="module")
def planted(lim):
    """Every planted case through the restatement with SuperLU, once: name -> (spec, case, inputs, result)."""
    B, G, M = lim
    made = {}

    def get(name):
        if name not in made:
            spec = xe.specs(B, G, M)[name]
            case = xe.spec_case(spec)
            assert case.trans == spec.trans
            _, AX0 = xe.batch_values(case, spec.batch)
            inp = xe.planted_inputs(case, spec.k, spec.batch, xe.cpu_solve_all(case, AX0), B, M)
            made[name] = (spec, case, inp, _run(case, inp, spec.max_iters))
        return made[name]

    return get


# ---- the restatement --------------------------------------------------------------------------------------------------

def test_batched_restatement_equals_the_single_one_in_every_bit():
    for name, case in xc.refinement_cases().items():
        solve = xc.superlu_solver(case)
        x0 = solve(case.b)
        one = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, case.b, x0, 10, case.trans)
        many = xp_ref.refine_xp_all(lambda R: solve(R.reshape(-1)).reshape(R.shape), case.n, case.Ap, case.Ai, case.Ax[None, :],
                                    case.b.reshape(1, -1, 1), x0.reshape(1, -1, 1), 10, case.trans)
        assert _same_bits(one["x"], many["x"].reshape(-1)) and _same_bits(one["xt"], many["xt"].reshape(-1)), name
        assert one["iters"] == many["iters"][0] and one["flag"] == many["flag"][0], name
        for key in ("rate", "ferr", "berr", "nd_prev"):
            assert _same_bits(one[key], many[key]), (name, key)
        assert len(many["trace"]) == one["iters"] + (one["flag"] in (2, 3)), name


def test_a_column_does_not_depend_on_its_neighbours(lim):
    B, G, M = lim
    case, AX, AX0 = xe.mixed_values(3)
    solve_all = xe.cpu_solve_all(case, AX0)
    inp = xe.mixed_inputs(11, 3, solve_all)
    whole = xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, AX, inp["B"], inp["X0"])
    for t in range(11):
        alone = xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, AX, inp["B"][:, :, t:t + 1], inp["X0"][:, :, t:t + 1])
        assert _same_bits(alone["x"][:, :, 0], whole["x"][:, :, t]) and _same_bits(alone["xt"][:, :, 0], whole["xt"][:, :, t])
        for key in ("rate", "ferr", "berr"):
            assert _same_bits(alone[key], whole[key].reshape(3, 11)[:, t]), key
        for key in ("iters", "flag"):
            assert np.array_equal(alone[key], whole[key].reshape(3, 11)[:, t]), key
    assert len(set(len(xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, AX, inp["B"][:, :, t:t + 1],
                                            inp["X0"][:, :, t:t + 1])["trace"]) for t in range(5))) >= 3


# ---- the sizes --------------------------------------------------------------------------------------------------------

def test_sizes_land_where_intended(lim):
    B, G, M = lim
    S = xe.specs(B, G, M)
    shape = {name: xe.shapes(xe.base_case(s.base).n * s.reps, s.k, s.batch, B, G, M) for name, s in S.items()}
    n = 45
    want = {1: (1, B, 0, 1), 2: (2, B // 2, 0, 1), 3: (3, B // 3, B - 3 * (B // 3), 1), 85: (85, B // 85, B - 85 * (B // 85), 1),
            86: (86, B // 86, B - 86 * (B // 86), 1), 128: (128, B // 128, B - 128 * (B // 128), 1),
            129: (129, B // 129, B - 129 * (B // 129), 1), 255: (255, B // 255, B - 255 * (B // 255), 1), B: (B, 1, 0, 1),
            B + 1: (B, 1, 0, 2), 2 * B + 1: (B, 1, 0, 3)}
    for k in xe.column_tile_ks(B):
        sh = shape[xe.tile_name(k, B)]
        assert (sh["w"], sh["rows"], sh["dead"], sh["tiles"]) == want[k], k
        assert sh["maxima_grid"] == (min(-(-n // sh["rows"]), M), 1, sh["tiles"]) and not sh["maxima_strides"]
        assert not sh["update_strides"]
    if B == 256:                                                  # the k of the list are edges of THIS block size
        assert [shape[xe.tile_name(k, B)]["dead"] for k in (3, 85, 86, 129, 255)] == [1, 1, 84, 127, 1]
        assert [shape[xe.tile_name(k, B)]["rows"] for k in (85, 86, 128, 129)] == [3, 2, 2, 1]
    for k in (B + 1, 2 * B + 1):                                  # ragged: one column in the last tile
        assert shape[xe.tile_name(k, B)]["last_tile_cols"] == 1
    assert shape["a_n1"]["maxima_grid"] == (1, 1, 2) and shape["a_n1"]["last_tile_cols"] == 1
    # b: rows == 1 and the first order above M: the row loop strides, for the rows M .. n - 1 alone
    for name in ("b_k129", "b_kB1", "c_trans"):
        s, sh = S[name], shape[name]
        nb = 32 * s.reps
        assert sh["rows"] == 1 and M < nb <= M + 32 and sh["maxima_strides"] and sh["maxima_grid"][0] == M
        assert not sh["update_strides"]
    assert shape["b_k129"]["tiles"] == 1 and shape["b_kB1"]["tiles"] == 2
    sh = shape["b_k5"]                                            # the last row class of a tall tile has rows, one dead lane
    assert sh["rows"] == B // 5 and 1 < sh["rows"] <= 32 * S["b_k5"].reps and sh["maxima_grid"][0] > 1 and not sh["maxima_strides"]
    assert sh["rows"] - 1 in xe.plan_rows(32 * S["b_k5"].reps, 5, B, M)[1]
    # c: past the cap of the residual and update kernels, the second grid pass partial, its last workgroup too
    s, sh = S["c_plain"], shape["c_plain"]
    nk = 32 * s.reps * s.k
    assert s.k == B + 1 and G * B + B < nk < 2 * G * B and sh["update_strides"] and sh["update_partial_second_pass"]
    assert sh["update_grid"] == (G, 1) and sh["maxima_strides"] and sh["tiles"] == 2
    if (B, G) == (256, 4096):
        assert s.reps == 129 and nk == 1060896
    # d: a second workgroup of k_xp_control
    D = xe.mixed_specs(B)
    main = D["d_main"]
    assert xe.shapes(32, main.k, main.batch, B, G, M)["control_groups"] == 2 and main.batch * main.k > B + main.k
    assert all(sh["control_groups"] == 1 for name, sh in shape.items() if not name.startswith("c_") and S[name].k <= B)
    assert shape["e_trans"]["update_grid"][1] == 2 and S["e_trans"].k > 16 and S["e_matched_k3"].k < 16


def test_planted_rows_cover_every_lane_class(lim):
    B, G, M = lim
    for name, s in xe.specs(B, G, M).items():
        n = xe.base_case(s.base).n * s.reps
        if n == 1:
            continue
        ix, idr = xe.plan_rows(n, s.k, B, M)
        xe.check_planted_rows_cover(n, s.k, B, M, ix[None, :], idr[None, :])
        assert ((0 <= ix) & (ix < n) & (0 <= idr) & (idr < n)).all()
    # the very last element of case c carries a maximum
    s = xe.specs(B, G, M)["c_plain"]
    ix, idr = xe.plan_rows(32 * s.reps, s.k, B, M)
    assert ix[s.k - 1] == 32 * s.reps - 1 or idr[s.k - 1] == 32 * s.reps - 1


# ---- the conditions of every case, with SuperLU -----------------------------------------------------------------------

def _planted_names():
    return sorted(xe.specs(256, 4096, 1024))                      # (the names do not depend on the limits)


@pytest.mark.parametrize("name", _planted_names())
def test_planted_case_meets_its_conditions(planted, lim, name):
    B, G, M = lim
    spec, case, inp, out = planted(name)
    assert out["x"].shape == (spec.batch, case.n, spec.k)
    if case.n == 1:
        assert set(out["flag"].tolist()) == {1}
        return
    xe.check_planted_rows_cover(case.n, spec.k, B, M, inp["ix"], inp["id"])
    rx, rd = xe.check_planted(out, inp["ix"], inp["id"])
    print("%-16s n %d k %d passes %d ratios x %.3g dx %.3g iters %s flags %s" % (
        name, case.n, spec.k, len(out["trace"]), rx, rd, sorted(set(out["iters"].tolist())), sorted(set(out["flag"].tolist()))))
    assert rd >= 11.0
    assert set(out["flag"].tolist()) == {1} and 2 <= out["iters"].min() and out["iters"].max() <= 9
    assert len(out["trace"]) >= 2                                # more than one pass: the maxima words are used twice


def test_mixed_cases_meet_their_conditions(lim):
    B, G, M = lim
    for name, spec in xe.mixed_specs(B).items():
        case, AX, AX0 = xe.mixed_values(spec.batch)
        solve_all = xe.cpu_solve_all(case, AX0)
        inp = xe.mixed_inputs(spec.k, spec.batch, solve_all)
        out = xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, AX, inp["B"], inp["X0"])
        xe.check_mixed(out, spec.batch, spec.k, B)
        print(name, "passes", len(out["trace"]), "flags", sorted(set(out["flag"].tolist())), "iters of the converged",
              sorted(set(out["iters"][out["flag"] == 1].tolist())))
        if spec.batch == 3 and spec.k >= len(xe.KINDS):
            kinds = inp["kinds"].reshape(-1)
            assert (out["flag"][kinds >= 3] == 3).all() and (out["iters"][kinds >= 3] == 0).all()
            assert (out["flag"].reshape(3, -1)[1][inp["kinds"][1] < 2] == 2).all()          # the hopeless matrix stalls
            branches = set()
            for mi in (0, 1, 2):
                cut = xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, AX, inp["B"], inp["X0"], mi)
                assert len(cut["trace"]) == mi
                assert xe.ferr_branches(cut) == {0: {"no_iters"}, 1: {"nan", "zero", "bound"}, 2: {"nan", "rate", "zero", "bound"}}[mi]
                branches |= xe.ferr_branches(cut)
                if mi:
                    assert 0 in set(cut["flag"].tolist())
                else:
                    assert set(cut["flag"].tolist()) == {0} and _same_bits(cut["x"], inp["X0"])
            assert branches | xe.ferr_branches(out) == {"nan", "no_iters", "rate", "zero", "bound"}
