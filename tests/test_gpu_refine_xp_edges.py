"""The extra-precise refinement (csrc/refine_xp.hip, refine_xp_run in api.cpp) at tile, grid, batch and state edges, on the
cases of tests/xp_edge_cases.py: the column tiles of k_xp_maxima (dead lanes, rows == 1, a second and a ragged third
blockIdx.z tile), its strided row loop, the second grid pass of the residual and update kernels inside a refinement, the
second workgroup of k_xp_control with converged, stalled, non-finite and iterating systems in one call, batches with
k > 1, Cholesky, matched and transposed handles above one right-hand side, and work memory reused by a smaller call.

The reference is xp_ref.refine_xp_all driven by the handle's OWN solve, F.solve(R, trans) on the whole [batch, n, k]
array: it and the correction inside refine_xp_run are the same run_solve(h, res, k, 0, stream, trans), so every pass is
reproduced bit for bit and x, xt, rate, ferr and berr are compared as raw 64-bit patterns, iters and flag for equality:
there is no tolerance in this file.  The inputs are made with the handle's own solve too, and every case re-asserts from
the trace of its own run the conditions it is there for (tests/test_xp_edge_cases_cpu.py proves the same plan with
SuperLU, without a device)."""
import numpy as np
import pytest

import xp_edge_cases as xe
import xp_ref

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(x, info, out, what):
    """The device's result against the restatement's: every bit of x, xt, rate, ferr, berr; iters and flag equal."""
    for key in ("iters", "flag"):
        got, want = np.asarray(info[key]), out[key]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %s differs in %d systems, first %d: %d, restated %d" % (
            what, key, bad.size, bad[0], got[bad[0]], want[bad[0]])
    for key, got, want in (("x", x, out["x"]), ("xt", info["xt"], out["xt"]), ("rate", info["rate"], out["rate"]),
                           ("ferr", info["ferr"], out["ferr"]), ("berr", info["berr"], out["berr"])):
        got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %s differs in %d of %d entries, first at %d: %016x, restated %016x" % (
            what, key, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def lim(gpu):
    return xe.limits()


@pytest.fixture(scope="module")
def held(gpu):
    """One factorised handle per (matrix, batch, values), shared by the tests of this module."""
    made = {}

    def get(key, case, AX0):
        if key not in made:
            kind = gpu.CS3_CHOLESKY if case.kind == "chol" else gpu.CS3_LU
            F = gpu.Factorization(case.n, case.n, case.Ap, case.Ai, kind=kind, order=gpu.ORDER_NATURAL, batch=AX0.shape[0],
                                  match_values=case.Ax if case.kind == "matched" else None)
            F.factor(np.ascontiguousarray(AX0))
            made[key] = F
        return made[key]

    yield get
    for F in made.values():
        F.close()


def _planted_handle(held, spec):
    case = xe.spec_case(spec)
    _, AX0 = xe.batch_values(case, spec.batch)
    return case, held((spec.base, spec.reps, spec.batch), case, AX0)


def _refine_both(F, case, inp, max_iters):
    solve_all = lambda R: F.solve(R, trans=case.trans)
    x, info = F.refine_xp(inp["AX"], inp["B"], x=inp["X0"], max_iters=max_iters, trans=case.trans, want_tail=True)
    out = xp_ref.refine_xp_all(solve_all, case.n, case.Ap, case.Ai, inp["AX"], inp["B"], inp["X0"], max_iters, case.trans)
    return x, info, out


@pytest.fixture(scope="module")
def planted(held, lim):
    """name -> (spec, case, F, inputs): the planted inputs of a case, made once with the handle's own solve."""
    B, G, M = lim
    made = {}

    def get(name):
        if name not in made:
            spec = xe.specs(B, G, M)[name]
            case, F = _planted_handle(held, spec)
            inp = xe.planted_inputs(case, spec.k, spec.batch, lambda R: F.solve(R, trans=case.trans), B, M)
            made[name] = (spec, case, F, inp)
        return made[name]

    return get


def _run_planted(planted, lim, name, max_iters=None):
    B, G, M = lim
    spec, case, F, inp = planted(name)
    x, info, out = _refine_both(F, case, inp, spec.max_iters if max_iters is None else max_iters)
    if case.n > 1:                                                # the conditions first: a failure below then means the kernels
        xe.check_planted_rows_cover(case.n, spec.k, B, M, inp["ix"], inp["id"])
        rx, rd = xe.check_planted(out, inp["ix"], inp["id"])
        print("%-15s n %d k %d batch %d passes %d: planted ratios x %.3g dx %.3g, iters %s" % (
            name, case.n, spec.k, spec.batch, len(out["trace"]), rx, rd, sorted(set(out["iters"].tolist()))))
    _assert_same(x, info, out, name)
    return spec, case, out


# ---- the premise ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a_k3", "a_k129"])
def test_one_pass_is_the_handles_own_solve(planted, lim, name):
    """max_iters = 1: residual, ONE correction, maxima, control, update.  F.solve gives the in-loop correction's bits."""
    spec, case, out = _run_planted(planted, lim, name, max_iters=1)
    assert len(out["trace"]) == 1 and out["trace"][0]["apply"].all() and set(out["flag"].tolist()) == {0}
    assert np.isfinite(out["ferr"]).all() and out["xt"].any()


# ---- a. column tiles --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [xe.tile_name(k, 256) for k in xe.column_tile_ks(256)])
def test_column_tiles(planted, lim, name):
    spec, case, out = _run_planted(planted, lim, name)
    assert set(out["flag"].tolist()) == {1} and len(out["trace"]) >= 2


def test_last_row_class_of_a_tall_tile(planted, lim):
    """k = 5 on n = 1056: rows = B / 5 row classes, and max |dx| of one column sits in row rows - 1."""
    B, G, M = lim
    spec, case, out = _run_planted(planted, lim, "b_k5")
    assert B // 5 - 1 in out["trace"][0]["row_d"][0] and set(out["flag"].tolist()) == {1}


def test_order_one_with_a_ragged_second_tile(planted, lim):
    spec, case, out = _run_planted(planted, lim, "a_n1")
    assert case.n == 1 and spec.k == lim[0] + 1 and set(out["flag"].tolist()) == {1}


# ---- b. the row stride of the maxima ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["b_k129", "b_kB1"])
def test_maxima_row_stride(planted, lim, name):
    B, G, M = lim
    spec, case, out = _run_planted(planted, lim, name)
    sh = xe.shapes(case.n, spec.k, spec.batch, B, G, M)
    assert sh["rows"] == 1 and sh["maxima_strides"]
    first = out["trace"][0]
    assert (first["row_d"] >= M).sum() >= 2 and (first["row_x"] >= M).sum() >= 1 and first["row_x"][0, spec.k - 1] == case.n - 1
    assert set(out["flag"].tolist()) == {1}


# ---- c. past the grid cap inside a refinement -------------------------------------------------------------------------

def test_past_the_grid_cap(planted, lim):
    B, G, M = lim
    spec, case, out = _run_planted(planted, lim, "c_plain")
    assert G * B + B < case.n * spec.k < 2 * G * B
    assert out["trace"][0]["row_x"][0, spec.k - 1] == case.n - 1 and out["trace"][0]["apply"].all()
    assert set(out["flag"].tolist()) == {1}


def test_transposed_on_the_strided_matrix(planted, lim):
    spec, case, out = _run_planted(planted, lim, "c_trans")
    assert case.trans and set(out["flag"].tolist()) == {1}


# ---- d. many systems, mixed states ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(held, lim):
    """name -> (spec, case, F, inputs) of the mixed-state cases."""
    made = {}

    def get(name):
        if name not in made:
            spec = xe.mixed_specs(lim[0])[name]
            case, AX, AX0 = xe.mixed_values(spec.batch)
            F = held(("mixed", spec.batch), case, AX0)
            made[name] = (spec, case, F, xe.mixed_inputs(spec.k, spec.batch, F.solve))
        return made[name]

    return get


@pytest.mark.parametrize("name", ["d_main", "d_b2_k3", "d_b3_k1"])
def test_mixed_states_in_one_call(mixed, lim, name):
    spec, case, F, inp = mixed(name)
    x, info, out = _refine_both(F, case, inp, 10)
    xe.check_mixed(out, spec.batch, spec.k, lim[0])
    print("%s: nsys %d passes %d flags %s iters of the converged %s" % (
        name, spec.batch * spec.k, len(out["trace"]), sorted(set(out["flag"].tolist())),
        sorted(set(out["iters"][out["flag"] == 1].tolist()))))
    _assert_same(x, info, out, name)
    if name == "d_main":
        assert spec.batch * spec.k > lim[0]
        kinds = inp["kinds"].reshape(-1)
        assert (out["flag"][kinds >= 3] == 3).all()
        # the columns of a system that never applied hold their input bits
        never = np.broadcast_to((out["iters"] == 0).reshape(spec.batch, 1, spec.k), x.shape)
        assert never.any() and np.array_equal(_bits(x)[never], _bits(inp["X0"])[never])


@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_mixed_states_cut_short(mixed, lim, max_iters):
    spec, case, F, inp = mixed("d_main")
    x, info, out = _refine_both(F, case, inp, max_iters)
    assert len(out["trace"]) == max_iters and 0 in set(out["flag"].tolist())
    want = {0: {"no_iters"}, 1: {"nan", "zero", "bound"}, 2: {"nan", "rate", "zero", "bound"}}[max_iters]
    assert xe.ferr_branches(out) == want, xe.ferr_branches(out)
    _assert_same(x, info, out, "d_main, max_iters %d" % max_iters)


# ---- e. handle kinds --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["e_spd", "e_matched_k3", "e_matched_k129", "e_trans"])
def test_handle_kinds(planted, lim, name):
    spec, case, out = _run_planted(planted, lim, name)
    assert set(out["flag"].tolist()) == {1}
    assert {"e_spd": case.kind == "chol", "e_matched_k3": case.kind == "matched", "e_matched_k129": case.kind == "matched",
            "e_trans": case.trans and spec.batch == 2}[name]


# ---- f. reused work memory --------------------------------------------------------------------------------------------

def test_a_smaller_call_after_a_larger_one(gpu, planted, lim):
    B, G, M = lim
    names = ["a_k2B1", "a_k3", "a_k129"]
    case = xe.spec_case(xe.specs(B, G, M)[names[0]])
    results = {}
    with gpu.Factorization(case.n, case.n, case.Ap, case.Ai, order=gpu.ORDER_NATURAL) as F:
        F.factor(case.Ax0)
        for name in names:                                        # the inputs of the shared handle: the same factors, the same bits
            spec, _, _, inp = planted(name)
            x, info, out = _refine_both(F, case, inp, 10)
            _assert_same(x, info, out, "%s on the reused handle" % name)
            results[name] = (x, info)
        allocs0, _ = F.debug_alloc_counters()
        spec, _, _, inp = planted("a_k129")
        x, info, _ = _refine_both(F, case, inp, 10)
        assert F.debug_alloc_counters()[0] == allocs0
        assert np.array_equal(_bits(x), _bits(results["a_k129"][0]))
    with gpu.Factorization(case.n, case.n, case.Ap, case.Ai, order=gpu.ORDER_NATURAL) as fresh:
        fresh.factor(case.Ax0)
        spec, _, _, inp = planted("a_k3")
        x, info = fresh.refine_xp(inp["AX"], inp["B"], x=inp["X0"], want_tail=True)
    old_x, old = results["a_k3"]
    assert np.array_equal(_bits(x), _bits(old_x))
    for key in ("xt", "rate", "ferr", "berr"):
        assert np.array_equal(_bits(info[key]), _bits(old[key])), key
    for key in ("iters", "flag"):
        assert np.array_equal(info[key], old[key]), key
