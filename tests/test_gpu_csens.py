"""Complex sparse right-hand sides (cs3_cplx_sens_*) on the GPU.

Bit for bit against the NumPy restatement (tests/csens_ref.py) driven by the handle's own solve_dev: the scatter alone
(parts = 1, the tile read back), the combine alone (parts = 4 on a tile the test wrote), the full call, for every (side,
op), both identity operands, host and device forms; the lane-map, workgroup and tile edges; accuracy against dense NumPy
complex128; NaN containment, refactorisation, the no-allocation contract.

"Bit for bit" is equality of the 64-bit words; where both sides hold a NaN its sign and payload are not compared.

The structural patterns and the diag_zoo matrix cannot be factorised (an empty column, NaN diagonals).  The C ABI takes the
complex plan and the handle separately, so for them the plan of the pattern -- its s, from its values -- runs on the handle
of a banded matrix of the same order: the kernels read that s, and the bits are those the restatement gives with it."""
import numpy as np
import pytest

import cplx_ref as ref
import csens_cases as cc
import csens_ref as cr
import sens_ref as sr

pytestmark = pytest.mark.gpu

OPS = {"N": ref.N, "T": ref.T, "H": ref.H}
SIDES = {"right": sr.RIGHT, "left": sr.LEFT}
MATS = cc.matrices()


def _args(op):
    return None if op is None else (op.ncols, op.indptr, op.indices)


def _vals(op):
    return None if op is None else op.values


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def handle_solve(F):
    """solve(T [2n, w], trans): the real handle's solve_dev at the tile's width, the bits the plan's own solve gives."""
    import torch

    def solve(Tl, trans):
        d = torch.from_numpy(np.ascontiguousarray(Tl)).to("cuda:0")
        F.real.solve_dev(d.data_ptr(), Tl.shape[1], _stream(), trans=trans)
        torch.cuda.synchronize()
        return d.cpu().numpy()
    return solve


class Case:
    """A factorised handle, the plan whose s the kernels read, and that s restated."""

    def __init__(self, gpu, name):
        n, Ap, Ai, Az, kind, rotate = MATS[name]
        self.n, self.name, self.own = n, name, None
        self.real_thing = name in ("ybus40", "hermitian_pd")
        if self.real_thing:
            self.A = ref.dense_complex(n, Ap, Ai, Az)
            self.F = gpu.ComplexFactorization(n, Ap, Ai, kind=gpu.CS3_CHOLESKY if kind == "chol" else gpu.CS3_LU, rotate=rotate).factor(Az)
        else:
            bn, bAp, bAi, bAz = cc.banded(n, seed=n)
            self.F = gpu.ComplexFactorization(bn, bAp, bAi).factor(bAz)
            self.own, self.F.plan = self.F.plan, gpu.ComplexPlan(n, Ap, Ai, rotate=rotate)
            self.F.plan.values(Az)
        Azr, Azi = ref.split(Az, (1, -1))
        sr_, si_ = ref.rotation(n, Ap, Ai, Azr, Azi, rotate)
        self.sr, self.si = sr_[0], si_[0]
        assert cr.same(self.F.plan.rotation()[0], ref.join(self.sr, self.si))
        self.solve = handle_solve(self.F)

    def close(self):
        self.F.close()
        if self.own is not None:
            self.own.close()


@pytest.fixture(scope="module")
def made(gpu):
    cases = {}

    def get(name):
        if name not in cases:
            cases[name] = Case(gpu, name)
        return cases[name]
    yield get
    for c in cases.values():
        c.close()


def restated(c, B, Ct, side, op, lim, tile_env=None, parts=7, tile_in=None):
    ns = (c.n if B is None else B.ncols) if side == sr.RIGHT else (c.n if Ct is None else Ct.ncols)
    return cr.y_restated(c.n, B, Ct, side, op, c.sr, c.si, sr.tiles(ns, lim, tile_env), c.solve, parts, tile_in)


def dev_call(c, plan, B, Ct, parts=None):
    """The device form (or the debug call with `parts`) into a Y with a NaN guard behind it.  -> (Y, guard intact)."""
    import torch
    up = lambda op: None if op is None else torch.from_numpy(np.ascontiguousarray(op.values, dtype=np.complex128)).to("cuda:0")    # noqa: E731
    d_b, d_c = up(B), up(Ct)
    count = plan.p * plan.k
    d_y = torch.full((count + 2,), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda:0")
    pb, pc = (0 if d_b is None else d_b.data_ptr()), (0 if d_c is None else d_c.data_ptr())
    if parts is None:
        c.F.sens_solve_dev(plan, pb, pc, d_y.data_ptr(), _stream())
    else:
        c.F.debug_sens_parts(plan, parts, pb, pc, d_y.data_ptr(), _stream())
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    return y[:count].reshape(plan.p, plan.k), bool(np.isnan(y[count:]).all())


def check_full(c, B, Ct, side, opname, lim, tile_env=None, device=True):
    with c.F.sens_plan(_args(B), _args(Ct), side=side, trans=opname) as plan:
        got = c.F.sens_solve(plan, _vals(B), _vals(Ct))
        want, _ = restated(c, B, Ct, plan.info.side, OPS[opname], lim, tile_env)
        assert cr.same(got, want), (c.name, side, opname, tile_env, "host form")
        if device:
            got_d, intact = dev_call(c, plan, B, Ct)
            assert intact and cr.same(got_d, want), (c.name, side, opname, tile_env, "device form")
    return got


# ---- every (side, op), both identities, host and device forms ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MATS))
@pytest.mark.parametrize("opname", ["N", "T", "H"])
def test_the_full_call_bit_for_bit(gpu, made, monkeypatch, name, opname):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c, lim = made(name), gpu.cplx_sens_limits()
    n = c.n
    B, Ct = cc.incidence(n, 9, 5), cc.incidence(n, 7, 6)
    for side in ("right", "left"):
        check_full(c, B, Ct, side, opname, lim)
        check_full(c, cc.awkward(n, 3), cc.selection([n - 1, 0, n - 1]), side, opname, lim)
        check_full(c, cc.selection([0, n - 1]), cc.awkward(n, 4), side, opname, lim)
    check_full(c, None, Ct, "auto", opname, lim)                                      # B = I: side left, the identity combines
    check_full(c, B, None, "auto", opname, lim)                                       # C = I: side right
    check_full(c, cc.awkward(n, 3), None, "right", opname, lim)


@pytest.mark.parametrize("name", ["ybus40", "diag_zoo", "absent_diagonal"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_scatter_alone_and_combine_alone(gpu, made, monkeypatch, name, side):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c, lim = made(name), gpu.cplx_sens_limits()
    n = c.n
    rng = np.random.default_rng(17)
    for opname, op in OPS.items():
        inner, conj = cr.glue(SIDES[side], op)
        for B, Ct in ((cc.awkward(n, 3), cc.incidence(n, 20, 6)), (cc.incidence(n, 20, 5), cc.awkward(n, 4)),
                      (None, cc.awkward(n, 4)) if side == "left" else (cc.awkward(n, 3), None)):
            solved = B if side == "right" else Ct
            other = Ct if side == "right" else B
            with c.F.sens_plan(_args(B), _args(Ct), side=side, trans=opname) as plan:
                inf = plan.info
                assert inf.ntiles == 1 and inf.side == SIDES[side]
                t, w = solved.ncols, int(inf.max_width)
                # parts = 1: the tile as the scatter left it
                dev_call(c, plan, B, Ct, parts=1)
                got_t = c.F.real.debug_sens_tile((2 * n, w))
                assert cr.same(got_t, cr.scatter(n, w, solved, 0, t, inner, conj, c.sr, c.si)), (name, side, opname, "scatter")
                # parts = 4: the combine on a tile of the test's
                tile = rng.standard_normal((2 * n, w))
                tile.reshape(-1)[::7] = -0.0
                c.F.real.debug_sens_tile((2 * n, w), write=tile)
                got_y, intact = dev_call(c, plan, B, Ct, parts=4)
                want_y, _ = restated(c, B, Ct, SIDES[side], op, lim, parts=4, tile_in=lambda c0, ww: tile)
                assert intact and cr.same(got_y, want_y), (name, side, opname, "combine", other is None)


def test_an_identity_operand_hands_the_unpacked_solution_over(gpu, made, monkeypatch):
    """An identity operand forces the other side, so through a plan it is always the COMBINING operand: the combine then
    is cs3_cplx_unpack_dev (and the table's conjugation) on the tile, nothing else."""
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c, lim = made("diag_zoo"), gpu.cplx_sens_limits()
    n = c.n
    Ct = cc.incidence(n, 6, 9)
    rng = np.random.default_rng(3)
    for opname, op in OPS.items():
        with c.F.sens_plan(None, _args(Ct), trans=opname) as plan:
            w = int(plan.info.max_width)
            dev_call(c, plan, None, Ct, parts=1)                                      # (makes the tile buffer)
            tile = rng.standard_normal((2 * n, w))
            c.F.real.debug_sens_tile((2 * n, w), write=tile)
            got, intact = dev_call(c, plan, None, Ct, parts=4)
            inner, conj = cr.glue(sr.LEFT, op)
            yr, yi = cr.unpacked(tile, inner, conj, c.sr, c.si)
            assert intact and cr.same(got, ref.join(yr, yi)[:, :6].T), opname


# ---- edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["right", "left"])
def test_lane_map_edges(gpu, made, monkeypatch, side):
    """Solved-for columns 1, 15, 16, 17, 63, 64, 65 against 31, 32, 33 columns of the other operand."""
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c, lim = made("ybus40"), gpu.cplx_sens_limits()
    big, small = cc.incidence(c.n, 65, 21), cc.incidence(c.n, 33, 23)
    for i, t in enumerate((1, 15, 16, 17, 63, 64, 65)):
        for g in (31, 32, 33):
            solved, other = _prefix(big, t), _prefix(small, g)
            B, Ct = (solved, other) if side == "right" else (other, solved)
            check_full(c, B, Ct, side, ("N", "T", "H")[(i + g) % 3], lim, device=(g == 32))


def _prefix(op, ncols):
    e = int(op.indptr[ncols])
    return sr.Op(ncols, op.indptr[:ncols + 1], op.indices[:e], op.values[:e])


@pytest.mark.parametrize("n", [15, 16, 17, 33])
def test_scatter_workgroup_edges(gpu, n):
    """2n = 30, 32, 34 and 66 real rows against scatter workgroups of cs3_cplx_sens_limits().scatter_rows."""
    lim = gpu.cplx_sens_limits()
    assert lim.scatter_rows == 32
    _, Ap, Ai, Az = cc.banded(n, seed=n)
    Azr, Azi = ref.split(Az, (1, -1))
    sr_, si_ = ref.rotation(n, Ap, Ai, Azr, Azi, True)

    class C:
        pass
    c = C()
    with gpu.ComplexFactorization(n, Ap, Ai) as F:
        F.factor(Az)
        c.n, c.name, c.F, c.sr, c.si, c.solve = n, "banded%d" % n, F, sr_[0], si_[0], handle_solve(F)
        every_row = cc.cplx(sr.Op(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy(), np.ones(n)), n)
        for opname in OPS:
            check_full(c, every_row, cc.incidence(n, 5, 2), "right", opname, lim, device=False)
            check_full(c, cc.incidence(n, 5, 2), every_row, "left", opname, lim, device=False)
            check_full(c, None, cc.incidence(n, 5, 2), "auto", opname, lim, device=False)


@pytest.mark.parametrize("tile", ["5", "16"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_tiles_are_crossed(gpu, made, monkeypatch, tile, side):
    """17 solved-for columns: four tiles of 5, 5, 5, 2 (nothing padded below the pad width), or 16 and a last tile of 1
    padded to 16; 32: two full tiles of 16, the last not padded."""
    monkeypatch.setenv("CS3_SENS_TILE", tile)
    c, lim = made("ybus40"), gpu.cplx_sens_limits()
    for t in (17, 32):
        solved, other = cc.incidence(c.n, t, 31), cc.incidence(c.n, 33, 32)
        B, Ct = (solved, other) if side == "right" else (other, solved)
        for opname in OPS:
            with c.F.sens_plan(_args(B), _args(Ct), side=side, trans=opname) as plan:
                assert plan.info.ntiles == len(sr.tiles(t, lim, tile)) > 1
            check_full(c, B, Ct, side, opname, lim, tile_env=tile, device=(opname == "H"))


@pytest.mark.parametrize("side", ["right", "left"])
def test_a_scatter_thread_owns_two_columns(gpu, made, monkeypatch, side):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c, lim = made("ybus40"), gpu.cplx_sens_limits()
    t = int(lim.scatter_threads) + 44
    solved, other = cc.incidence(c.n, t, 41), cc.incidence(c.n, 33, 42)
    B, Ct = (solved, other) if side == "right" else (other, solved)
    check_full(c, B, Ct, side, "H" if side == "left" else "N", lim)


# ---- accuracy against the definition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ybus40", "hermitian_pd"])
def test_accuracy_against_dense_numpy(gpu, made, monkeypatch, name):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c = made(name)
    cond = float(np.linalg.cond(c.A))
    B, Ct = cc.incidence(c.n, 40, 51), cc.incidence(c.n, 24, 52)
    for opname, op in OPS.items():
        for Bo, Co, side in ((B, Ct, "right"), (B, Ct, "left"), (B, Ct, "auto"), (None, Ct, "auto"), (B, None, "auto")):
            with c.F.sens_plan(_args(Bo), _args(Co), side=side, trans=opname) as plan:
                Y = c.F.sens_solve(plan, _vals(Bo), _vals(Co))
            want = cr.y_dense(c.A, Bo, Co, op)
            err, bound = np.abs(Y - want).max(), 1e3 * cond * 2.0 ** -53 * np.abs(want).max()
            print("%s op %s side %s: max error %.3e, bound %.3e (cond %.2e)" % (name, opname, side, err, bound, cond))
            assert Y.shape == want.shape and err <= bound, (name, opname, side, err, bound)


# ---- propagation and reuse ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("opname", ["N", "H"])
def test_a_nan_value_stays_in_its_column_or_row(gpu, made, monkeypatch, side, opname):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    c = made("ybus40")
    B, Ct = cc.incidence(c.n, 20, 61), cc.incidence(c.n, 12, 67)
    with c.F.sens_plan(_args(B), _args(Ct), side=side, trans=opname) as plan:
        Y0 = c.F.sens_solve(plan, B.values, Ct.values)
        assert np.isfinite(Y0.view(np.float64)).all()
        bad = B.values.copy()
        bad[B.indptr[7]] = complex(np.nan, 1.0)
        Y = c.F.sens_solve(plan, bad, Ct.values)
        others = np.arange(20) != 7
        assert np.isnan(Y[:, 7]).all() and cr.same(Y[:, others], Y0[:, others]), "NaN in B"
        bad = Ct.values.copy()
        bad[Ct.indptr[3]] = complex(1.0, np.nan)
        Y = c.F.sens_solve(plan, B.values, bad)
        others = np.arange(12) != 3
        assert np.isnan(Y[3, :]).all() and cr.same(Y[others, :], Y0[others, :]), "NaN in C"


def test_a_plan_survives_a_refactorisation_and_reads_the_new_rotation(gpu, monkeypatch):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    n, Ap, Ai, Az = cc.ybus40()
    lim = gpu.cplx_sens_limits()
    B, Ct = cc.incidence(n, 30, 71), cc.incidence(n, 9, 72)
    rng = np.random.default_rng(73)
    Az2 = Az * (1.0 + 0.2 * rng.uniform(-1, 1, len(Az))) + 0.3 * rng.uniform(0, 1, len(Az))      # other phases on the diagonal
    with gpu.ComplexFactorization(n, Ap, Ai) as F, F.sens_plan(_args(B), _args(Ct), trans="H") as plan:
        seen = []
        for values in (Az, Az2, Az):
            F.factor(values)
            s = F.plan.rotation()[0]
            Y = F.sens_solve(plan, B.values, Ct.values)
            want, _ = cr.y_restated(n, B, Ct, plan.info.side, ref.H, s.real.copy(), s.imag.copy(),
                                    sr.tiles(Ct.ncols, lim), handle_solve(F))
            assert cr.same(Y, want)
            A = ref.dense_complex(n, Ap, Ai, values)
            ref_y = cr.y_dense(A, B, Ct, ref.H)
            assert np.abs(Y - ref_y).max() <= 1e3 * np.linalg.cond(A) * 2.0 ** -53 * np.abs(ref_y).max()
            seen.append((s, Y))
        assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1])
        assert cr.same(seen[0][1], seen[2][1])


def test_a_second_call_neither_allocates_nor_synchronises(gpu, made, monkeypatch):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    import torch
    c = made("ybus40")
    B, Ct = cc.incidence(c.n, 70, 81), cc.incidence(c.n, 33, 82)
    for side in ("right", "left"):
        with c.F.sens_plan(_args(B), _args(Ct), side=side, trans="T") as plan:
            first, _ = dev_call(c, plan, B, Ct)
            counters = c.F.real.debug_alloc_counters()
            d_b = torch.from_numpy(B.values).to("cuda:0")
            d_c = torch.from_numpy(Ct.values).to("cuda:0")
            d_y = torch.empty((plan.p, plan.k), dtype=torch.complex128, device="cuda:0")
            live = gpu.debug_live_device_buffers()
            c.F.sens_solve_dev(plan, d_b.data_ptr(), d_c.data_ptr(), d_y.data_ptr(), _stream())
            assert c.F.real.debug_alloc_counters() == counters, "a second call allocated or synchronised"
            assert gpu.debug_live_device_buffers() == live
            torch.cuda.synchronize()
            assert cr.same(d_y.cpu().numpy(), first)


def test_misaligned_arrays_and_a_plan_of_another_order_are_refused(gpu, made):
    import torch
    c = made("ybus40")
    B, Ct = cc.incidence(c.n, 4, 91), cc.incidence(c.n, 3, 92)
    buf = torch.zeros(256, dtype=torch.float64, device="cuda:0")
    p = buf.data_ptr()
    with c.F.sens_plan(_args(B), _args(Ct)) as plan:
        for args in ((p + 8, p + 512, p + 1024), (p, p + 520, p + 1024), (p, p + 512, p + 1032)):
            with pytest.raises(gpu.Cs3Error) as e:
                c.F.sens_solve_dev(plan, *args)
            assert e.value.code == gpu.CS3_ERR_ARG and "16 bytes" in str(e.value)
        with pytest.raises(gpu.Cs3Error) as e:
            c.F.debug_sens_parts(plan, 8, p, p + 512, p + 1024)
        assert "mask of 1, 2 and 4" in str(e.value)
        n2, Ap2, Ai2 = 2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
        with gpu.ComplexPlan(n2, Ap2, Ai2) as other:
            rc = gpu.lib().cs3_cplx_sens_solve_dev(other._p, c.F.real._h, plan._u, p, p + 512, p + 1024, None)
            assert rc == gpu.CS3_ERR_ARG and "another order" in gpu.lib().cs3_last_error().decode()
