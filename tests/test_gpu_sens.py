"""Sparse right-hand sides (cs3_sens_*) on the GPU: Y = C op(A)^-1 B against the SciPy restatement (tests/sens_ref.py,
within helpers.RTOL), from both sides, plain and transposed; the tile, width and block edges taken from cs3_sens_limits;
the bit-exact hand-over between the handle's solves and the two kernels around them; structure (empty, duplicated,
unsorted, long columns, identity operands); NaN containment; the no-allocation contract; refactorisations."""
import numpy as np
import pytest

from helpers import RTOL, csc_to_scipy, rel_err
import sens_cases as sc
import sens_ref as sr
from sens_ref import Op

pytestmark = pytest.mark.gpu

SIDES = ("right", "left", "auto")
_YREF = {}


def _solve(F, B, Ct, side="auto", trans=False):
    """-> (Y, info) through the host-array form."""
    with F.sens_plan(None if B is None else B[:3], None if Ct is None else Ct[:3], side=side, trans=trans) as plan:
        Y = F.sens_solve(plan, None if B is None else B.values, None if Ct is None else Ct.values)
        return Y, plan.info


def _solve_dev(F, plan, B, Ct, stream=None):
    """-> Y through the device form on `stream` (synchronises afterwards)."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda op: None if op is None else torch.from_numpy(np.array(op.values, dtype=np.float64)).to(dev)    # noqa: E731
    d_b, d_c = up(B), up(Ct)
    d_y = torch.full((plan.p, plan.k), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    F.sens_solve_dev(plan, 0 if d_b is None else d_b.data_ptr(), 0 if d_c is None else d_c.data_ptr(), d_y.data_ptr(), st.cuda_stream)
    counters = F.debug_alloc_counters()
    torch.cuda.synchronize()
    return d_y.cpu().numpy(), counters


def _factored(gpu, name):
    F, factor = sc.handle(gpu, name)
    factor(F)
    return F


def _dense_solve(F, rhs, trans):
    """solve_dev on a dense [n, w] block -> the solutions, the bits the plan's own solve of that tile must produce."""
    import torch
    d_x = torch.from_numpy(np.ascontiguousarray(rhs)).to("cuda:0")
    F.solve_dev(d_x.data_ptr(), rhs.shape[1], torch.cuda.current_stream().cuda_stream, trans=trans)
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


def _padded(op, n, width):
    D = np.zeros((n, width))
    D[:, :op.ncols] = sr.dense(op, n)
    return D


# 1. parity
@pytest.mark.parametrize("name", list(sc.MATRICES))
def test_parity_with_the_reference_from_both_sides(gpu, name):
    A = sc.matrix(name)[6]
    B, Ct = sc.default_operands(name)
    with _factored(gpu, name) as F:
        for trans in (False, True):
            want = sr.y_right(A, B, Ct, trans)
            for side in SIDES:
                Y, info = _solve(F, B, Ct, side, trans)
                err = rel_err(Y, want)
                print("%s side=%s (%d) trans=%s: relative error %.2e" % (name, side, info.side, trans, err))
                assert info.side == sr.choose_side(B.ncols, Ct.ncols, sr.SIDES[side])
                assert Y.shape == (Ct.ncols, B.ncols) and err <= RTOL, (name, side, trans, err)


# 2. tile and width edges on jacobian_like (n = 200)
def _edge_reference(kmax, pmax):
    if (kmax, pmax) not in _YREF:
        n, A = sc.matrix("jacobian_like")[1], sc.matrix("jacobian_like")[6]
        B, Ct = sc.incidence(n, kmax, seed=21), sc.incidence(n, pmax, seed=23)
        _YREF[(kmax, pmax)] = (B, Ct, sr.y_right(A, B, Ct))
    return _YREF[(kmax, pmax)]


def _prefix(op, c):
    e = int(op.indptr[c])
    return Op(c, op.indptr[:c + 1], op.indices[:e], op.values[:e])


@pytest.mark.parametrize("side", ["right", "left"])
def test_tile_edges_at_a_tile_width_of_16(gpu, monkeypatch, side):
    monkeypatch.setenv("CS3_SENS_TILE", "16")
    edges = (1, 15, 16, 17, 31, 32, 33)
    B, Ct, want = _edge_reference(33, 33)
    lim = gpu.sens_limits()
    worst = 0.0
    with _factored(gpu, "jacobian_like") as F:
        for k in edges:
            for p in edges:
                Y, info = _solve(F, _prefix(B, k), _prefix(Ct, p), side)
                tl = sr.tiles(k if side == "right" else p, lim, 16)
                assert info.ntiles == len(tl) and info.max_width == 16
                err = rel_err(Y, want[:p, :k])
                worst = max(worst, err)
                assert err <= RTOL, (side, k, p, err)
    print("tile 16, side %s: worst relative error %.2e" % (side, worst))


@pytest.mark.parametrize("side", ["right", "left"])
def test_tile_edges_at_the_default_width(gpu, monkeypatch, side):
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    B, Ct, want = _edge_reference(1025, 1025)
    lim = gpu.sens_limits()
    with _factored(gpu, "jacobian_like") as F:
        for c in (1023, 1024, 1025):
            k, p = (c, 7) if side == "right" else (7, c)
            Y, info = _solve(F, _prefix(B, k), _prefix(Ct, p), side)
            tl = sr.tiles(c, lim)
            assert (info.ntiles, info.max_width) == (len(tl), max(w for _, _, w in tl))
            err = rel_err(Y, want[:p, :k])
            print("default width, side %s, %d columns in %d tiles: relative error %.2e" % (side, c, info.ntiles, err))
            assert err <= RTOL, (side, c, err)


# 3. bit-exact hand-over
@pytest.mark.parametrize("name, cols", [("jacobian_like", 5), ("jacobian_like", 40), ("grid5000", 40), ("grid5000", 300),
                                        ("kkt400", 40), ("spd900", 40)])
def test_hand_over_is_bit_exact_on_both_sides(gpu, monkeypatch, name, cols):
    """A selection with unit values on the combining side: Y must be the selected rows of what solve_dev gives for the
    densified tile at the plan's solve width -- the scatter wrote exactly that tile, the combine moved its bits."""
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    n = sc.matrix(name)[1]
    op = sc.incidence(n, cols, seed=31)
    pick = np.random.default_rng(37).choice(n, size=min(n, 50), replace=False)
    sel = sc.selection(pick)
    with _factored(gpu, name) as F:
        for trans in (False, True):
            Y, info = _solve(F, op, sel, "right", trans)                       # C = selection of rows
            assert info.ntiles == 1 and info.max_width == max(cols, gpu.sens_limits().pad_width)
            X = _dense_solve(F, _padded(op, n, info.max_width), trans)
            assert np.array_equal(Y, X[pick, :cols]), (name, cols, trans, "right")
            Y, info = _solve(F, sel, op, "left", trans)                        # B = selection of columns, C' = op
            assert info.ntiles == 1
            Z = _dense_solve(F, _padded(op, n, info.max_width), not trans)
            assert np.array_equal(Y, Z[pick, :cols].T), (name, cols, trans, "left")


# 4. structure
def test_empty_columns_and_rows_give_exact_zeros(gpu):
    n, A = sc.matrix("jacobian_like")[1], sc.matrix("jacobian_like")[6]
    B = sc.from_columns([([], []), ([3, 40], [1.0, -1.0]), ([], []), ([7], [0.5]), ([], [])])
    Ct = sc.from_columns([([9], [2.0]), ([], []), ([11, 5], [1.0, 1.0]), ([], [])])
    allempty = sc.from_columns([([], [])] * 3)
    with _factored(gpu, "jacobian_like") as F:
        for side in ("right", "left"):
            Y, _ = _solve(F, B, Ct, side)
            assert rel_err(Y, sr.y_right(A, B, Ct)) <= RTOL
            assert not Y[:, [0, 2, 4]].any() and not Y[[1, 3], :].any()
            assert Y[np.ix_([0, 2], [1, 3])].all()
            assert not _solve(F, allempty, Ct, side)[0].any() and not _solve(F, B, allempty, side)[0].any()


def test_duplicates_add_and_unsorted_rows(gpu):
    n, A = sc.matrix("jacobian_like")[1], sc.matrix("jacobian_like")[6]
    rows, vals = sc.long_column(n, 9, seed=41)
    order = np.argsort(rows)
    B_dup = sc.from_columns([([5, 9, 5, 5], [0.25, 1.0, 0.5, -0.125]), (rows, vals), ([3], [2.0])])
    B_sum = sc.from_columns([([9, 5], [1.0, 0.625]), (rows[order], vals[order]), ([3], [2.0])])
    # (0.5 T + 0.5 T and 2 T - T are exact, so the summed entry must give the same bits)
    C_dup = sc.from_columns([([8, 8], [0.5, 0.5]), ([4, 60, 4], [2.0, 0.75, -1.0]), (rows, vals)])
    C_sum = sc.from_columns([([8], [1.0]), ([60, 4], [0.75, 1.0]), (rows, vals)])
    with _factored(gpu, "jacobian_like") as F:
        for side in ("right", "left"):
            Y, _ = _solve(F, B_dup, C_dup, side)
            assert rel_err(Y, sr.y_right(A, B_dup, C_dup)) <= RTOL
            # on the solved-for side duplicates and order vanish in the tile: every row is bit-exact; on the combining side
            # the exactly summed duplicates are
            Ys, _ = _solve(F, B_sum, C_dup, side) if side == "right" else _solve(F, B_dup, C_sum, side)
            assert np.array_equal(Ys, Y), side
            Yo, _ = _solve(F, B_dup, C_sum, side) if side == "right" else _solve(F, B_sum, C_dup, side)
            assert np.array_equal(Yo[:1], Y[:1]) if side == "right" else np.array_equal(Yo[:, 2:], Y[:, 2:])
            assert rel_err(Yo, Y) <= RTOL


@pytest.mark.parametrize("count", [63, 64, 65, 200])
def test_long_columns_and_rows(gpu, count):
    n, A = sc.matrix("jacobian_like")[1], sc.matrix("jacobian_like")[6]
    B = sc.from_columns([([2], [1.0]), sc.long_column(n, count, seed=count), ([4, 6], [1.0, -1.0])])
    Ct = sc.from_columns([sc.long_column(n, count, seed=count + 1), ([0], [1.0])])
    want = sr.y_right(A, B, Ct)
    with _factored(gpu, "jacobian_like") as F:
        for side in ("right", "left"):
            assert rel_err(_solve(F, B, Ct, side)[0], want) <= RTOL, (count, side)


def _grid137():
    from csparse3_amd import synth
    m, n, Ap, Ai, Ax = synth.jacobian_like(nbus=80, nedges=120, n_pv=21, seed=137)
    assert n == 137
    return m, n, Ap, Ai, Ax, csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()


def test_identity_operands(gpu):
    m, n, Ap, Ai, Ax, A = _grid137()
    Ct = sc.incidence(n, 9, seed=43)
    B = sc.incidence(n, 11, seed=47)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax, 1e-3)
        for trans in (False, True):
            Y, info = _solve(F, None, Ct, "auto", trans)                       # rows of op(A)^-1, forced left
            assert info.side == sr.LEFT and Y.shape == (9, n)
            assert rel_err(Y, sr.y_left(A, None, Ct, trans)) <= RTOL
            Y, info = _solve(F, B, None, "auto", trans)                        # the plain solution, forced right
            assert info.side == sr.RIGHT and Y.shape == (n, 11)
            assert rel_err(Y, sr.y_right(A, B, None, trans)) <= RTOL
            assert np.array_equal(Y, _dense_solve(F, _padded(B, n, info.max_width), trans)[:, :11])
        pick = [5, 136, 0]
        Y, _ = _solve(F, None, sc.selection(pick))                             # selected rows of A^-1
        assert rel_err(Y, np.linalg.inv(A.toarray())[pick, :]) <= RTOL


def test_single_row_and_single_column(gpu):
    n, A = sc.matrix("jacobian_like")[1], sc.matrix("jacobian_like")[6]
    one, many = sc.incidence(n, 1, seed=53), sc.incidence(n, 70, seed=59)
    with _factored(gpu, "jacobian_like") as F:
        for B, Ct in ((one, many), (many, one), (one, one)):
            want = sr.y_right(A, B, Ct)
            for side in SIDES:
                assert rel_err(_solve(F, B, Ct, side)[0], want) <= RTOL, (B.ncols, Ct.ncols, side)


def test_output_blocks_around_the_block_edges(gpu, monkeypatch):
    """The combining kernel's blocks: combine_cols (= the transposing block edge) columns of the other operand by
    combine_lanes tile columns -- one short of, equal to and one past each, on both sides."""
    monkeypatch.delenv("CS3_SENS_TILE", raising=False)
    lim = gpu.sens_limits()
    assert lim.tblock == lim.combine_cols
    across = [lim.tblock + d for d in (-1, 0, 1)]
    along = [lim.combine_lanes + d for d in (-1, 0, 1)]
    B, Ct, want = _edge_reference(1025, 1025)
    with _factored(gpu, "jacobian_like") as F:
        for g in across:
            for j in along:
                Y, _ = _solve(F, _prefix(B, j), _prefix(Ct, g), "right")       # tile columns of B, rows of C across
                assert rel_err(Y, want[:g, :j]) <= RTOL, ("right", g, j)
                Y, _ = _solve(F, _prefix(B, g), _prefix(Ct, j), "left")        # tile columns = rows of C, columns of B across
                assert rel_err(Y, want[:j, :g]) <= RTOL, ("left", g, j)


# 5. NaN containment
@pytest.mark.parametrize("side", ["right", "left"])
def test_a_nan_value_stays_in_its_column_or_row(gpu, side):
    n = sc.matrix("jacobian_like")[1]
    B, Ct = sc.incidence(n, 20, seed=61), sc.incidence(n, 12, seed=67)
    with _factored(gpu, "jacobian_like") as F:
        Y0, _ = _solve(F, B, Ct, side)
        assert np.isfinite(Y0).all()
        bad = B._replace(values=B.values.copy())
        bad.values[B.indptr[7]] = np.nan
        Y, _ = _solve(F, bad, Ct, side)
        others = np.arange(20) != 7
        assert not np.isfinite(Y[:, 7]).any() and np.array_equal(Y[:, others], Y0[:, others]), "NaN in B, side " + side
        bad = Ct._replace(values=Ct.values.copy())
        bad.values[Ct.indptr[3]] = np.nan
        Y, _ = _solve(F, B, bad, side)
        others = np.arange(12) != 3
        assert not np.isfinite(Y[3, :]).any() and np.array_equal(Y[others, :], Y0[others, :]), "NaN in C, side " + side


# 6. the device form, the no-allocation contract, run to run
@pytest.mark.parametrize("side", ["right", "left"])
def test_dev_form_equals_the_host_form_and_later_calls_do_not_allocate(gpu, monkeypatch, side):
    import torch
    monkeypatch.setenv("CS3_SENS_TILE", "16")
    n = sc.matrix("jacobian_like")[1]
    B, Ct = sc.incidence(n, 40, seed=71), sc.incidence(n, 37, seed=73)
    with _factored(gpu, "jacobian_like") as F:
        with F.sens_plan(B[:3], Ct[:3], side=side) as plan:
            assert plan.info.ntiles == 3
            Y = F.sens_solve(plan, B.values, Ct.values)
            assert np.array_equal(F.sens_solve(plan, B.values, Ct.values), Y), "two runs of one call differ"
            other = torch.cuda.Stream()
            before = F.debug_alloc_counters()
            for stream in (None, other, other):
                Yd, after = _solve_dev(F, plan, B, Ct, stream)
                assert np.array_equal(Yd, Y)
                assert after == before, "a later call allocated or synchronised: %r -> %r" % (before, after)
        with F.sens_plan(None, Ct[:3]) as plan:                                # an identity operand: its value pointer is ignored
            Y = F.sens_solve(plan, None, Ct.values)
            assert np.array_equal(_solve_dev(F, plan, None, Ct)[0], Y)


# 7. refactorisations
def test_a_plan_survives_refactorisations(gpu):
    m, n, Ap, Ai, Ax, kind, A = sc.matrix("jacobian_like")
    B, Ct = sc.default_operands("jacobian_like")
    rng = np.random.default_rng(79)
    with gpu.Factorization(m, n, Ap, Ai) as F:
        with F.sens_plan(B[:3], Ct[:3], side="right") as right, F.sens_plan(B[:3], Ct[:3], side="left", trans=True) as left:
            for step in range(3):
                Ax2 = Ax if step == 0 else Ax * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=len(Ax)))
                A2 = csc_to_scipy(m, n, Ap, Ai, Ax2).tocsc()
                F.factor(Ax2, 1e-3)
                Y = F.sens_solve(right, B.values, Ct.values)
                assert rel_err(Y, sr.y_right(A2, B, Ct)) <= RTOL, step
                Yt = F.sens_solve(left, B.values, Ct.values)
                assert rel_err(Yt, sr.y_right(A2, B, Ct, trans=True)) <= RTOL, step
                if step:
                    assert rel_err(Y, first) > 1e-4, "Y did not follow the new values"
                else:
                    first = Y


# 8. the one-call form
def test_cscmat_sensitivities(gpu):
    from csparse3_amd.csc import CscMat
    m, n, Ap, Ai, Ax, kind, A = sc.matrix("jacobian_like")
    B, Ct = sc.default_operands("jacobian_like")
    Bs = sr.to_scipy(B, n)
    Cs = sr.to_scipy(Ct, n).T.tocsc()                                          # C in its natural orientation, p x n
    Bm = CscMat(n, B.ncols, indptr=Bs.indptr.astype(np.int32), indices=Bs.indices.astype(np.int32), data=Bs.data)
    Cm = CscMat(Ct.ncols, n, indptr=Cs.indptr.astype(np.int32), indices=Cs.indices.astype(np.int32), data=Cs.data)
    M = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    for trans in (False, True):
        want = sr.y_right(A, B, Ct, trans)
        for side in SIDES:
            assert rel_err(M.sensitivities(Bm, Cm, tol=1e-3, trans=trans, side=side), want) <= RTOL
    assert rel_err(M.sensitivities(Bm, tol=1e-3), sr.y_right(A, B, None)) <= RTOL
