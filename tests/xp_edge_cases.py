"""The extra-precise refinement at tile, grid, batch and state edges (tests/test_xp_edge_cases_cpu.py,
tests/test_gpu_refine_xp_edges.py): the cases, their launch shapes recomputed in Python, and the conditions each case is
there for.

Every size comes from refine_xp_limits(): B = block (threads per workgroup of the family), G = grid_cap (workgroups of the
residual and update kernels), M = maxima_grid_cap (workgroups over the rows of k_xp_maxima).

Matrices: block-diagonal copies of xc.chain(4, 8) and xc.chain(3, 15), copy c scaled by 1 + 0.01 noise_c (one factor per
copy: the conditioning of a copy is the chain's).  Planted systems: xtrue = uniform noise in [-1, 1] with a spike of 4 at
row ix, b = op(A) xtrue, x0 = solve(b) plus one correction solve(b - op(A) x0), with 2^-10 max |x0| added at row id != ix:
max |x| sits at ix and the first pass's max |dx| at id, both far above the runner-up of their column.  (The correction is
needed on chain(3, 15): with b = op(A) xtrue the error of solve(b) alone is cond eps max |x| = 3.5e-3 max |x|, the size
of the planted 2^-10, and the planted row led by 3.8 plain and by 1.3 transposed with SuperLU; after one correction it
leads by 100 or more.)  The inputs are made with the solver that is then refined
with (SuperLU here, the handle's own solve on the device), so the conditions are asserted from the trace of every run."""
from collections import namedtuple

import numpy as np

import xp_cases as xc
import xp_ref

Spec = namedtuple("Spec", "name base reps k batch trans max_iters mixed")
Spec.__new__.__defaults__ = (1, 1, 1, False, 10, False)

PLANT = 2.0 ** -10
SPIKE = 4.0
MIN_RATIO = 2.0


def limits():
    """(B, G, M) of the library (needs no device)."""
    from csparse3_amd import csc_hip
    lim = csc_hip.refine_xp_limits()
    return int(lim.block), int(lim.grid_cap), int(lim.maxima_grid_cap)


def base_case(name):
    if name == "chain_4_8":
        return xc.chain(4, 8)
    if name == "chain_3_15":
        return xc.chain(3, 15)
    if name == "chain_3_15_t":
        return xc.chain(3, 15, trans=True, name="chain_3_15_t")
    if name == "chain_4_8_t":
        return xc.chain(4, 8, trans=True, name="chain_4_8_t")
    if name == "chain_spd":
        return xc.chain_spd()
    if name == "permuted":
        return xc.permuted()
    if name == "n1":
        return xc.one_by_one()
    raise KeyError(name)


def tiled(base, reps, seed=21):
    """reps block-diagonal copies of `base` (built sparsely), the values of copy c scaled by 1 + 0.01 noise_c."""
    if reps == 1:
        return base
    assert base.kind == "lu"
    nnz = int(base.Ap[-1])
    Ap = np.concatenate([[0], (base.Ap[1:][None, :] + nnz * np.arange(reps)[:, None]).reshape(-1)]).astype(np.int32)
    Ai = (base.Ai[None, :nnz] + base.n * np.arange(reps)[:, None]).reshape(-1).astype(np.int32)
    scale = 1.0 + 0.01 * np.random.default_rng(seed).standard_normal(reps)
    Ax = (base.Ax[None, :nnz] * scale[:, None]).reshape(-1)
    n = reps * base.n
    return base._replace(name="%s_x%d" % (base.name, reps), n=n, Ap=Ap, Ai=Ai, Ax=Ax, Ax0=Ax, b=np.zeros(n))


def batch_values(case, batch, seed=22):
    """-> (AX, AX0) [batch, nnz]: matrix 0 the case's values, matrix m > 0 scaled by 1 + 0.01 noise_m."""
    scale = np.ones(batch)
    scale[1:] = 1.0 + 0.01 * np.random.default_rng(seed).standard_normal(batch - 1)
    return case.Ax[None, :] * scale[:, None], case.Ax0[None, :] * scale[:, None]


def shapes(n, k, batch, B, G, M):
    """The launches of one pass, recomputed: the tile of k_xp_maxima and the grids of the four kernels."""
    w = min(k, B)
    rows = B // w
    tiles = -(-k // w)
    last = k - (tiles - 1) * w                                   # columns of the last tile
    gx_max = min(-(-n // rows), M)
    gx_upd = min(-(-(n * k) // B), G)
    return dict(w=w, rows=rows, live=w * rows, dead=B - w * rows, tiles=tiles, last_tile_cols=last,
                maxima_grid=(gx_max, batch, tiles), maxima_strides=n > M * rows,
                update_grid=(gx_upd, batch), update_strides=n * k > G * B,
                update_partial_second_pass=G * B < n * k < 2 * G * B and (n * k - G * B) % B != 0,
                control_groups=-(-(batch * k) // B))


def special_rows(n, k, B, M):
    """Rows that only one lane class of k_xp_maxima sees, where they exist: the last row, row 0, the last row class of
    the tile (rows - 1), the first strided row (M * rows) and the last but one."""
    rows = B // min(k, B)
    out = []
    for r in (n - 1, 0, rows - 1, M * rows, n - 2, M * rows + rows - 1):
        if 0 <= r < n and r not in out:
            out.append(r)
    return out


def plan_rows(n, k, B, M):
    """-> (ix, id) [k]: the planted rows of max |x| and of the first max |dx| of every column.  Column 0 has id = n - 1,
    the last column id = 0 and ix = n - 1, the next columns take the special rows in turn (as id, and shifted by two as ix), the rest
    are spread with strides 7 and 11.  ix != id in every column; n >= 2."""
    assert n >= 2
    special = special_rows(n, k, B, M)
    ix, idr = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    for t in range(k):
        if t == 0:
            d = n - 1
        elif t == k - 1:
            d = 0
        elif t - 1 < len(special):
            d = special[t - 1]
        else:
            d = (3 + 7 * t) % n
        x = special[(t + 2) % len(special)] if t < 2 * len(special) else (5 + 11 * t) % n
        if t == k - 1 and k > 1:                                  # the very last element (n - 1, k - 1) carries max |x|
            x = n - 1
        if x == d:
            x = (x + 1) % n
        ix[t], idr[t] = x, d
    return ix, idr


def _op(case, Ax):
    import scipy.sparse as sp
    A = sp.csc_matrix((Ax, case.Ai, case.Ap), shape=(case.n, case.n))
    return A.T.tocsr() if case.trans else A.tocsr()


def planted_inputs(case, k, batch, solve_all, B_, M_, seed=23):
    """-> dict(AX, AX0, B, X0 [batch, n, k], ix, id [batch, k]).  The rows of matrix m are those of plan_rows rotated by
    m columns, so that every system of the call differs."""
    n = case.n
    AX, AX0 = batch_values(case, batch)
    rng = np.random.default_rng(seed + k)
    if n == 1:
        Bm = rng.uniform(1.0, 2.0, (batch, 1, k))
        return dict(AX=AX, AX0=AX0, B=Bm, X0=solve_all(Bm) * (1.0 + PLANT), ix=None, id=None)
    ix0, id0 = plan_rows(n, k, B_, M_)
    ix = np.stack([np.roll(ix0, m) for m in range(batch)])
    idr = np.stack([np.roll(id0, m) for m in range(batch)])
    Xtrue = rng.uniform(-1.0, 1.0, (batch, n, k))
    for m in range(batch):
        Xtrue[m, ix[m], np.arange(k)] = SPIKE
    Bm = np.stack([_op(case, AX[m]) @ Xtrue[m] for m in range(batch)])
    X0 = np.array(solve_all(Bm), dtype=np.float64).reshape(batch, n, k)
    R = np.stack([xp_ref.resid_xp(n, case.Ap, case.Ai, AX[m], Bm[m], X0[m], None, case.trans)[0] for m in range(batch)])
    X0 = X0 + np.asarray(solve_all(R), dtype=np.float64).reshape(batch, n, k)      # (one correction: see the module's text)
    for m in range(batch):
        X0[m, idr[m], np.arange(k)] += PLANT * np.abs(X0[m]).max(axis=0)
    return dict(AX=AX, AX0=AX0, B=Bm, X0=X0, ix=ix, id=idr)


KINDS = ("solve", "zero_x0", "zero_b", "nan_b", "inf_x0")


def mixed_kinds(batch, k):
    """[batch, k] indices into KINDS: the columns cycle through the five kinds, the very last system starts from 0."""
    kinds = np.tile(np.arange(k) % len(KINDS), (batch, 1))
    kinds[batch - 1, k - 1] = KINDS.index("zero_x0")
    return kinds


def mixed_values(batch):
    """Matrices 0 and 2 are chain(4, 8) (matrix 2 scaled by 1.01), matrix 1 is the hopeless pair on the same pattern:
    refined against its values, factorised from the noisy ones.  -> (case, AX, AX0)."""
    good, bad = xc.chain(4, 8), xc.hopeless_pair()
    assert np.array_equal(good.Ap, bad.Ap) and np.array_equal(good.Ai, bad.Ai)
    AX = np.stack([good.Ax, bad.Ax, good.Ax * 1.01][:batch])
    AX0 = np.stack([good.Ax0, bad.Ax0, good.Ax0 * 1.01][:batch])
    return good, AX, AX0


def mixed_inputs(k, batch, solve_all, seed=24):
    """Case d -> dict(AX, AX0, B, X0, kinds)."""
    case, AX, AX0 = mixed_values(batch)
    n = case.n
    kinds = mixed_kinds(batch, k)
    rng = np.random.default_rng(seed + k)
    Bm = rng.standard_normal((batch, n, k))
    Bm[kinds[:, None, :].repeat(n, axis=1) == KINDS.index("zero_b")] = 0.0
    X0 = np.array(solve_all(Bm), dtype=np.float64).reshape(batch, n, k)
    for m in range(batch):
        for t in range(k):
            kind = KINDS[kinds[m, t]]
            if kind in ("zero_x0", "zero_b"):
                X0[m, :, t] = 0.0
            elif kind == "nan_b":
                Bm[m, (3 * t + m) % n, t] = np.nan
            elif kind == "inf_x0":
                X0[m, (5 * t + m) % n, t] = np.inf if t % 2 else -np.inf
    return dict(AX=AX, AX0=AX0, B=Bm, X0=X0, kinds=kinds)


# ---- the conditions, asserted from a trace ----------------------------------------------------------------------------

def check_planted(out, ix, idr):
    """Pass 0 of the trace: every max |x| at its planted row, every max |dx| at its planted row, both at least
    MIN_RATIO times the runner-up of their column.  -> the smallest two ratios."""
    first = out["trace"][0]
    assert np.array_equal(first["row_x"], ix), "max |x| is not where it was planted"
    assert np.array_equal(first["row_d"], idr), "max |dx| of the first pass is not where it was planted"
    assert (first["ratio_x"] >= MIN_RATIO).all() and (first["ratio_d"] >= MIN_RATIO).all(), \
        (first["ratio_x"].min(), first["ratio_d"].min())
    return float(first["ratio_x"].min()), float(first["ratio_d"].min())


def check_planted_rows_cover(n, k, B, M, ix, idr):
    """What the plan promises: ix != id everywhere, column 0 at the last row and the last column at row 0, every special
    row (the last row class, the last row, the strided rows) is some column's id and (k >= 3) some column's ix."""
    assert (ix != idr).all()
    assert idr[0, 0] == n - 1 and (k == 1 or idr[0, k - 1] == 0)
    special = special_rows(n, k, B, M)
    if k >= len(special) + 2:
        assert set(special) <= set(idr[0].tolist())
        assert set(special) <= set(ix[0].tolist()) | set(idr[0].tolist())
    rows = B // min(k, B)
    if k >= 5 and rows - 1 < n:
        assert rows - 1 in idr[0]
    if k >= 6 and n > M * rows:
        assert (idr[0] >= M * rows).sum() >= 2 and (ix[0] >= M * rows).sum() >= 1


def stop_pass(trace, batch, k):
    """[batch, k]: the pass after which each system was stopped (len(trace) for one that never was)."""
    out = np.full((batch, k), len(trace), dtype=np.int64)
    for p in range(len(trace) - 1, -1, -1):
        out[trace[p]["stopped"]] = p
    return out


def check_mixed(out, batch, k, B):
    """The conditions of case d from the result and the trace of a run to the end (max_iters = 10).  A batch of 3 with
    every kind among its columns: flags 1, 2, 3 all occur, at least three iteration counts among the converged, the very
    last system is among the last active ones and sits in the second workgroup of k_xp_control, frozen columns next to
    applying ones.  Every batch with k > 1: the matrices differ in what applies in some pass."""
    flags, iters = out["flag"], out["iters"]
    trace = out["trace"]
    if batch > 1 and k > 1:                                                  # the offset blockIdx.y * nrhs matters
        assert any((s["apply"][0] != s["apply"][1]).any() for s in trace)
    if batch < 3 or k < len(KINDS):
        return
    assert {1, 2, 3} <= set(flags.tolist()), set(flags.tolist())
    assert len(set(iters[flags == 1].tolist())) >= 3, set(iters[flags == 1].tolist())
    stop = stop_pass(trace, batch, k).reshape(-1)
    assert stop.max() == len(trace) - 1                                     # the loop ended because nobody was left
    last = np.nonzero(stop == stop.max())[0]
    assert batch * k - 1 in last
    if batch * k > B:
        assert last.max() >= B, "the last active system must sit in the second workgroup"
    mixed_pass = False
    for step in trace:
        a = step["apply"]
        mixed_pass |= bool((a[:, 1:] != a[:, :-1]).any())
    assert mixed_pass, "no pass has a frozen column next to an applying one"


def ferr_branch(iters, flag, rate, nd_prev, nxf):
    """Which rule of ferr_rule fires."""
    if flag == 3:
        return "nan"
    if iters == 0:
        return "no_iters"
    if rate >= 1.0:
        return "rate"
    if nd_prev == 0.0 and nxf == 0.0:
        return "zero"
    return "bound"


def ferr_branches(out):
    x = out["x"]
    batch, n, k = x.shape
    got = set()
    for s in range(batch * k):
        nxf = xp_ref._max_nan(np.abs(x[s // k, :, s % k]))
        got.add(ferr_branch(int(out["iters"][s]), int(out["flag"][s]), float(out["rate"][s]), float(out["nd_prev"][s]), nxf))
    return got


# ---- the CPU solver ---------------------------------------------------------------------------------------------------

def cpu_solve_all(case, AX0):
    """solve_all of SuperLU, one matrix and one column at a time (column-independent by construction)."""
    solvers = [xc.superlu_solver(case._replace(Ax0=np.ascontiguousarray(AX0[m]))) for m in range(AX0.shape[0])]
    if case.kind == "matched":
        assert AX0.shape[0] == 1
        solvers = [xc.superlu_solver(case)]

    def solve_all(R):
        R = np.asarray(R, dtype=np.float64).reshape(len(solvers), case.n, -1)
        out = np.empty_like(R)
        for m, s in enumerate(solvers):
            for t in range(R.shape[2]):
                out[m, :, t] = s(np.ascontiguousarray(R[m, :, t]))
        return out

    return solve_all


# ---- the case lists ---------------------------------------------------------------------------------------------------

def column_tile_ks(B):
    return [1, 2, 3, 85, 86, 128, 129, 255, 256, 257, 2 * B + 1]


def tile_name(k, B):
    return "a_k2B1" if k == 2 * B + 1 else "a_k%d" % k


def reps_above(base_n, rows_wanted):
    """The fewest copies whose order is above rows_wanted."""
    return rows_wanted // base_n + 1


def specs(B, G, M):
    """Every planted case by name."""
    out = {}
    for k in column_tile_ks(B):
        out[tile_name(k, B)] = Spec(tile_name(k, B), "chain_3_15", 1, k)
    out["a_n1"] = Spec("a_n1", "n1", 1, B + 1)
    rb = reps_above(32, M)                                        # rows == 1 at both k: the first order above M
    out["b_k5"] = Spec("b_k5", "chain_4_8", rb, 5)                # a tall tile (rows = B / 5) whose last row class has rows
    out["b_k129"] = Spec("b_k129", "chain_4_8", rb, B // 2 + 1)
    out["b_kB1"] = Spec("b_kB1", "chain_4_8", rb, B + 1)
    rc = -(-(G * B + B + 1) // (32 * (B + 1)))                    # n k just above G B + B, the last workgroup of the
    while (rc * 32 * (B + 1) - G * B) % B == 0:                   # second grid pass partial
        rc += 1
    out["c_plain"] = Spec("c_plain", "chain_4_8", rc, B + 1)
    out["c_trans"] = Spec("c_trans", "chain_4_8_t", rb, B + 1, trans=True)
    out["e_spd"] = Spec("e_spd", "chain_spd", 1, B // 2 + 1)
    out["e_matched_k3"] = Spec("e_matched_k3", "permuted", 1, 3)
    out["e_matched_k129"] = Spec("e_matched_k129", "permuted", 1, B // 2 + 1)
    out["e_trans"] = Spec("e_trans", "chain_3_15_t", 1, 17, batch=2, trans=True)
    return out


def mixed_specs(B):
    k = B // 2 + 1
    return {"d_main": Spec("d_main", "chain_4_8", 1, k, batch=3, mixed=True),
            "d_b2_k3": Spec("d_b2_k3", "chain_4_8", 1, 3, batch=2, mixed=True),
            "d_b3_k1": Spec("d_b3_k1", "chain_4_8", 1, 1, batch=3, mixed=True)}


def spec_case(spec):
    return tiled(base_case(spec.base), spec.reps)
