"""Wide big fronts BELOW the root, and their sweeps in batches of 2 to 15.

Everywhere else in the suite the only front with w > 64 pivots and r > 136 rows is the root (r == w, no parent), and no
batch of 2 to 15 matrices has such a front at all.  The matrices of tests/sweep_cases.py have two of them on one level
under a big root (tests/test_sweep_cases_cpu.py asserts the shapes from the host analysis), which reaches
  k_big_step's Schur complement of the rows below the pivots and its assembly into a big parent (k_big_gather);
  the hand-over of those rows to the parent in k_fwd_big_step, k_fwd_big_step_multi and k_gemm_fwd;
  k_bwd_big_init and k_gemm_bwd_init with rows of the ancestors to read (nb = r - w > 0);
  a big launch group with two fronts (blockIdx.z > 0);
  k_fwd_big_step / k_bwd_big_step with 64-column chunks (batch * nrhs >= 8 and nrhs < 8: batches of 2 to 15 only);
  the wide and multi kernels and the GEMM sweeps of a big front at a matrix index b > 0;
  the fused step's pipelined root sweep with 64-column chunks.

References: the factors against the CPU oracle's; every half sweep against sweep_cases.substitute (np.longdouble) on
that handle's own factors, every column of every matrix; a full solve against the chain of two such sweeps.

Bounds.  Per column max|x - ref| / max|ref| <= RTOL (helpers, 1e-10): per column, so that the columns scaled by 2^200 and
2^-200 cannot hide the others.  Fewer than 16 right-hand sides (substitution kernels): |b - T x| <= 2 n u |T||x|
componentwise per half sweep -- Higham's bound for substitution in any order, with the factor 2 that
helpers.assert_backward_error uses for reciprocal multiplies; a float64 column-oriented substitution reaches 12 to 15 u
on these factors.  16 or more right-hand sides (explicit 64 x 64 inverses, not covered by that bound): the project's
norm-wise residual 1e-12 (norm(T) max|x| + max|b|) per column; the componentwise ratio is printed and recorded in
DESIGN.md section 7, nothing is asserted on it.  Exact, with no reference: a zero column stays zero; B 2^40 gives X 2^40;
a column's bits do not depend on what the other columns hold (one of them NaN); a repeated call gives the same bits."""
import collections

import numpy as np
import pytest

import pivot_cases as pc
import sweep_cases as sc
from helpers import RTOL, U_ROUND, assert_backward_error, assert_factor_equal, backward_error_ratio_dense, lower_transposed, permuted
from rhs_cases import right_hand_sides as _right_hand_sides         # (shared with tests/test_gpu_many_rhs_edges.py)

pytestmark = pytest.mark.gpu

LU_TOL = 1e-3
FRINGE = 40                    # as in tests/test_sweep_cases_cpu.py
KINDS = ("lu", "chol")

Held = collections.namedtuple("Held", "F AX mat q factors")


@pytest.fixture(scope="module")
def handles(gpu):
    """One factorised handle per (case, fringe, kind, batch), shared by every test of this module; every matrix of a batch
    has values of its own.  Tests that factorise again do so with the same values."""
    held = {}

    def get(name, kind, batch, fringe=0):
        key = (name, fringe, kind, batch)
        if key not in held:
            sym = kind == "chol"
            mat = sc.case_matrix(name, symmetric=sym, fringe=fringe)
            m, n, Ap, Ai, _ = mat
            F = gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY if sym else gpu.CS3_LU, batch=batch)
            AX = sc.case_values(name, batch, symmetric=sym, fringe=fringe)
            F.factor(AX, 0.0 if sym else LU_TOL)
            held[key] = Held(F, AX, mat, F.ordering()["q"], {})
        return held[key]

    yield get
    for h in held.values():
        h.F.close()


def _factors(h, b):
    """(L, U) of matrix b as CSC triples; U = None for Cholesky.  Read once per handle and matrix."""
    if b not in h.factors:
        Lp, Li, Lx, Up, Ui, Ux = h.F.factors(b=b)
        h.factors[b] = ((Lp, Li, Lx), None if Up is None else (Up, Ui, Ux))
    return h.factors[b]


# ------------------------------------------------------------------------ factors --

FACTOR_CASES = [(name, 0, batch) for name in ("w72", "w100", "w200") for batch in (1, 4, 20, 50)] + [("w72", FRINGE, 1), ("w72", FRINGE, 4)]


@pytest.mark.parametrize("name,fringe,batch", FACTOR_CASES, ids=["%s%s-b%d" % (nm, "f" if fr else "", b) for nm, fr, b in FACTOR_CASES])
@pytest.mark.parametrize("kind", KINDS)
def test_factors_of_big_fronts_with_a_parent(gpu, orc, handles, kind, name, fringe, batch):
    """k_big_step alone (1) and in a batch (4, 20), k_front_wg (50): the Schur complement below the pivots of a wide big
    front and its assembly into a big parent; with the fringe, small children assembled into a big front that has a parent."""
    h = handles(name, kind, batch, fringe)
    m, n, Ap, Ai, _ = h.mat
    K = sc.solve_kinds(gpu, h.F)
    below_root = [s for s in sc.wide_fronts(K) if K.parent[s] >= 0]
    assert len(below_root) >= 2 and all(K.r[s] > max(136, K.w[s]) for s in below_root)
    assert {K.cls[s] for s in sc.wide_fronts(K)} == {"wg" if batch >= 48 else "big_step"}
    first = {}
    for b in sorted({0, batch - 1}):
        L, U = _factors(h, b)
        what = "%s %s b%d/%d" % (name, kind, b, batch)
        A = permuted(n, Ap, Ai, h.AX[b], h.q)
        if kind == "lu":
            oL = orc.csc_lu_f(n, n, Ap, Ai, h.AX[b], h.q, LU_TOL)
            assert np.array_equal(oL[6], np.argsort(h.q)), what + ": the oracle left the diagonal"
            assert_factor_equal(n, L, oL[0:3], what + " L")
            assert_factor_equal(n, U, oL[3:6], what + " U")
            o_ratio = backward_error_ratio_dense(n, A, oL[0:3], oL[3:6])[0]
            g_ratio = assert_backward_error(n, A, L, U, what, oracle_ratio=o_ratio, dense=True)
        else:
            oL = pc.oracle_chol(orc, n, Ap, Ai, h.AX[b], h.q)
            assert_factor_equal(n, L, oL, what + " L")
            o_ratio = backward_error_ratio_dense(n, A, oL, lower_transposed(n, oL))[0]
            g_ratio = assert_backward_error(n, A, L, lower_transposed(n, L), what, oracle_ratio=o_ratio, dense=True)
        print("%s: max |PAQ - LU| / (u |L||U|): kernels %.2f, oracle %.2f (bound %d)" % (what, g_ratio, o_ratio, 2 * n))
        first[b] = (L[2].copy(), None if U is None else U[2].copy())
    # a second factorisation of the same values: the same bits
    h.F.factor(h.AX, 0.0 if kind == "chol" else LU_TOL)
    for b, (Lx, Ux) in first.items():
        got = h.F.factors(b=b)
        assert np.array_equal(got[2], Lx), "matrix %d: L differs between two factorisations" % b
        assert Ux is None or np.array_equal(got[5], Ux), "matrix %d: U differs between two factorisations" % b


# ------------------------------------------------------------------------- sweeps --

# (batch, right-hand sides) -> how the big fronts are swept (kernels.hip: launch_solve_group, big_sweep_plan)
PAIRS = {(1, 1): "wide", (1, 7): "wide", (1, 8): "multi", (1, 9): "multi", (1, 15): "multi",
         (1, 16): "gemm", (1, 17): "gemm", (1, 65): "gemm", (1, 256): "gemm",            # (256: the permutation rides the sweeps)
         (2, 3): "wide", (2, 4): "narrow", (4, 1): "wide", (4, 2): "narrow", (4, 7): "narrow", (4, 9): "multi", (4, 17): "gemm",
         (15, 1): "narrow", (15, 7): "narrow", (16, 1): "block"}
GEMM_MIN = 16                  # cs3_device.hpp: RHS_LANES_MIN


def _path(batch, nrhs):
    if batch > sc.BIG_BATCH_MAX:
        return "block"
    if nrhs >= GEMM_MIN:
        return "gemm"
    if batch * nrhs < 8:
        return "wide"
    return "multi" if nrhs >= 8 else "narrow"


def test_the_pairs_take_the_paths_they_are_there_for():
    assert all(_path(*pair) == path for pair, path in PAIRS.items())
    assert set(PAIRS.values()) == {"wide", "multi", "narrow", "gemm", "block"}


SWEEP_CASES = ([(name, 0, pair) for name in ("w72", "w140") for pair in PAIRS] + [("w200", 0, pair) for pair in PAIRS if pair[0] == 1] +
               [("w72", FRINGE, pair) for pair in ((1, 1), (1, 9), (1, 17), (4, 2))])
SWEEP_IDS = ["%s%s-b%d-k%d-%s" % (nm, "f" if fr else "", p[0], p[1], PAIRS[p]) for nm, fr, p in SWEEP_CASES]

# mode -> ((factor, lower, trans) of each sweep in turn, permuted); factor 'L' or 'U'
MODES = {"lu": {"lsolve": ((("L", True, False),), False), "usolve": ((("U", False, False),), False),
                "utsolve": ((("U", False, True),), False), "ltsolve": ((("L", True, True),), False),
                "solve": ((("L", True, False), ("U", False, False)), True),
                "solve_t": ((("U", False, True), ("L", True, True)), True)},
         "chol": {"lsolve": ((("L", True, False),), False), "usolve": ((("L", True, True),), False),
                  "solve": ((("L", True, False), ("L", True, True)), True)}}


def _run(F, mode, B):
    if mode == "solve_t":
        return F.solve(B, trans=True)
    return getattr(F, mode)(B)


def _reference(h, b, mode, kind, Bb):
    """np.longdouble [n, nrhs]: the sweeps of `mode` on matrix b's own factors."""
    n = h.F.n
    L, U = _factors(h, b)
    sweeps, permute = MODES[kind][mode]
    x = Bb[h.q] if permute else Bb
    for which, lower, trans in sweeps:
        x = sc.substitute(n, *(L if which == "L" else U), x, lower, trans)
    if permute:
        out = np.empty_like(x)
        out[h.q] = x
        return out
    return x


def _oracle_sweep_ratio(orc, n, G, lower, trans, T, Bb):
    """The componentwise ratio of the oracle's own float64 sweep on the same factor and right-hand sides."""
    fn = {(True, False): orc.csc_lsolve_f, (False, False): orc.csc_usolve_f, (True, True): orc.csc_ltsolve_f,
          (False, True): orc.csc_utsolve_f}[lower, trans]
    X = np.empty_like(Bb)
    for j in range(Bb.shape[1]):
        x = Bb[:, j].copy()
        fn(n, *G, x)
        X[:, j] = x
    return sc.substitution_error_ratio(T, X, Bb).max()


@pytest.mark.parametrize("name,fringe,pair", SWEEP_CASES, ids=SWEEP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_sweeps_of_big_fronts_with_a_parent(gpu, orc, handles, kind, name, fringe, pair):
    batch, nrhs = pair
    h = handles(name, kind, batch, fringe)
    F = h.F
    m, n, Ap, Ai, _ = h.mat
    K = sc.solve_kinds(gpu, F)
    below_root = [s for s in sc.wide_fronts(K) if K.parent[s] >= 0]
    assert len(below_root) >= 2 and {K.kind[s] for s in sc.wide_fronts(K)} == {"block" if PAIRS[pair] == "block" else "big"}
    ncol = batch * nrhs
    B = _right_hand_sides(batch, n, nrhs, seed=1000 * batch + nrhs)
    zero = [(c // nrhs, c % nrhs) for c in range(ncol) if not B[c // nrhs, :, c % nrhs].any()]
    assert len(zero) == (1 if ncol >= 4 else 0)
    # the same right-hand sides with everything but two columns replaced: fresh values, and one column all NaN
    keep = sorted({0, ncol - 1}) if ncol >= 3 else [0]
    B_other = np.random.default_rng(7).standard_normal((batch, n, nrhs)) * 3.0
    if ncol >= 2:
        B_other[1 // nrhs, :, 1 % nrhs] = np.nan
    for c in keep:
        B_other[c // nrhs, :, c % nrhs] = B[c // nrhs, :, c % nrhs]
    gemm_ratio = {}
    for mode, (sweeps, permute) in MODES[kind].items():
        what = "%s %s batch %d nrhs %d %s" % (name, kind, batch, nrhs, mode)
        X = _run(F, mode, B)
        assert X.shape == B.shape
        for b in range(batch):
            L, U = _factors(h, b)
            Xb, Bb = X[b], B[b]
            ref = _reference(h, b, mode, kind, Bb)
            scale = np.abs(ref).max(axis=0)
            err = np.abs(Xb - ref).max(axis=0)
            for j in range(nrhs):
                if scale[j] == 0:
                    assert (b, j) in zero and not Xb[:, j].any(), "%s matrix %d column %d: a zero column came back nonzero" % (what, b, j)
                else:
                    assert err[j] <= RTOL * scale[j], "%s matrix %d column %d: relative error %.3e" % (what, b, j, float(err[j] / scale[j]))
            if permute:                                  # the system itself (solve_t: its transpose)
                T64 = sc.dense64(n, Ap, Ai, h.AX[b], trans=mode == "solve_t")
            else:
                which, lower, trans = sweeps[0]
                G = L if which == "L" else U
                T64 = sc.dense64(n, *G, trans=trans)
            # the project's norm-wise residual, per column.  T x is a float64 product here; what that product can be off
            # by, n u |T||x|, is taken off the limit.
            res = np.abs(T64 @ Xb - Bb).max(axis=0) + n * U_ROUND * (np.abs(T64) @ np.abs(Xb)).max(axis=0)
            lim = 1e-12 * (np.abs(T64).sum(axis=0).max() * np.abs(Xb).max(axis=0) + np.abs(Bb).max(axis=0))
            assert (res <= lim).all(), "%s matrix %d: residual / limit %.3g" % (what, b, float((res / np.where(lim > 0, lim, 1)).max()))
            if not permute and (nrhs < GEMM_MIN or b == 0):
                cols = np.arange(nrhs) if nrhs < GEMM_MIN else np.r_[0:GEMM_MIN, nrhs - 1]      # (GEMM sweeps: a sample, reported)
                ratio = sc.substitution_error_ratio(T64.astype(np.longdouble), Xb[:, cols], Bb[:, cols])
                if nrhs < GEMM_MIN:
                    assert (ratio <= 2 * n).all(), "%s matrix %d: max |b - T x| / (u |T||x|) = %.2f > %d" % (what, b, ratio.max(), 2 * n)
                else:
                    gemm_ratio[mode] = (ratio.max(), _oracle_sweep_ratio(orc, n, G, lower, trans, T64.astype(np.longdouble), Bb[:, cols]))
        # B 2^40 -> X 2^40, exactly
        assert np.array_equal(_run(F, mode, B * 2.0 ** 40), X * 2.0 ** 40), what + ": scaling the right-hand sides by 2^40 changes bits"
        # the other columns replaced, one of them NaN: the kept columns come back with the same bits
        X_other = _run(F, mode, B_other)
        for c in keep:
            assert np.array_equal(X_other[c // nrhs, :, c % nrhs], X[c // nrhs, :, c % nrhs]), \
                "%s: matrix %d column %d depends on the other columns" % (what, c // nrhs, c % nrhs)
        # and the same call again
        assert np.array_equal(_run(F, mode, B), X), what + ": two calls differ"
    for mode, (g, o) in gemm_ratio.items():
        print("%s %s batch %d nrhs %d %s: max |b - T x| / (u |T||x|): kernels %.2f, oracle %.2f (2 n = %d, not asserted)"
              % (name, kind, batch, nrhs, mode, g, o, 2 * n))


# --------------------------------------------------------------------- fused step --

FUSED_PAIRS = [(1, 1), (1, 9), (1, 17), (2, 4), (4, 2), (15, 1)]


@pytest.mark.parametrize("pair", FUSED_PAIRS, ids=["b%d-k%d" % p for p in FUSED_PAIRS])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_equals_factor_then_solve(gpu, handles, kind, pair):
    """factor_solve_bx_dev == factor_dev + solve_dev bit for bit, three times (the third call replays the graph kept per
    solution buffer).  (2, 4), (4, 2) and (15, 1): the root's pipelined sweep in 64-column chunks; (1, 1): big fronts on the
    level below the root, where the forward sweep forks off the factorisation."""
    import torch
    batch, nrhs = pair
    h = handles("w140", kind, batch)
    F = h.F
    n = F.n
    tol = 0.0 if kind == "chol" else LU_TOL
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    B = _right_hand_sides(batch, n, nrhs, seed=77 + nrhs)
    d_ax = torch.from_numpy(h.AX.copy()).to(dev)
    d_b = torch.from_numpy(B).to(dev)
    x_split = d_b.clone()
    F.factor_dev(d_ax.data_ptr(), tol, sh)
    F.solve_dev(x_split.data_ptr(), nrhs, sh)
    F.factor_status(sh)
    x_fused = torch.zeros_like(d_b)
    for _ in range(3):
        x_fused.zero_()
        F.factor_solve_bx_dev(d_ax.data_ptr(), d_b.data_ptr(), x_fused.data_ptr(), nrhs, tol, sh)
        F.factor_status(sh)
        assert torch.equal(x_fused, x_split)
    assert torch.equal(d_b, torch.from_numpy(B).to(dev))
    X = x_split.cpu().numpy()
    for b in sorted({0, batch - 1}):
        ref = _reference(h, b, "solve", kind, B[b])
        scale = np.abs(ref).max(axis=0)
        assert (np.abs(X[b] - ref).max(axis=0) <= RTOL * scale).all()
