"""Sweeps of 1 to 15 right-hand sides on the level schedule, at the edges of their waves, blocks, lists and launch groups.

Below 16 right-hand sides -- refinement, GMRES, low-rank updates, condition estimates, every transposed and every batched
solve -- the fronts are swept by k_fwd_wave / k_bwd_wave<KIND, 1 | 8> (one wave per front, four fronts per workgroup, 8
columns per tile), k_fwd_blk / k_bwd_blk (one workgroup per front and column), k_fwd_il / k_bwd_il (lane = matrix, from
128 matrices on) and the forward assembly through gather_front / gather_front_vec over the lists of emit_runs, and the
launcher regroups what the analysis scheduled (sweep_groups, absorb_small_group).  The matrices of tests/few_rhs_cases.py
are built for the edges of all that; tests/test_few_rhs_cases_cpu.py asserts from the host analysis that they deliver
them, and names the kernel of every front in every call made here:
  wave       (33, 1), (64, 8) against (65, 9), (127, 63) against (128, 64), w % 8 != 0 with (r - w) % 8 = 1 and 7, (73, 60)
             with ancestors in rows 60 .. 72, a root (64, 64) without a parent, launches of 4 k + 1 fronts, the small group
             of a level inside its wave launch, pivot rows with 63, 64, 65 and 66 sources (the last two: long runs);
  block      (129, 64), (137, 64), w = 8 with 255, 256, 257 ancestors, (100, 65), (136, 128), (136, 129), (82, 81), w = 31,
             32, 33, (262, 64) with a list of 17 chunks, lists of exactly 64 and of 64 + 1 entries, a long run that would
             start at chunk position 63, runs moved because they would straddle a chunk;
  promote16  15 fronts of order <= 32 and one of order 34 swept by the block kernels beside a block front (a lone matrix),
  promote17  one front more: by the wave kernels;
  hub, t16   (tests/rhs_cases.py) a long run under an order-136 root; lane = matrix fronts at 2 and 9 right-hand sides;
  w72        (tests/sweep_cases.py) wide fronts on the block kernels in a batch of 20, 3 and 9 right-hand sides.

References: every column of every checked matrix against sweep_cases.substitute (np.longdouble) on that handle's own
factors; a full solve against the chain of two such sweeps.

Bounds.  Per column max|x - ref| <= RTOL max|ref| (helpers, 1e-10).  Per column the project's norm-wise residual 1e-12
(norm(T) max|x| + max|b|) with n u |T||x| taken off, the residual formed in np.longdouble.  Every half sweep:
|b - T x| <= 2 n u |T||x| componentwise (Higham's bound for substitution in any order, the factor 2 for reciprocal
multiplies as in helpers.assert_backward_error) -- every kernel reached here is plain substitution; the largest ratio is
printed next to the oracle's.  Exact, with no reference: a zero column stays zero; B 2^40 gives
X 2^40; a column's bits do not depend on what the other columns hold (one of them NaN), nor on where it sits (reversed
columns), nor on how many columns follow it (2, 9, 15; transposed: 1 as well); a repeated call gives the same bits; a
poisoned LDS changes none; the fused step equals factor + solve; the _dev half sweeps equal the host forms."""
import collections
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import few_rhs_cases as fc
import rhs_cases as rc
import sweep_cases as sc
from helpers import RTOL, U_ROUND

pytestmark = pytest.mark.gpu

LU_TOL = 1e-3
KINDS = ("lu", "chol")

Held = collections.namedtuple("Held", "F AX mat q factors")


def _tol(kind):
    return 0.0 if kind == "chol" else LU_TOL


@pytest.fixture(scope="module")
def handles(gpu):
    """One factorised handle per (case, kind, batch), shared by every test of this module; every matrix of a batch has
    values of its own.  Tests that factorise again do so with the same values."""
    held = {}

    def get(name, kind, batch):
        key = (name, kind, batch)
        if key not in held:
            sym = kind == "chol"
            mat = fc.case_matrix(name, symmetric=sym)
            F = fc.handle(gpu, name, kind, batch)
            AX = fc.case_values(name, batch, symmetric=sym)
            F.factor(AX, _tol(kind))
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


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


# -------------------------------------------------------------------------- paths --

Path = collections.namedtuple("Path", "wave tiles last_tile batch")


def _path(batch, nrhs):
    """What a sweep of `nrhs` right-hand sides in a batch of `batch` goes through: the instance of the wave kernels, its
    tiles of 8 columns and the live columns of the last one; the batch class (single: the wave group of a level may join
    its block group; few; block: wide big fronts on the block kernels from 16 matrices on; il: fronts of order <= 16
    lane = matrix)."""
    assert 1 <= nrhs <= fc.FEW_RHS_MAX
    cls = "il" if batch >= rc.IL_MIN_BATCH else "block" if batch > sc.BIG_BATCH_MAX else "few" if batch > 1 else "single"
    return Path(1 if nrhs == 1 else fc.KT, -(-nrhs // fc.KT), (nrhs - 1) % fc.KT + 1, cls)


PAIRS = {(1, 1): Path(1, 1, 1, "single"),          # k_fwd_wave / k_bwd_wave<KIND, 1>
         (1, 2): Path(8, 1, 2, "single"),          # the fewest columns of <KIND, 8>
         (1, 7): Path(8, 1, 7, "single"),
         (1, 8): Path(8, 1, 8, "single"),          # a full tile
         (1, 9): Path(8, 2, 1, "single"),          # one column into the second
         (1, 15): Path(8, 2, 7, "single"),         # the most columns of these kernels
         (4, 2): Path(8, 1, 2, "few"),
         (4, 9): Path(8, 2, 1, "few"),
         (20, 3): Path(8, 1, 3, "block"),
         (20, 9): Path(8, 2, 1, "block"),
         (130, 2): Path(8, 1, 2, "il"),            # lane = row parents over lane = matrix children, 2 .. 15 columns
         (130, 9): Path(8, 2, 1, "il")}
REDUCED = {"promote16": ((1, 1), (1, 9), (4, 2)), "promote17": ((1, 1), (1, 9), (4, 2)), "hub": ((1, 1), (1, 9), (20, 3)),
           "t16": ((130, 2), (130, 9)), fc.WIDE: ((20, 3), (20, 9))}


def _pairs(name):
    return REDUCED.get(name, tuple(PAIRS))


def test_the_pairs_take_the_paths_they_are_there_for():
    assert all(_path(*pair) == path for pair, path in PAIRS.items())
    assert {p.batch for p in PAIRS.values()} == {"single", "few", "block", "il"}
    assert {p.wave for p in PAIRS.values()} == {1, fc.KT} and {p.last_tile for p in PAIRS.values()} >= {1, 2, 7, 8}
    assert {(p.tiles, p.batch) for p in PAIRS.values()} >= {(t, c) for t in (1, 2) for c in ("single", "few", "block", "il")}
    assert all(pair in PAIRS for pairs in REDUCED.values() for pair in pairs) and set(REDUCED) | {"wave", "block"} == set(fc.CASES)
    assert all(b == 130 for b, _ in REDUCED["t16"]) and all(b == 20 for b, _ in REDUCED[fc.WIDE])
    assert all({(1, 1), (1, 9)} <= set(REDUCED[nm]) and any(b > 1 for b, _ in REDUCED[nm]) for nm in ("promote16", "promote17", "hub"))


# mode -> ((factor, lower, trans) of each sweep in turn, permuted); factor 'L' or 'U'
MODES = {"lu": {"lsolve": ((("L", True, False),), False), "usolve": ((("U", False, False),), False),
                "utsolve": ((("U", False, True),), False), "ltsolve": ((("L", True, True),), False),
                "solve": ((("L", True, False), ("U", False, False)), True),
                "solve_t": ((("U", False, True), ("L", True, True)), True)},
         "chol": {"lsolve": ((("L", True, False),), False), "usolve": ((("L", True, True),), False),
                  "solve": ((("L", True, False), ("L", True, True)), True)}}
TRANS_CALLS = ("utsolve", "ltsolve", "solve_t")        # LU: the calls that take the level schedule whatever nrhs is

SWEEP_CASES = [(name, kind, pair, mode) for name in fc.CASES for pair in _pairs(name) for kind in KINDS for mode in MODES[kind]]
SWEEP_IDS = ["%s-%s-b%d-k%d-%s" % (nm, kd, p[0], p[1], md) for nm, kd, p, md in SWEEP_CASES]


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


def _checked(batch):
    """The matrices whose every column is compared with the reference: all of a batch up to 20; of a larger one the first,
    one in the middle, the last of the first lane = matrix group of 64, the first of the second, and the last."""
    return list(range(batch)) if batch <= 20 else sorted({0, batch // 2, min(63, batch - 1), min(64, batch - 1), batch - 1})


def _system(h, b, mode, kind):
    """(the CSC matrix T that `mode` solves with on matrix b, transposed, a half sweep)."""
    m, n, Ap, Ai, _ = h.mat
    sweeps, permute = MODES[kind][mode]
    if permute:
        return (Ap, Ai, h.AX[b]), mode == "solve_t", False
    which, lower, trans = sweeps[0]
    L, U = _factors(h, b)
    return (L if which == "L" else U), trans, True


def _oracle_sweep(orc, n, G, lower, trans, Bb):
    fn = {(True, False): orc.csc_lsolve_f, (False, False): orc.csc_usolve_f, (True, True): orc.csc_ltsolve_f,
          (False, True): orc.csc_utsolve_f}[lower, trans]
    X = np.empty_like(Bb)
    for j in range(Bb.shape[1]):
        x = Bb[:, j].copy()
        fn(n, *G, x)
        X[:, j] = x
    return X


@pytest.mark.parametrize("name,kind,pair,mode", SWEEP_CASES, ids=SWEEP_IDS)
def test_sweeps(gpu, orc, handles, name, kind, pair, mode):
    batch, nrhs = pair
    h = handles(name, kind, batch)
    F = h.F
    n = F.n
    sweeps, permute = MODES[kind][mode]
    what = "%s %s batch %d nrhs %d %s" % (name, kind, batch, nrhs, mode)
    ncol = batch * nrhs
    B = rc.right_hand_sides(batch, n, nrhs, seed=1000 * batch + nrhs)
    zero = [(c // nrhs, c % nrhs) for c in range(ncol) if not B[c // nrhs, :, c % nrhs].any()]
    assert zero == ([(2 // nrhs, 2 % nrhs)] if ncol >= 4 else [])
    X = _run(F, mode, B)
    assert X.shape == B.shape
    worst = 0.0
    for b in _checked(batch):
        # every column against the reference
        ref = _reference(h, b, mode, kind, B[b])
        scale = np.abs(ref).max(axis=0)
        err = np.abs(X[b] - ref).max(axis=0)
        for j in range(nrhs):
            if scale[j] == 0:
                assert (b, j) in zero and not X[b][:, j].any(), "%s matrix %d column %d: a zero column came back nonzero" % (what, b, j)
            else:
                assert err[j] <= RTOL * scale[j], "%s matrix %d column %d: relative error %.3e" % (what, b, j, float(err[j] / scale[j]))
        # the project's norm-wise residual, per column.  A full solve: T x is a float64 product; what that product can be
        # off by, n u |T||x|, is taken off the limit.  A half sweep: the residual is formed in np.longdouble for the
        # componentwise bound below, and the same term stays on its side of the comparison
        G, trans, half = _system(h, b, mode, kind)
        Xb, Bb = X[b], B[b]
        if half:
            ratio, E, W = fc.error_ratio(n, G, Xb, Bb, trans)
        else:
            T = sp.csc_matrix((G[2], G[1], G[0]), shape=(n, n))
            T = T.T.tocsc() if trans else T
            E, W = np.abs(T @ Xb - Bb).max(axis=0), (abs(T) @ np.abs(Xb)).max(axis=0)
        res = E + n * U_ROUND * W
        lim = 1e-12 * (fc.norm1(n, *G, trans) * np.abs(Xb).max(axis=0) + np.abs(Bb).max(axis=0))
        assert (res <= lim).all(), "%s matrix %d: residual / limit %.3g" % (what, b, float((res / np.where(lim > 0, lim, 1)).max()))
        if not half:
            continue
        # half sweeps, componentwise
        assert (ratio <= 2 * n).all(), "%s matrix %d column %d: max |b - T x| / (u |T||x|) = %.2f > %d" % (what, b, int(ratio.argmax()), ratio.max(), 2 * n)
        worst = max(worst, float(ratio.max()))
        if b == 0:
            which, lower, tr = sweeps[0]
            o = fc.error_ratio(n, G, _oracle_sweep(orc, n, G, lower, tr, Bb), Bb, trans)[0].max()
    if not permute:
        print("%s: max |b - T x| / (u |T||x|): kernels %.2f, oracle (matrix 0) %.2f (bound 2 n = %d)" % (what, worst, o, 2 * n))
    # B 2^40 -> X 2^40, exactly
    assert np.array_equal(_run(F, mode, B * 2.0 ** 40), X * 2.0 ** 40), what + ": scaling the right-hand sides by 2^40 changes bits"
    # everything but the first and the last column replaced, one column all NaN: the kept columns keep their bits
    keep = sorted({0, ncol - 1})
    if ncol >= 3:
        B_other = np.random.default_rng(7).standard_normal((batch, n, nrhs)) * 3.0
        B_other[1 // nrhs, :, 1 % nrhs] = np.nan
        for c in keep:
            B_other[c // nrhs, :, c % nrhs] = B[c // nrhs, :, c % nrhs]
        X_other = _run(F, mode, B_other)
        for c in keep:
            assert np.array_equal(X_other[c // nrhs, :, c % nrhs], X[c // nrhs, :, c % nrhs]), \
                "%s: matrix %d column %d depends on the other columns" % (what, c // nrhs, c % nrhs)
    # the same call again
    assert np.array_equal(_run(F, mode, B), X), what + ": two calls differ"
    # the columns of every matrix in reverse order: every column runs the same instruction stream in another slot of a tile
    if nrhs > 1:
        X_rev = _run(F, mode, np.ascontiguousarray(B[:, :, ::-1]))[:, :, ::-1]
        assert np.array_equal(X_rev, X), what + ": a column's bits depend on where it sits"


# ------------------------------------------------------------- leading columns --

PREFIX_CASES = [(name, kind, batch) for name in fc.CASES for batch in sorted({p[0] for p in _pairs(name)}) for kind in KINDS]


@pytest.mark.parametrize("name,kind,batch", PREFIX_CASES, ids=["%s-%s-b%d" % c for c in PREFIX_CASES])
def test_a_column_does_not_depend_on_how_many_follow(gpu, handles, name, kind, batch):
    """Column j of a 2-column, a 9-column and a 15-column call on the same leading columns has the same bits: the wave
    kernels run one instruction stream per column of a tile, the block and lane = matrix kernels one per column.  A
    transposed call of ONE column takes the same schedule (<KIND, 1>): the same bits again.  (A plain call of one column may
    take the bottom forest's sweeps: compared with the reference in test_sweeps only.)"""
    h = handles(name, kind, batch)
    B = rc.right_hand_sides(batch, h.F.n, 15, seed=15 + batch)
    for mode in MODES[kind]:
        X15 = _run(h.F, mode, B)
        for k in (9, 2) + ((1,) if mode in TRANS_CALLS else ()):
            Xk = _run(h.F, mode, np.ascontiguousarray(B[:, :, :k]))
            assert np.array_equal(Xk, X15[:, :, :k]), "%s %s batch %d %s: the leading %d columns of 15 differ from a call of %d" % (name, kind, batch, mode, k, k)


# ------------------------------------------------------------------- promotion --

@pytest.mark.parametrize("nrhs", (1, 2, 9))
@pytest.mark.parametrize("kind", KINDS)
def test_promoted_fronts_against_the_wave_kernels(gpu, kind, nrhs):
    """The 16 fronts that promote16 and promote17 have in common hold the same values (fc.promote_pair) and are leaves:
    their pivot rows of lsolve depend on nothing else.  promote16 sweeps them with k_fwd_blk (promoted into the level's
    block group), promote17 with k_fwd_wave: the same rows to RTOL."""
    sym = kind == "chol"
    Ax16, Ax17, cols = fc.promote_pair(sym)
    with fc.handle(gpu, "promote16", kind, 1) as F16, fc.handle(gpu, "promote17", kind, 1) as F17:
        D16, D17 = fc.dispatch(gpu, F16, nrhs), fc.dispatch(gpu, F17, nrhs)
        group = [s for s in range(len(D16.P.w)) if D16.P.level[s] == 0 and D16.P.r[s] <= 128]
        assert len(group) == 16 and {D16.kernel_of[s] for s in group} == {"blk"}
        assert {D17.kernel_of[s] for s in range(len(D17.P.w)) if D17.P.level[s] == 0 and D17.P.r[s] <= 128} == {"wave1" if nrhs == 1 else "wave8"}
        F16.factor(Ax16, _tol(kind))
        F17.factor(Ax17, _tol(kind))
        q16, q17 = F16.ordering()["q"], F17.ordering()["q"]
        b17 = np.random.default_rng(16 + nrhs).standard_normal((F17.n, nrhs))
        b16 = b17[cols]
        Y16 = np.empty_like(b16)
        Y17 = np.empty_like(b17)
        Y16[q16] = F16.lsolve(np.ascontiguousarray(b16[q16]))            # (rows back in the order of the matrix' columns)
        Y17[q17] = F17.lsolve(np.ascontiguousarray(b17[q17]))
        sn_ptr = F16.supernodes()[0]
        for s in group:
            mine = q16[sn_ptr[s]:sn_ptr[s + 1]]
            got, want = Y16[mine], Y17[cols[mine]]
            assert (np.abs(got - want).max(axis=0) <= RTOL * np.abs(want).max(axis=0)).all(), "front %d (%d, %d)" % (s, D16.P.r[s], D16.P.w[s])


# --------------------------------------------------------------------- fused step --

FUSED_PAIRS = [(1, 1), (1, 2), (1, 9), (4, 7), (20, 3), (130, 2)]


@pytest.mark.parametrize("pair", FUSED_PAIRS, ids=["b%d-k%d" % p for p in FUSED_PAIRS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["wave", "block"])
def test_fused_step_equals_factor_then_solve(gpu, handles, name, kind, pair):
    """factor_solve_bx_dev == factor_dev + solve_dev bit for bit, three times (the third call replays the graph kept per
    solution buffer)."""
    import torch
    batch, nrhs = pair
    h = handles(name, kind, batch)
    F = h.F
    n = F.n
    tol = _tol(kind)
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    B = rc.right_hand_sides(batch, n, nrhs, seed=77 + nrhs)
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
        ok = np.where(scale > 0, np.abs(X[b] - ref).max(axis=0) <= RTOL * scale, ~X[b].any(axis=0))
        assert ok.all()


# ------------------------------------------------------------------- poisoned LDS --

@pytest.mark.parametrize("pair", [(1, 9), (4, 2)], ids=["b1-k9", "b4-k2"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["wave", "block"])
def test_a_poisoned_lds_changes_no_bit(gpu, handles, name, kind, pair):
    """k_fwd_blk multiplies whole 64-wide chunks of its vector and k_fwd_wave assembles through LDS: whatever an earlier
    kernel left there must not reach a result."""
    batch, nrhs = pair
    h = handles(name, kind, batch)
    B = rc.right_hand_sides(batch, h.F.n, nrhs, seed=99 + nrhs)
    for mode in MODES[kind]:
        X = _run(h.F, mode, B)
        _poison(gpu)
        assert np.array_equal(_run(h.F, mode, B), X), "%s %s batch %d nrhs %d %s" % (name, kind, batch, nrhs, mode)


# ------------------------------------------------------------ device half sweeps --

@pytest.mark.parametrize("k", (1, 9))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["wave", "block"])
def test_device_half_sweeps_equal_the_host_forms(gpu, handles, name, kind, k):
    import torch
    for batch in (1, 4):
        h = handles(name, kind, batch)
        F = h.F
        sh = torch.cuda.current_stream().cuda_stream
        B = rc.right_hand_sides(batch, F.n, k, seed=31 + k)
        for mode in ("lsolve", "usolve", "ltsolve", "utsolve"):
            x = torch.from_numpy(B).to(torch.device("cuda", 0))
            call = getattr(F, mode + "_dev")
            if mode == "utsolve" and kind == "chol":
                with pytest.raises(gpu.Cs3Error):
                    F.utsolve(B)
                with pytest.raises(gpu.Cs3Error):
                    call(x.data_ptr(), k, sh)
                continue
            call(x.data_ptr(), k, sh)
            torch.cuda.synchronize()
            assert np.array_equal(x.cpu().numpy(), getattr(F, mode)(B)), "%s %s batch %d k %d %s" % (name, kind, batch, k, mode)
