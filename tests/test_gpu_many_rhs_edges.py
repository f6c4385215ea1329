"""Sweeps of 16 or more right-hand sides at the edges of their slot rounds, register-size instances, tiles and batches.

From 16 right-hand sides on the sweeps run through kernels of their own -- k_fwd_rhs / k_bwd_rhs<KIND, RMAX> (lane =
right-hand side; RMAX 16, 24, 32), the GEMM sweeps (k_gemm_gather, k_gemm_fwd, k_gemm_bwd_init, k_gemm_bwd on the
inverted diagonal blocks of k_inv_diag), the permutation fused into them from 256 right-hand sides, parallel graph
branches from 512 -- and the inverted blocks are recomputed outside the graph when a host flag says they are stale.
The matrices of tests/rhs_cases.py are built for the edges of all that (tests/test_rhs_cases_cpu.py asserts the shapes
from the host analysis): a front with 5, 9 to 14 slot rounds in every instance of k_fwd_rhs (it keeps 4 in registers),
64 and 65 rounds into k_gemm_gather (it keeps 64), fronts of order 17 and 32, of one pivot and of one row below the
pivots, two GEMM fronts in one launch group, an order-136 block front, and all of it in batches that sweep their small
fronts lane = matrix underneath (130).

References: every column of every checked matrix against sweep_cases.substitute (np.longdouble) on that handle's own
factors; a full solve against the chain of two such sweeps.

Bounds.  Per column max|x - ref| <= RTOL max|ref| (helpers, 1e-10).  Per column and for every matrix the project's
norm-wise residual 1e-12 (norm(T) max|x| + max|b|), the float64 product's own error n u |T||x| taken off.  t16, t24, t32
(every front swept by plain substitution with reciprocal multiplies, lane = right-hand side or lane = matrix): every half
sweep has |b - T x| <= 2 n u |T||x| componentwise, the bound of helpers.assert_backward_error; the oracle's float64 sweeps
reach a few u on these factors (tests/test_rhs_cases_cpu.py).  hub (explicit 64 x 64 inverses, not covered by that bound):
the ratio is printed next to the oracle's and recorded in DESIGN.md section 7, nothing is asserted on it.  Exact, with no
reference: a zero column stays zero; B 2^40 gives X 2^40; a column's bits do not depend on what the other columns hold
(one of them NaN); a repeated call gives the same bits; on t16, t24, t32 a column's bits do not depend on where it sits
(B with its columns reversed) nor on whether the permutation rides the sweeps (256 columns against 255)."""
import collections

import numpy as np
import pytest

import rhs_cases as rc
import sweep_cases as sc
from helpers import RTOL, U_ROUND

pytestmark = pytest.mark.gpu

LU_TOL = 1e-3
KINDS = ("lu", "chol")
SUBSTITUTION_ONLY = ("t16", "t24", "t32")          # no front beyond order 32: no explicit inverses anywhere

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
            mat = rc.case_matrix(name, symmetric=sym)
            F = rc.handle(gpu, name, kind, batch)
            AX = rc.case_values(name, batch, symmetric=sym)
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


# -------------------------------------------------------------------------- paths --

TILE = 64                      # kernels.hip: right-hand sides per wave (k_fwd_rhs) and per GEMM tile (GC)
FUSED_PERM_MIN = 256           # schedule.cpp: permutation_can_fuse (and no interleaved pool: il_len == 0)
BRANCHES_MIN = 512             # schedule.cpp: plan_solve_levels, parallel
WG_MIN_BATCH = 48              # schedule.cpp: CS3_WG_MIN_BATCH (k_front_wg factors the big fronts)

Path = collections.namedtuple("Path", "tiles last_tile perm branches batch")


def _path(batch, nrhs):
    """What a sweep of `nrhs` right-hand sides in a batch of `batch` goes through: tiles of 64 columns and the columns of
    the last one; the permutation as kernels of its own or fused into the sweeps; the groups of a level one after the
    other or as parallel graph branches; the batch class (single / few: wide big fronts SK_BIG; block: SK_BLOCK from 16
    matrices on; wg: big fronts factored by k_front_wg; il: fronts of order <= 16 lane = matrix)."""
    assert nrhs >= rc.RHS_LANES_MIN
    cls = ("il" if batch >= rc.IL_MIN_BATCH else "wg" if batch >= WG_MIN_BATCH else "block" if batch > sc.BIG_BATCH_MAX else
           "few" if batch > 1 else "single")
    fused = nrhs >= FUSED_PERM_MIN and batch < rc.IL_MIN_BATCH
    return Path(-(-nrhs // TILE), (nrhs - 1) % TILE + 1, "fused" if fused else "kernels", nrhs >= BRANCHES_MIN, cls)


PAIRS = {(1, 16): Path(1, 16, "kernels", False, "single"),        # the fewest right-hand sides of these kernels
         (1, 17): Path(1, 17, "kernels", False, "single"),
         (1, 64): Path(1, 64, "kernels", False, "single"),        # a full tile
         (1, 65): Path(2, 1, "kernels", False, "single"),         # one column into the second
         (1, 255): Path(4, 63, "kernels", False, "single"),       # the last count with permutation kernels
         (1, 256): Path(4, 64, "fused", False, "single"),         # the first with the permutation in the sweeps
         (1, 257): Path(5, 1, "fused", False, "single"),
         (1, 512): Path(8, 64, "fused", True, "single"),          # the groups of a level as parallel branches
         (2, 16): Path(1, 16, "kernels", False, "few"),
         (2, 256): Path(4, 64, "fused", False, "few"),            # the fused permutation at a matrix index > 0
         (4, 70): Path(2, 6, "kernels", False, "few"),
         (20, 17): Path(1, 17, "kernels", False, "block"),        # GEMM sweeps with blockIdx.z = front * batch + matrix, batch >= 16
         (50, 16): Path(1, 16, "kernels", False, "wg"),
         (130, 16): Path(1, 16, "kernels", False, "il"),          # lane = right-hand-side parents over lane = matrix children
         (130, 65): Path(2, 1, "kernels", False, "il"),
         (130, 256): Path(4, 64, "kernels", False, "il")}         # 256 right-hand sides that cannot fuse
REDUCED = ((1, 16), (1, 65), (1, 256), (4, 70), (130, 16))


def test_the_pairs_take_the_paths_they_are_there_for():
    assert all(_path(*pair) == path for pair, path in PAIRS.items())
    assert {p.batch for p in PAIRS.values()} == {"single", "few", "block", "wg", "il"}
    assert {(p.perm, p.batch != "single") for p in PAIRS.values()} == {("kernels", False), ("fused", False), ("kernels", True), ("fused", True)}
    assert any(p.branches for p in PAIRS.values()) and all(pair in PAIRS for pair in REDUCED)


# mode -> ((factor, lower, trans) of each sweep in turn, permuted); factor 'L' or 'U'
MODES = {"lu": {"lsolve": ((("L", True, False),), False), "usolve": ((("U", False, False),), False),
                "utsolve": ((("U", False, True),), False), "ltsolve": ((("L", True, True),), False),
                "solve": ((("L", True, False), ("U", False, False)), True),
                "solve_t": ((("U", False, True), ("L", True, True)), True)},
         "chol": {"lsolve": ((("L", True, False),), False), "usolve": ((("L", True, True),), False),
                  "solve": ((("L", True, False), ("L", True, True)), True)}}

SWEEP_CASES = [(name, kind, pair, mode) for name in rc.TREES for pair in PAIRS if name in ("t24", "hub") or pair in REDUCED
               for kind in KINDS for mode in MODES[kind]]
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
    """(dense float64 T, the CSC factor or None, lower, trans) of what `mode` solves on matrix b."""
    m, n, Ap, Ai, _ = h.mat
    sweeps, permute = MODES[kind][mode]
    if permute:
        return sc.dense64(n, Ap, Ai, h.AX[b], trans=mode == "solve_t"), None, None, None
    which, lower, trans = sweeps[0]
    L, U = _factors(h, b)
    G = L if which == "L" else U
    return sc.dense64(n, *G, trans=trans), G, lower, trans


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
    assert zero == [(0, 2)]
    X = _run(F, mode, B)
    assert X.shape == B.shape
    # every column of the checked matrices against the reference
    for b in _checked(batch):
        ref = _reference(h, b, mode, kind, B[b])
        scale = np.abs(ref).max(axis=0)
        err = np.abs(X[b] - ref).max(axis=0)
        for j in range(nrhs):
            if scale[j] == 0:
                assert (b, j) in zero and not X[b][:, j].any(), "%s matrix %d column %d: a zero column came back nonzero" % (what, b, j)
            else:
                assert err[j] <= RTOL * scale[j], "%s matrix %d column %d: relative error %.3e" % (what, b, j, float(err[j] / scale[j]))
    # the project's norm-wise residual, per column, every matrix.  T x is a float64 product here; what that product can be
    # off by, n u |T||x|, is taken off the limit.
    for b in range(batch):
        T64, G, lower, trans = _system(h, b, mode, kind)
        Xb, Bb = X[b], B[b]
        res = np.abs(T64 @ Xb - Bb).max(axis=0) + n * U_ROUND * (np.abs(T64) @ np.abs(Xb)).max(axis=0)
        lim = 1e-12 * (np.abs(T64).sum(axis=0).max() * np.abs(Xb).max(axis=0) + np.abs(Bb).max(axis=0))
        assert (res <= lim).all(), "%s matrix %d: residual / limit %.3g" % (what, b, float((res / np.where(lim > 0, lim, 1)).max()))
        if permute or b not in _checked(batch):
            continue
        # half sweeps, componentwise
        if name in SUBSTITUTION_ONLY:
            ratio = sc.substitution_error_ratio(T64.astype(np.longdouble), Xb, Bb)
            assert (ratio <= 2 * n).all(), "%s matrix %d column %d: max |b - T x| / (u |T||x|) = %.2f > %d" % (what, b, int(ratio.argmax()), ratio.max(), 2 * n)
            if b == 0:
                print("%s: max |b - T x| / (u |T||x|) = %.2f (bound 2 n = %d)" % (what, ratio.max(), 2 * n))
        elif b == 0:
            cols = np.unique(np.r_[0:min(nrhs, 16), nrhs - 1])                               # (a sample, reported)
            TL = T64.astype(np.longdouble)
            g = sc.substitution_error_ratio(TL, Xb[:, cols], Bb[:, cols]).max()
            o = sc.substitution_error_ratio(TL, _oracle_sweep(orc, n, G, lower, trans, Bb[:, cols]), Bb[:, cols]).max()
            print("%s: max |b - T x| / (u |T||x|): kernels %.2f, oracle %.2f (2 n = %d, not asserted)" % (what, g, o, 2 * n))
    # B 2^40 -> X 2^40, exactly
    assert np.array_equal(_run(F, mode, B * 2.0 ** 40), X * 2.0 ** 40), what + ": scaling the right-hand sides by 2^40 changes bits"
    # everything but the first and the last column replaced, one column all NaN: the kept columns keep their bits
    keep = [0, ncol - 1]
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
    # the columns of every matrix in reverse order: lane j runs the instruction stream of lane k - 1 - j on another column
    X_rev = _run(F, mode, np.ascontiguousarray(B[:, :, ::-1]))[:, :, ::-1]
    if name in SUBSTITUTION_ONLY:
        assert np.array_equal(X_rev, X), what + ": a column's bits depend on where it sits"
    else:                                              # (the matrix cores sum a tile's columns in lane-dependent places)
        scale = np.abs(X).max(axis=1, keepdims=True)
        assert (np.abs(X_rev - X) <= RTOL * scale).all(), what + ": a column depends on where it sits"


# ------------------------------------------------------------- fused permutation --

@pytest.mark.parametrize("batch", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(rc.TREES))
def test_fused_permutation_equals_the_permutation_kernels(gpu, handles, name, kind, batch):
    """Column j of a 256-column solve (the permutation rides the sweeps: XMap) against column j of the 255-column solve of
    the same leading columns (permutation kernels)."""
    h = handles(name, kind, batch)
    n = h.F.n
    assert _path(batch, 256).perm == "fused" and _path(batch, 255).perm == "kernels"
    B = rc.right_hand_sides(batch, n, 256, seed=256 + batch)
    for mode in [m for m, (_, permute) in MODES[kind].items() if permute]:
        X256 = _run(h.F, mode, B)
        X255 = _run(h.F, mode, np.ascontiguousarray(B[:, :, :255]))
        what = "%s %s batch %d %s" % (name, kind, batch, mode)
        if name in SUBSTITUTION_ONLY:
            assert np.array_equal(X256[:, :, :255], X255), what + ": the fused permutation changes bits"
        else:
            scale = np.abs(X255).max(axis=1, keepdims=True)
            assert (np.abs(X256[:, :, :255] - X255) <= RTOL * scale).all(), what


# --------------------------------------------------------------------- fused step --

FUSED_PAIRS = [(1, 16), (1, 256), (4, 70), (20, 17), (130, 16)]


@pytest.mark.parametrize("pair", FUSED_PAIRS, ids=["b%d-k%d" % p for p in FUSED_PAIRS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["t24", "hub"])
def test_fused_step_equals_factor_then_solve(gpu, handles, name, kind, pair):
    """factor_solve_bx_dev == factor_dev + solve_dev bit for bit, three times (the third call replays the graph kept per
    solution buffer); in the fused step the forward sweep inverts the diagonal blocks group by group."""
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


# ---------------------------------------------- state of the inverted diagonal blocks --

STATE_K = 16


class _Dev:
    """A handle of `hub` driven through device pointers, next to what a fresh handle gives."""

    def __init__(self, gpu, kind, batch):
        import torch
        self.torch, self.gpu, self.kind, self.batch = torch, gpu, kind, batch
        self.dev = torch.device("cuda", 0)
        self.sh = torch.cuda.current_stream().cuda_stream
        sym = kind == "chol"
        self.A = [rc.case_values("hub", batch, symmetric=sym, other=o) for o in (False, True)]
        self.dA = [torch.from_numpy(a.copy()).to(self.dev) for a in self.A]
        self.F = rc.handle(gpu, "hub", kind, batch)
        self.n = self.F.n
        self.B = rc.right_hand_sides(batch, self.n, STATE_K, seed=5 + batch)
        self.B1 = np.ascontiguousarray(self.B[:, :, :1])

    def close(self):
        self.F.close()

    def factor(self, which):
        self.F.factor_dev(self.dA[which].data_ptr(), _tol(self.kind), self.sh)
        self.F.factor_status(self.sh)

    def fused(self, which, B):
        d_b = self.torch.from_numpy(B).to(self.dev)
        x = self.torch.zeros_like(d_b)
        self.F.factor_solve_bx_dev(self.dA[which].data_ptr(), d_b.data_ptr(), x.data_ptr(), B.shape[2], _tol(self.kind), self.sh)
        self.F.factor_status(self.sh)
        return x.cpu().numpy()

    def sweep(self, mode, F=None):
        return _run(F or self.F, mode, self.B)

    def fresh(self, which, mode):
        """`mode` on a handle that has seen nothing but the values `which`."""
        with rc.handle(self.gpu, "hub", self.kind, self.batch) as G:
            G.factor(self.A[which], _tol(self.kind))
            return self.sweep(mode, G)


@pytest.fixture(scope="module")
def fresh_results(gpu):
    """What fresh handles give for the 16 right-hand sides of the state tests, per (kind, batch, value set, mode): once."""
    got = {}

    def get(d, which, mode):
        key = (d.kind, d.batch, which, mode)
        if key not in got:
            got[key] = d.fresh(which, mode)
        return got[key]
    return get


@pytest.fixture(params=[(k, b) for k in KINDS for b in (1, 4)], ids=lambda p: "%s-b%d" % p)
def dev(gpu, request):
    d = _Dev(gpu, *request.param)
    yield d
    d.close()


def _same(got, want, what):
    assert np.array_equal(got, want), what + ": differs from a fresh handle that saw only the final values"


def test_state_refactor_between_two_sweeps(dev, fresh_results):
    """factor(A1), solve, factor(A2), solve: the second solve needs the inverses of A2's diagonal blocks."""
    dev.factor(0)
    _same(dev.sweep("solve"), fresh_results(dev, 0, "solve"), "solve after factor(A1)")
    dev.factor(1)
    _same(dev.sweep("solve"), fresh_results(dev, 1, "solve"), "solve after factor(A1), solve, factor(A2)")


def test_state_sweeps_after_a_fused_step_of_many_columns(dev, fresh_results):
    """The fused step on 16 columns inverts inside its forward sweep and leaves the inverses current."""
    dev.factor(0)
    dev.sweep("solve")
    _same(dev.fused(1, dev.B), fresh_results(dev, 1, "solve"), "fused step")
    for mode in ("solve", "lsolve", "usolve") + (("solve_t",) if dev.kind == "lu" else ()):
        _same(dev.sweep(mode), fresh_results(dev, 1, mode), mode + " after a fused step of 16 columns")


def test_state_sweeps_after_a_fused_step_of_one_column(dev, fresh_results):
    """The fused step on ONE column computes no inverses: those of the earlier factorisation must not survive it."""
    dev.factor(0)
    _same(dev.sweep("solve"), fresh_results(dev, 0, "solve"), "solve after factor(A1)")
    x1 = dev.fused(1, dev.B1)
    want = fresh_results(dev, 1, "solve")
    scale = np.abs(want[:, :, :1]).max(axis=1, keepdims=True)
    assert (np.abs(x1 - want[:, :, :1]) <= RTOL * scale).all()             # (one column takes other kernels: not the same bits)
    _same(dev.sweep("solve"), want, "solve after solve(A1), fused step of one column on A2")


def test_state_half_sweeps_after_a_refactorisation(dev, fresh_results):
    """lsolve and usolve return before the permutations (mode != 0): they need current inverses all the same."""
    _same(dev.fused(0, dev.B), fresh_results(dev, 0, "solve"), "fused step")
    dev.factor(1)
    for mode in ("lsolve", "usolve"):
        _same(dev.sweep(mode), fresh_results(dev, 1, mode), mode + " after fused step (A1), factor(A2)")


def test_state_imported_factors(gpu, fresh_results):
    """import_factor_dev into a handle whose inverted blocks belong to other factors."""
    import torch
    src, dst = _Dev(gpu, "lu", 1), _Dev(gpu, "lu", 1)
    try:
        src.factor(1)
        buf = torch.empty(int(src.F.info.factor_bytes) // 8, dtype=torch.float64, device=src.dev)
        src.F.export_factor_dev(buf.data_ptr(), src.sh)
        dst.factor(0)
        _same(dst.sweep("solve"), fresh_results(dst, 0, "solve"), "solve after factor(A1)")
        dst.F.import_factor_dev(buf.data_ptr(), dst.sh)
        _same(dst.sweep("solve"), fresh_results(dst, 1, "solve"), "solve after import of A2's factors")
    finally:
        src.close()
        dst.close()
