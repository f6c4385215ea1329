"""The cases of tests/test_gpu_big_step_slices.py, tests/test_big_step_slice_cases_cpu.py and
tests/golden/make_big_step_slice_bits.py: matrices whose last block of pivots ends at or beside a multiple of 8.

k_big_step (csrc/kernels.hip) eliminates a block of 32 pivots in four column slices of 8, one wave per slice and half: a
slice receives the pivots to its left through LDS, then eliminates its own.  In a last block of bw < 32 pivots a slice
owns no pivot, one, all but one or all eight of its columns; where that can go wrong is bw at or beside 8, 16 and 24
(tests/big_step_tile_cases.py and tests/big_step_bits_cases.py reach the widths 1, 2, 12 - 17 and 29 - 32, 16 at a root only).

Two groups of sweep_cases.blocks_on_separator((D,) * 4, s), each two fronts (D + s, D) below a dense parentless root of
order 2 D + s:

  group "below"   D = 135, 136, 137, 144, 151, 152, 153,     the NON-ROOT fronts end in a block of D - 128 = 7, 8, 9, 16,
                  s = 30                                      23, 24, 25 pivots with 30 rows and columns behind it: the
                                                              diagonal, block-column and block-row tiles all run it
                                                              (16: the existing shapes reach it at a root only)
  group "root"    D = 129, s = 37, 38, 39, 53, 54, 55         the ROOT (order 258 + s = 9 blocks + s - 30) ends in a block
                                                              of 7, 8, 9, 23, 24, 25 pivots: the diagonal tile alone

tests/test_big_step_slice_cases_cpu.py recomputes the widths from the fronts that the analysis gives and asserts that these
shapes, with the eight existing ones, reach every bucket of WIDTH_BUCKETS twice: in a front with trailing tiles and in a
parentless root.

Each shape as LU and as Cholesky, in batches of 1 and 2; one LU shape of each group also with static pivot perturbation on
and a delta below every pivot (the PivotRule<true> instance, whose steps past bw run with zero multipliers: npiv = bw), so
that nothing is replaced."""
import hashlib

import numpy as np

import big_step_bits_cases as bb
import big_step_tile_cases as tc
import sweep_cases as sc

BIG_NB = tc.BIG_NB
# (D, s) per shape
BELOW = tuple((d, 30) for d in (135, 136, 137, 144, 151, 152, 153))
ROOT = tuple((129, s) for s in (37, 38, 39, 53, 54, 55))
SHAPES = BELOW + ROOT
NAMES = tuple("d%ds%d" % ds for ds in SHAPES)
KINDS = ("lu", "chol")
BATCHES = (1, 2)
LU_TOL = bb.LU_TOL
DELTA = bb.DELTA
PERTURBED = ("d136s30", "d129s54")              # one shape of each group: last blocks of 8 (below the root) and of 24 (root)
# (name, kind, batch, perturbation on)
CASES = [(name, kind, batch, False) for name in NAMES for kind in KINDS for batch in BATCHES] + [
    (name, "lu", 1, True) for name in PERTURBED]

# (r, w) of the fronts with w > 64 in supernode order, the root last
FRONTS = {"d%ds%d" % (d, s): ((d + s, d),) * 2 + ((2 * d + s,) * 2,) for d, s in SHAPES}

WIDTH_BUCKETS = ("1", "2-7", "8", "9-15", "16", "17-23", "24", "25-31", "32")


def bucket(x):
    """The bucket of a block width (1 .. 32): the multiples of 8, 1, and the ranges between them."""
    assert 1 <= x <= BIG_NB
    if x == 1 or x % 8 == 0:
        return str(x)
    lo = max(2, 8 * (x // 8) + 1)
    return "%d-%d" % (lo, 8 * (x // 8) + 7)


def last_width(w):
    """The width of the last block of a front with w pivots."""
    return w - BIG_NB * ((w - 1) // BIG_NB)


def case_id(c):
    name, kind, batch, perturb = c
    return "%s-%s-b%d%s" % (name, kind, batch, "-perturb" if perturb else "")


def _shape(name):
    return SHAPES[NAMES.index(name)]


def _seed(name, i):
    return 7000 * (1 + NAMES.index(name)) + i


def case_matrix(name, symmetric=False):
    d, s = _shape(name)
    return sc.blocks_on_separator((d,) * 4, s, _seed(name, 0), symmetric=symmetric)


_VALUES = {}


def case_values(name, batch, symmetric=False):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own (built once; read-only)."""
    key = (name, batch, symmetric)
    if key not in _VALUES:
        d, s = _shape(name)
        AX = np.stack([sc.blocks_on_separator((d,) * 4, s, _seed(name, i), symmetric=symmetric)[4] for i in range(batch)])
        AX.setflags(write=False)
        _VALUES[key] = AX
    return _VALUES[key]


def record(hip, case):
    """big_step_bits_cases.record for a case of this file: factor, read the factors back, then one fused refactor + solve.
    -> {"Lx", "Ux", "x": SHA-256 of the bytes, "sum_*": their sums}.  Asserts that the factor and fused plans hold BIG_BLOCK
    steps (the case runs k_big_step) and, with perturbation on, that no pivot was replaced."""
    import torch
    name, kind, batch, perturb = case
    sym = kind == "chol"
    m, n, Ap, Ai, _ = case_matrix(name, symmetric=sym)
    AX = case_values(name, batch, symmetric=sym)
    tol = 0.0 if sym else LU_TOL
    B = np.random.default_rng(6100 + batch).standard_normal((batch, n, 1))
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if sym else hip.CS3_LU, batch=batch) as F:
        for op in ("factor", "fused"):
            assert bb.has_big_block_steps(hip, F, op), "%s: the %s plan holds no BIG_BLOCK step" % (case_id(case), op)
        if perturb:
            F.set_perturbation(DELTA)
        F.factor(AX, tol)
        parts = [F.factors(b) for b in range(batch)]
        Lx = np.concatenate([p[2] for p in parts])
        Ux = np.concatenate([p[5] for p in parts]) if not sym else np.zeros(0)
        if perturb:
            assert not F.perturbed().any()
        d_ax = torch.from_numpy(AX.copy()).to(dev)
        d_b = torch.from_numpy(B).to(dev)
        d_x = torch.zeros_like(d_b)
        F.factor_solve_bx_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, tol, sh)
        F.factor_status(sh)
        x = d_x.cpu().numpy()
    out = {}
    for key, a in (("Lx", Lx), ("Ux", Ux), ("x", x)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        out[key] = hashlib.sha256(a.tobytes()).hexdigest()
        out["sum_" + key] = repr(float(a.sum()))
    return out
