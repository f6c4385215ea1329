"""The cases of tests/test_gpu_big_step_tiles.py, tests/test_big_step_tile_cases_cpu.py and
tests/golden/make_big_step_tile_bits.py: matrices that put k_big_step's panel tiles (csrc/kernels.hip: the diagonal tile,
the block-column tiles and the block-row tiles of a block step) at the block widths and ragged tile extents that the
three shapes of tests/big_step_bits_cases.py leave out.

The panel tiles compute only the 16 x 16 blocks that their 32-wide panel uses, and a block-row tile deals its eight blocks
to its four waves, 32 rows by 32 columns each.  Where that can go wrong is a block or a last tile that ends at or beside a
multiple of 16: a last block of 16 pivots, a ragged last tile of 1, 16, 32 or 48 rows or columns.

The matrices are sweep_cases.blocks_on_separator((129,) * 4, s): two fronts (129 + s, 129) on one level below a dense
parentless root of order 258 + s.  A front (r, w) runs the block steps kb = 0, 32, .. < w; step kb has the block
[kb, ke), ke = min(kb + 32, w), and r - ke rows and columns behind it in tiles of 64, the last one ragged:

  case      non-root (r, w)   root   last block (non-root, root)   last tile's extent over the steps (non-root; root)
  d129s31   (160, 129)        289    1, 1                          31, 32, 64; 1, 33
  d129s45   (174, 129)        303    1, 15                         14, 46, 45; 15, 47
  d129s46   (175, 129)        304    1, 16                         15, 47, 46; 16, 48
  d129s47   (176, 129)        305    1, 17                         16, 48, 47; 17, 49
  d129s61   (190, 129)        319    1, 31                         30, 62, 61; 31, 63

The non-root fronts have 1 to 3 trailing tile rows, the roots 1 to 5.  The shapes of big_step_bits_cases add a last block
of 32 and of 2 - 15 below the root, and the extents 32 and 64 at the root.  test_big_step_tile_cases_cpu.py recomputes the
buckets from the fronts that the analysis gives and asserts that the eight shapes together reach every one of them."""
import numpy as np

import big_step_bits_cases as bb
import sweep_cases as sc

BIG_NB = 32                                    # cs3_device.hpp: pivots per block step
D = 129
SEPS = (31, 45, 46, 47, 61)
NAMES = tuple("d%ds%d" % (D, s) for s in SEPS)
KINDS = ("lu", "chol")
BATCHES = (1, 2)
LU_TOL = bb.LU_TOL
# (name, kind, batch)
CASES = [(name, kind, batch) for name in NAMES for kind in KINDS for batch in BATCHES]

# (r, w) of the fronts with w > 64 in supernode order, the root last
FRONTS = {"d%ds%d" % (D, s): ((D + s, D),) * 2 + ((2 * D + s,) * 2,) for s in SEPS}
# ... and of the three shapes of big_step_bits_cases (wide_chunk_cases.FRONTS)
BITS_FRONTS = {"d129s30": ((159, 129),) * 2 + ((288, 288),), "d160s30": ((190, 160),) * 2 + ((350, 350),),
               "d130s200": ((330, 130),) * 2 + ((460, 460),)}

WIDTH_BUCKETS = ("1", "2-15", "16", "17-31", "32")
EXTENT_BUCKETS = ("1", "2-15", "16", "17-31", "32", "33-47", "48", "49-63", "64")


def bucket(x):
    """The bucket of a block width (1 .. 32) or of a tile extent (1 .. 64)."""
    assert 1 <= x <= 64
    if x in (1, 16, 32, 48, 64):
        return str(x)
    lo = 2 if x < 16 else 16 * (x // 16) + 1
    return "%d-%d" % (lo, 16 * (x // 16) + 15)


def reach(r, w):
    """What the block steps of a front (r, w) reach: (buckets of the last block's width, buckets of the ragged last
    tile's extent over all steps, numbers of trailing tile rows over all steps)."""
    widths, extents, rows = set(), set(), set()
    for kb in range(0, w, BIG_NB):
        ke = min(kb + BIG_NB, w)
        if ke == w:
            widths.add(bucket(ke - kb))
        if r > ke:
            nsl = -(-(r - ke) // 64)
            rows.add(nsl)
            extents.add(bucket(r - ke - 64 * (nsl - 1)))
    return widths, extents, rows


def case_id(c):
    return "%s-%s-b%d" % c


def _seed(name, i):
    return 9000 * (1 + NAMES.index(name)) + i


def case_matrix(name, symmetric=False):
    return sc.blocks_on_separator((D,) * 4, SEPS[NAMES.index(name)], _seed(name, 0), symmetric=symmetric)


_VALUES = {}


def case_values(name, batch, symmetric=False):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own (built once; read-only)."""
    key = (name, batch, symmetric)
    if key not in _VALUES:
        AX = np.stack([sc.blocks_on_separator((D,) * 4, SEPS[NAMES.index(name)], _seed(name, i), symmetric=symmetric)[4]
                       for i in range(batch)])
        AX.setflags(write=False)
        _VALUES[key] = AX
    return _VALUES[key]


def record(hip, case):
    """big_step_bits_cases.record for a case of this file: factor, read the factors back, then one fused refactor + solve.
    -> {"Lx", "Ux", "x": SHA-256 of the bytes, "sum_*": their sums}.  Asserts that the factor and fused plans hold BIG_BLOCK
    steps: the case runs k_big_step."""
    import hashlib

    import torch
    name, kind, batch = case
    sym = kind == "chol"
    m, n, Ap, Ai, _ = case_matrix(name, symmetric=sym)
    AX = case_values(name, batch, symmetric=sym)
    tol = 0.0 if sym else LU_TOL
    B = np.random.default_rng(5300 + batch).standard_normal((batch, n, 1))
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if sym else hip.CS3_LU, batch=batch) as F:
        for op in ("factor", "fused"):
            assert bb.has_big_block_steps(hip, F, op), "%s: the %s plan holds no BIG_BLOCK step" % (case_id(case), op)
        F.factor(AX, tol)
        parts = [F.factors(b) for b in range(batch)]
        Lx = np.concatenate([p[2] for p in parts])
        Ux = np.concatenate([p[5] for p in parts]) if not sym else np.zeros(0)
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
