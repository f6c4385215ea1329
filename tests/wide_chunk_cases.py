"""Matrices whose wide big fronts are swept four 64-blocks (256 columns) per launch, and a restatement of the rule that
picks the chunk width, for tests/test_wide_chunk_cases_cpu.py and tests/test_gpu_wide_chunks.py.

The matrices are sweep_cases.blocks_on_separator((d,) * 4, s): two fronts (d + s, d) on one level below a parentless root
(2 d + s, 2 d + s).  With few right-hand sides (batch * nrhs < 8) a launch group of big fronts whose widest front has
more than 128 pivots takes k_fwd_big_step4 / k_bwd_big_step4 (schedule.cpp: big_sweep_plan); the cases put a front's
width w at every place where those kernels change what they do:

  case      non-root fronts   root        256-chunks of (non-root, root)    last chunk's columns (non-root, root)
  d129s30   (159, 129)        (288, 288)  1, 2                              129 (3 blocks: 64 64 1), 32
  d192s30   (222, 192)        (414, 414)  1, 2                              192 (3 blocks), 158
  d193s30   (223, 193)        (416, 416)  1, 2                              193 (4 blocks: .. 1), 160
  d256s30   (286, 256)        (542, 542)  1, 3                              256 (full), 30
  d257s30   (287, 257)        (544, 544)  2, 3                              1, 32
  d130s200  (330, 130)        (460, 460)  1, 2                              130, 204 (200 rows below the non-root pivots)
  d160s30   (190, 160)        (350, 350)  1, 2                              160, 94 (2 blocks: the one count the others lack)

The root has no rows of ancestors (r == w) and is alone in its launch group: its backward sweep has no k_bwd_big_init;
the first chunk launch reads X itself, parks its solution in the front vector when other workgroups may still be reading
X (a root of two or more chunks) and the second launch takes it home.  The non-root fronts come as a group of two with
rows of ancestors: they keep the init launch.
"""
import numpy as np

import sweep_cases as sc

# name -> (ds, s)
CASES = {"d129s30": ((129,) * 4, 30), "d192s30": ((192,) * 4, 30), "d193s30": ((193,) * 4, 30),
         "d256s30": ((256,) * 4, 30), "d257s30": ((257,) * 4, 30), "d130s200": ((130,) * 4, 200), "d160s30": ((160,) * 4, 30)}
ORDER = {name: sum(ds) + s for name, (ds, s) in CASES.items()}
# (r, w) of the fronts with w > 64 in supernode order, the root last
FRONTS = {name: ((ds[0] + s, ds[0]),) * 2 + ((2 * ds[0] + s,) * 2,) for name, (ds, s) in CASES.items()}

SOLVE_BW, BIG_CW, BIG_CW4 = 64, 128, 256       # cs3_device.hpp
GEMM_MIN = 16                                  # cs3_device.hpp: RHS_LANES_MIN

# (batch, right-hand sides): the first five sweep the cases' fronts in 256-column chunks, the last two as before
PAIRS_NEW = ((1, 1), (1, 2), (1, 7), (2, 3), (7, 1))
PAIRS_OLD = ((1, 8), (2, 4))
BATCHES = (1, 2, 7)


def chunk_width(batch, nrhs, max_w):
    """schedule.cpp, big_sweep_plan: columns per chunk launch of a group of big fronts whose widest has max_w pivots
    (fewer than 16 right-hand sides: beyond, the GEMM sweeps take them)."""
    assert nrhs < GEMM_MIN and batch <= sc.BIG_BATCH_MAX
    if batch * nrhs < 8:
        return BIG_CW4 if max_w > BIG_CW else BIG_CW
    return SOLVE_BW


def skips_init(batch, nrhs, fronts):
    """schedule.cpp, big_sweep_plan: no k_bwd_big_init for a group of one front without rows of ancestors, on the 256 path.
    fronts: the (r, w) of the group."""
    return chunk_width(batch, nrhs, max(w for _, w in fronts)) == BIG_CW4 and len(fronts) == 1 and fronts[0][0] == fronts[0][1]


def _seed(name, i):
    return 7000 * (1 + list(CASES).index(name)) + i


def case_matrix(name, symmetric=False):
    ds, s = CASES[name]
    return sc.blocks_on_separator(ds, s, _seed(name, 0), symmetric=symmetric)


_VALUES = {}


def case_values(name, batch, symmetric=False):
    """float64 [batch, nnz]: `batch` matrices of case `name`, each with values of its own (built once; read-only)."""
    key = (name, batch, symmetric)
    if key not in _VALUES:
        ds, s = CASES[name]
        AX = np.stack([sc.blocks_on_separator(ds, s, _seed(name, i), symmetric=symmetric)[4] for i in range(batch)])
        AX.setflags(write=False)
        _VALUES[key] = AX
    return _VALUES[key]
