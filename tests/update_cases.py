"""Case lists that put the low-rank-modified solves (cs3_updates_*: csrc/updates.hip and updates_build in csrc/apps.cpp)
at their engineered edges, for tests/test_update_cases_cpu.py and tests/test_gpu_update_edges.py.

What the kernels do with a case (updates.hip): k_upd_capacitance gives a wave to a case, forms S = I + D G in LDS with
the right-hand side in column 16, and eliminates with partial pivoting -- an xor butterfly over (|value|, row), a swap of
columns k .. 16 of two rows, a running minimum of the pivots -- then substitutes back.  k_upd_apply gives a lane to a case
and a workgroup of max(512, round64(cases of the tile)) threads to 128 rows; Z travels through LDS in stages of 8 rows
whose odd last entry goes through thread 0, and a lane finds its columns of Z in 16-bit positions packed two per word.
updates_build cuts the list into tiles of at most 1024 touched rows and 1024 cases.

The lists that arise from networks (updates_ref.branch_outages) are all 2 x 2 and their S is close to I: they swap at
most once and never reach a step k > 0, the capacity of a tile or an odd width.  Here S is DESIGNED: for a square case
on rows R with columns C = R, G = (A^-1)[R, R] comes from SuperLU and D = (S - I) G^-1 is emitted as r x r triplets, so
that the reference's S is the chosen one up to rounding (for s > r: D = (S - I) G^+).  `pivot_trace` restates the
elimination in NumPy, so that the CPU test can assert from the reference's own S what each case is there for."""
import collections
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import updates_ref as ur

RANKS = (2, 3, 5, 8, 15, 16)
MAX_RANK, MAX_TILE, MAX_TILE_CASES = 16, 1024, 1024        # cs3_device.hpp: UPD_MAX_RANK, UPD_MAX_TILE, UPD_MAX_TILE_CASES
N_PIVOT, N_TILES = 137, 1100                               # the matrices of the pivoting and of the structural lists
ROW_ORDERS = (1, 7, 8, 9, 127, 128, 129, 137)              # stages of 8 rows, row blocks of 128: below, at, above


# ------------------------------------------------------------------ matrices --

def small_matrix(n, spd=False):
    """-> (m, n, Ap, Ai, Ax) of any order n >= 1: three bands on either side, off-diagonal U(-1, 1) (unsymmetric, or
    mirrored for spd), diagonal = the row's absolute sum + U(1, 2): strictly diagonally dominant.  One seed per n."""
    rng = np.random.default_rng((7100000 if spd else 7000000) + n)
    diags, offs = [], []
    for k in range(1, min(3, n - 1) + 1):
        up = rng.uniform(-1.0, 1.0, size=n - k)
        lo = up if spd else rng.uniform(-1.0, 1.0, size=n - k)
        diags += [up, lo]
        offs += [k, -k]
    A = sp.diags(diags, offs, shape=(n, n), format="csr") if diags else sp.csr_matrix((n, n))
    d = np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, size=n)
    A = (A + sp.diags([d], [0], shape=(n, n))).tocsc()
    A.sort_indices()
    return n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def decoupled(case, i, value=2.0):
    """The matrix with row and column i cut off and a_ii = value: (A^-1)_ii = 1 / value in any arithmetic, so that with a
    power of two dA = (i, i, -value) has S = 1 + (-value)(1 / value) = 0 EXACTLY, on the device as in the reference."""
    m, n, Ap, Ai, Ax = case
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n)).tolil()
    A[i, :] = 0.0
    A[:, i] = 0.0
    A[i, i] = value
    A = A.tocsc()
    A.eliminate_zeros()
    A.sort_indices()
    return n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


Base = collections.namedtuple("Base", "m n Ap Ai Ax A lu b")


def _base(case, seed):
    m, n, Ap, Ai, Ax = case
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    Ax.setflags(write=False)
    b = np.random.default_rng(seed).standard_normal(n)
    b.setflags(write=False)
    return Base(m, n, Ap, Ai, Ax, A, spla.splu(A), b)


@functools.lru_cache(maxsize=None)
def base(n, spd=False):
    """The matrix of order n with its SuperLU factors and its right-hand side b (built once)."""
    return _base(small_matrix(n, spd), 7200000 + n)


ZERO_ROW = 4


@functools.lru_cache(maxsize=None)
def base_exact_zero():
    """Order 9 with row ZERO_ROW cut off (a_ii = 2): the one list with an exactly zero pivot."""
    return _base(decoupled(small_matrix(9), ZERO_ROW), 7200009)


# --------------------------------------------------------- the pivot counter --

PivotTrace = collections.namedtuple("PivotTrace", "picks swaps margins margin pivots smallest_step")


def pivot_trace(S):
    """Elimination with partial pivoting (largest |.|, ties to the lowest row), restated.  picks[k]: the row taken at step
    k; swaps: steps with picks[k] != k; margins[k]: (largest - second largest) / largest among the candidates of step k
    (steps 0 .. r-2; the last step has one candidate); margin: their minimum; pivots[k] = |pivot k|; smallest_step:
    where the smallest pivot falls."""
    U = np.array(S, dtype=np.float64, copy=True)
    r = U.shape[0]
    picks, margins, pivots = [], [], []
    for k in range(r):
        col = np.abs(U[k:, k])
        p = k + int(np.argmax(col))                        # the first of equal maxima: the lowest row
        if len(col) > 1:
            top = np.sort(col)[::-1]
            margins.append(float((top[0] - top[1]) / top[0]) if top[0] > 0 else 0.0)
        picks.append(p)
        pivots.append(float(col.max()))
        if pivots[-1] == 0.0:
            break
        U[[k, p]] = U[[p, k]]
        U[k + 1:, k:] -= np.outer(U[k + 1:, k] / U[k, k], U[k, k:])
    swaps = sum(p != k for k, p in enumerate(picks))
    return PivotTrace(picks, swaps, margins, min(margins) if margins else np.inf, pivots, int(np.argmin(pivots)))


# ----------------------------------------------------------- designed cases --

def _inverse_columns(B, R):
    E = np.zeros((B.n, len(R)))
    E[R, np.arange(len(R))] = 1.0
    return B.lu.solve(E)


def designed_case(B, R, S, C=None, same_rows=None):
    """The case on rows R (ascending), columns C (R itself, or ascending with more entries than R), whose S is the given
    one up to rounding: D = (S - I) G^-1 (G^+ when s > r), every entry of the r x s block a triplet of its own.
    same_rows = (i, j): row j of D is row i, bit for bit."""
    R = np.asarray(R)
    C = R if C is None else np.asarray(C)
    assert np.all(np.diff(R) > 0) and np.all(np.diff(C) > 0) and len(C) >= len(R)
    G = _inverse_columns(B, R)[C, :]                       # s x r
    T = np.asarray(S, dtype=np.float64) - np.eye(len(R))
    D = np.linalg.solve(G.T, T.T).T if len(C) == len(R) else T @ np.linalg.pinv(G)
    if same_rows is not None:
        D[same_rows[1]] = D[same_rows[0]]
    return np.repeat(R, len(C)), np.tile(C, len(R)), D.ravel().copy()


def cyclic_S(rng, r, shift=1, small_col=None):
    """P_cyclic (I + 0.05 N): every step k < r - 1 finds its pivot in another row (shift 1: the next one; shift -1: the
    last one).  small_col: that column times 1e-3, so that the smallest pivot falls at that step."""
    S = np.roll(np.eye(r) + 0.05 * rng.standard_normal((r, r)), shift, axis=0)
    if small_col is not None:
        S[:, small_col] *= 1e-3
    return S


# two candidates of step 0 that are the same bits (rows 1 and 2: the same row of D), larger than the other two
TIE_S = np.array([[0.5, 0.1, 0.05, -0.1],
                  [2.0, 1.3, -0.2, 0.1],
                  [2.0, 0.3, 0.8, 0.1],
                  [0.4, -0.1, 0.5, 1.1]])
RECT_SHAPES = ((1, 16), (16, 1), (3, 16), (16, 3), (2, 15))

# what a pivot case promises: swaps (None: nothing is promised), the step of the smallest pivot, rpiv about 1e-3, a tie
Designed = collections.namedtuple("Designed", "name case swaps smallest_step small tie")


def _rows(rng, n, r):
    return np.sort(rng.choice(n, size=r, replace=False))


def random_block(rng, n, r, s, scale=0.05):
    """r distinct rows x s distinct columns, every entry of the block one triplet, values scale N(0, 1): S close to I."""
    R, Cc = _rows(rng, n, r), _rows(rng, n, s)
    return np.repeat(R, s), np.tile(Cc, r), scale * rng.standard_normal(r * s)


@functools.lru_cache(maxsize=None)
def pivot_cases(n=N_PIVOT, spd=False):
    """-> [Designed] on base(n, spd)."""
    B = base(n, spd)
    rng = np.random.default_rng(7300000 + n + spd)
    out = []
    for r in RANKS:                                                        # a swap at every step, with the next row
        out.append(Designed("cyclic%d" % r, designed_case(B, _rows(rng, n, r), cyclic_S(rng, r)), r - 1, None, False, False))
    for r in (3, 8, 16):                                                   # ... with the last row
        out.append(Designed("cyclic_up%d" % r, designed_case(B, _rows(rng, n, r), cyclic_S(rng, r, -1)), r - 1, None, False, False))
    for r in (3, 5, 8, 16):                                                # the smallest pivot at an interior step
        out.append(Designed("small%d" % r, designed_case(B, _rows(rng, n, r), cyclic_S(rng, r, 1, r // 2)), r - 1, r // 2, True, False))
    R = _rows(rng, n, 5)                                                   # 5 rows x 9 columns
    Cc = np.union1d(R, rng.choice(np.setdiff1d(np.arange(n), R), size=4, replace=False))
    out.append(Designed("wide5x9", designed_case(B, R, cyclic_S(rng, 5), Cc), 4, None, False, False))
    out.append(Designed("tie4", designed_case(B, _rows(rng, n, 4), TIE_S, same_rows=(1, 2)), None, None, False, True))
    for r, s in RECT_SHAPES:
        out.append(Designed("rect%dx%d" % (r, s), random_block(rng, n, r, s), None, None, False, False))
    return out


def reference_S(B, case):
    """S of one case as updates_ref forms it."""
    rows_all = np.unique(case[0])
    return ur.capacitance(_inverse_columns(B, rows_all), rows_all, case)[3]


# ---------------------------------------------------------- structural lists --

EMPTY = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))


def light(rng, rows, scale=0.05):
    """The dense block on `rows` x `rows` with values scale N(0, 1): a healthy case with S close to I."""
    R = np.asarray(rows, dtype=np.int64)
    return np.repeat(R, len(R)), np.tile(R, len(R)), scale * rng.standard_normal(len(R) * len(R))


def width(rows, cap=MAX_TILE):
    return min(cap, -(-rows // 64) * 64)


def _ring(rng, nc, pool):
    """nc rank-2 cases; case c touches rows c mod pool and one 1 + c // pool further on: `pool` rows in all once
    nc >= pool - 1."""
    return [light(rng, sorted((c % pool, (c % pool + 1 + c // pool) % pool))) for c in range(nc)]


def _blocks16(rng, count):
    return [light(rng, range(16 * c, 16 * c + 16)) for c in range(count)]


@functools.lru_cache(maxsize=None)
def tile_lists():
    """-> {name: (cases, tiles)} on base(N_TILES); tiles: the expected rows of UpdatesPlan.tiles() -- first case, cases,
    touched rows, solve width."""
    rng = np.random.default_rng(7400000)
    L = {}
    # cases per tile: the workgroup of k_upd_apply is 512 wide up to 512 cases, then 576 ... 1024
    L["cases1"] = (_ring(rng, 1, 1100), [(0, 1, 2, 64)])
    L["cases64_rows1024"] = (_blocks16(rng, 64), [(0, 64, 1024, 1024)])    # the last case at positions 1008 .. 1023
    L["cases512_rows1024"] = ([light(rng, (2 * c, 2 * c + 1)) for c in range(512)], [(0, 512, 1024, 1024)])
    L["cases513"] = (_ring(rng, 513, 513), [(0, 513, 513, 576)])
    L["cases1024_rows1024"] = (_ring(rng, 1024, 1024), [(0, 1024, 1024, 1024)])
    L["cases1024_rows64"] = (_ring(rng, 1024, 64), [(0, 1024, 64, 64)])
    L["cases1025"] = (_ring(rng, 1025, 200), [(0, 1024, 200, 256), (1024, 1, 2, 64)])
    # touched rows per tile: 63 x 16 + 15 = 1023 rows, then the case at the boundary
    head = _blocks16(rng, 63) + [light(rng, range(1008, 1023))]
    fits = head + [light(rng, (5, 1023)), light(rng, (7, 1023))]          # one old row + one fresh: 1024; then old rows only
    L["rows1024_fits"] = (fits, [(0, 66, 1024, 1024)])
    L["rows1023_overflows"] = (head + [light(rng, (1023, 1024))], [(0, 64, 1023, 1024), (64, 1, 2, 64)])
    L["rows1024_then_fresh"] = (fits + [light(rng, (1024,))], [(0, 66, 1024, 1024), (66, 1, 1, 64)])
    mixed = [EMPTY, light(rng, (900,)), light(rng, range(40, 56)), EMPTY, light(rng, (41,)), light(rng, range(600, 1100, 32)),
             light(rng, (1099,)), EMPTY]
    L["ranks_0_1_16"] = (mixed, [(0, 8, 34, 64)])
    return L


FLAGGED_NC = 130


@functools.lru_cache(maxsize=None)
def flagged_lists():
    """-> (cases, twin, lanes) on base(N_PIVOT): one tile of FLAGGED_NC cases of which those at lanes 0, 63, 64 and
    nc - 1 are singular (updates_ref.singular_case); twin: the same list with empty cases there."""
    B = base(N_PIVOT)
    rng = np.random.default_rng(7500000)
    lanes = (0, 63, 64, FLAGGED_NC - 1)
    cases = _ring(rng, FLAGGED_NC, N_PIVOT)
    twin = list(cases)
    for k, lane in enumerate(lanes):
        cases[lane] = ur.singular_case(B.A, (3, 70, 71, N_PIVOT - 1)[k])
        twin[lane] = EMPTY
    return cases, twin, lanes


@functools.lru_cache(maxsize=None)
def row_list(n):
    """Ranks min(n, 16), 1 and (n >= 2) 2 on base(n).  The rank-1 case sits on the LAST row and, for n > 16, is the 17th
    row of its tile: at the odd width 17 the entry of Z that travels through thread 0 (row n - 1, column 16) is one it
    reads; for n = 9 at width 9 the first case does (row 8, column 8)."""
    rng = np.random.default_rng(7600000 + n)
    rk = min(n, MAX_RANK)
    first = np.arange(n) if n <= MAX_RANK else np.sort(rng.choice(n - 1, size=rk, replace=False))
    cases = [light(rng, first), light(rng, (n - 1,))]
    if n >= 2:
        cases.append(light(rng, (n // 2 - (n // 2 == n - 1), n - 1)))
    return cases


def odd_width_lists():
    """-> {name: (cases, CS3_UPD_TILE, tiles)} on base(N_PIVOT): widths 9 and 15, both odd (a tile is never narrower than
    the largest rank of its list)."""
    rng = np.random.default_rng(7700000)
    nine = [light(rng, range(0, 9)), light(rng, range(4, 13)), light(rng, (12, 20)), light(rng, range(30, 37))]
    fifteen = [light(rng, range(0, 15)), light(rng, (3,)), light(rng, (15,)), light(rng, range(20, 35))]
    return {"tile9_rank9": (nine, 9, [(0, 1, 9, 9), (1, 1, 9, 9), (2, 2, 9, 9)]),
            "tile1_rank15": (fifteen, 1, [(0, 2, 15, 15), (2, 1, 1, 15), (3, 1, 15, 15)]),
            "tile9_rank15": (fifteen, 9, [(0, 2, 15, 15), (2, 1, 1, 15), (3, 1, 15, 15)])}
