"""Matrices and case lists for the complex low-rank-modified solves (cs3_cplx_updates_*: csrc/cplxupd.hip), for
tests/test_cupd_cpu.py and tests/test_gpu_cupd.py.

Two families.  ACCURACY cases are networks: synth.ybus, its lossless twin and a larger one, with every single-branch
outage, pairs and triples of outages, and a Hermitian positive definite matrix with a non-Hermitian dA.  ENGINEERED cases
put the kernels at their edges on a complex analogue of update_cases.small_matrix -- banded, strictly dominant, its
diagonal running through the branches of the rotation (Re-dominant, Im-dominant, negative, tied) so that s != 1 on the
touched rows -- with a DESIGNED S: D = (S - I) G^-1 from the dense inverse, as update_cases does for the real path.  The
structural lists (tiles, flagged lanes, orders, odd widths) are update_cases' own with complex values, so that the plan
must come out as the real plan does."""
import collections
import functools

import numpy as np

import cplx_cases
import cplx_ref as ref
import update_cases as uc
from csparse3_amd import synth

RANKS = uc.RANKS
N_PIVOT, N_TILES = uc.N_PIVOT, uc.N_TILES
RECT_SHAPES = uc.RECT_SHAPES
PHASE = 0.8 + 0.6j                                         # |PHASE| = 1: a real list becomes complex without changing sizes
DIAG_PHASES = (1.0 + 0.3j, 0.3 + 1.0j, -1.0 - 0.2j, 1.0 + 1.0j)      # Re-dominant, Im-dominant, negative, tied


# ------------------------------------------------------------------ matrices --

def small_matrix(n):
    """-> (n, Ap, Ai, Az): three bands on either side with entries U(-1, 1) + j U(-1, 1); diagonal = (the row's sum of
    moduli + U(1, 2)) times DIAG_PHASES[i % 4] (each of modulus >= 1): strictly diagonally dominant by rows."""
    rng = np.random.default_rng(7800000 + n)
    A = np.zeros((n, n), dtype=np.complex128)
    for k in range(1, min(3, n - 1) + 1):
        i = np.arange(n - k)
        A[i, i + k] = rng.uniform(-1, 1, n - k) + 1j * rng.uniform(-1, 1, n - k)
        A[i + k, i] = rng.uniform(-1, 1, n - k) + 1j * rng.uniform(-1, 1, n - k)
    mag = np.abs(A).sum(axis=1) + rng.uniform(1.0, 2.0, n)
    A[np.arange(n), np.arange(n)] = mag * np.array([DIAG_PHASES[i % 4] for i in range(n)])
    return csc_of(A)


def csc_of(A):
    n = A.shape[0]
    Ap, Ai, Az = [0], [], []
    for j in range(n):
        rows = np.flatnonzero(A[:, j] != 0)
        Ai += [int(i) for i in rows]
        Az += [A[i, j] for i in rows]
        Ap.append(len(Ai))
    return n, np.array(Ap, dtype=np.int32), np.array(Ai, dtype=np.int32), np.array(Az, dtype=np.complex128)


Base = collections.namedtuple("Base", "n Ap Ai Az A inv b")


def _base(mat, seed):
    n, Ap, Ai, Az = mat
    A = ref.dense_complex(n, Ap, Ai, Az)
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for a in (Az, A, b):
        a.setflags(write=False)
    return Base(n, Ap, Ai, Az, A, np.linalg.inv(A), b)


@functools.lru_cache(maxsize=None)
def base(n):
    return _base(small_matrix(n), 7900000 + n)


ZERO_ROW = 4


@functools.lru_cache(maxsize=None)
def base_exact_zero():
    """Order 9 with row and column ZERO_ROW cut off and a_ii = 2j: s = -j, Z_ii = -0.5j in any arithmetic, and dA = -2j
    gives S = 1 + (-2j)(-0.5j) = 0 EXACTLY, on the device as in the restatement."""
    n, Ap, Ai, Az = small_matrix(9)
    A = np.array(ref.dense_complex(n, Ap, Ai, Az))
    A[ZERO_ROW, :] = 0
    A[:, ZERO_ROW] = 0
    A[ZERO_ROW, ZERO_ROW] = 2j
    return _base(csc_of(A), 7900009)


EXACT_ZERO_CASE = (np.array([ZERO_ROW]), np.array([ZERO_ROW]), np.array([-2j]))


@functools.lru_cache(maxsize=None)
def network(name):
    """ybus40, ybus40_lossless, ybus300 (rotated LU) and hermitian_pd (Cholesky, unrotated) as Base + (kind, rotate)."""
    if name == "hermitian_pd":
        return _base(cplx_cases.hermitian_pd(40, 60, seed=3), 8000003), "chol", False
    mat = {"ybus40": lambda: synth.ybus(40, 60, seed=40), "ybus40_lossless": lambda: synth.ybus(40, 60, seed=40, lossless=True),
           "ybus300": lambda: synth.ybus(300, 480, seed=300)}[name]()
    return _base(mat, 8000000 + mat[0]), "lu", True


# --------------------------------------------------------------- network cases --

def branches(A):
    """All (i, j), i < j, with a_ij and a_ji both nonzero, sorted."""
    n = A.shape[0]
    return [(i, j) for i in range(n) for j in range(i + 1, n) if A[i, j] != 0 and A[j, i] != 0]


def outage(A, i, j):
    """Branch (i, j) of an admittance matrix taken out: y = -a_ij leaves both diagonals and both off-diagonals."""
    return (np.array([i, j, i, j]), np.array([j, i, i, j]), np.array([-A[i, j], -A[j, i], A[i, j], A[j, i]]))


def merged(cases):
    return tuple(np.concatenate([c[k] for c in cases]) for k in range(3))


def outages(A):
    return [outage(A, i, j) for i, j in branches(A)]


def multiple_outages(A, count, size, seed):
    """`count` cases of `size` branches each (ranks 3 to 2 size), duplicates on shared diagonals adding."""
    rng = np.random.default_rng(seed)
    br = branches(A)
    return [merged([outage(A, *br[k]) for k in rng.choice(len(br), size=size, replace=False)]) for _ in range(count)]


def accuracy_lists(name):
    """-> (Base, cases): every single-branch outage (and, on the small networks, 12 pairs and 12 triples: ranks 3 to 6);
    on the Hermitian matrix dense non-Hermitian blocks of ranks 1 to 16."""
    B = network(name)[0]
    if name == "hermitian_pd":
        rng = np.random.default_rng(8500000)
        return B, [random_block(rng, B.n, r, s, scale=0.3) for r, s in ((1, 1), (2, 2), (3, 5), (6, 6), (16, 16))]
    lists = outages(B.A)
    if name != "ybus300":
        lists = lists + multiple_outages(B.A, 12, 2, 8600000 + B.n) + multiple_outages(B.A, 12, 3, 8700000 + B.n)
    return B, lists


# ----------------------------------------------------------- designed cases --

def designed_case(B, R, S, C=None, same_rows=None):
    """update_cases.designed_case in complex arithmetic: D = (S - I) G^-1 (G^+ when s > r), every entry a triplet."""
    R = np.asarray(R)
    C = R if C is None else np.asarray(C)
    G = B.inv[np.ix_(C, R)]                                # s x r
    T = np.asarray(S, dtype=np.complex128) - np.eye(len(R))
    D = np.linalg.solve(G.T, T.T).T if len(C) == len(R) else T @ np.linalg.pinv(G)
    if same_rows is not None:
        D[same_rows[1]] = D[same_rows[0]]
    return np.repeat(R, len(C)), np.tile(C, len(R)), D.ravel().copy()


def cyclic_S(rng, r, shift=1, small_col=None):
    """P_cyclic (I + 0.05 N), N complex: every step k < r - 1 finds its pivot in another row.  small_col: that column
    times 1e-3, so that the smallest pivot falls at that step."""
    S = np.roll(np.eye(r) + 0.05 * (rng.standard_normal((r, r)) + 1j * rng.standard_normal((r, r))), shift, axis=0)
    if small_col is not None:
        S[:, small_col] *= 1e-3
    return S


# rows 1 and 2 of S - I are the same row of D: the candidates (1, 0) and (2, 0) of step 0 are the same bits
TIE_S = np.array([[0.5 + 0.1j, 0.1, 0.05j, -0.1],
                  [2.0 + 0.5j, 1.3 + 0.2j, -0.2 + 0.1j, 0.1],
                  [2.0 + 0.5j, 0.3 + 0.2j, 0.8 + 0.1j, 0.1],
                  [0.4, -0.1j, 0.5, 1.1 + 0.1j]])
# step 0: 0.6 + 0.6j (cabs1 1.2, modulus 0.85) against 1.0 (cabs1 1.0, modulus 1.0).  By cabs1 row 1 is taken and
# rpiv = 1.2 / 2.0 = 0.6; by modulus row 0 would be, with rpiv = 1.0 / 2.0 = 0.5
CABS1_S = np.array([[1.0, 0.1], [0.6 + 0.6j, 2.0]])
CABS1_RPIV, MODULUS_RPIV = 0.6, 0.5

Designed = collections.namedtuple("Designed", "name case swaps smallest_step small tie")


def _rows(rng, n, r):
    return np.sort(rng.choice(n, size=r, replace=False))


def random_block(rng, n, r, s, scale=0.05):
    R, Cc = _rows(rng, n, r), _rows(rng, n, s)
    return np.repeat(R, s), np.tile(Cc, r), scale * (rng.standard_normal(r * s) + 1j * rng.standard_normal(r * s))


@functools.lru_cache(maxsize=None)
def pivot_cases(n=N_PIVOT):
    """-> [Designed] on base(n)."""
    B = base(n)
    rng = np.random.default_rng(8100000 + n)
    out = []
    for r in RANKS:
        out.append(Designed("cyclic%d" % r, designed_case(B, _rows(rng, n, r), cyclic_S(rng, r)), r - 1, None, False, False))
    for r in (3, 5, 8, 16):
        out.append(Designed("small%d" % r, designed_case(B, _rows(rng, n, r), cyclic_S(rng, r, 1, r // 2)), r - 1, r // 2, True, False))
    out.append(Designed("tie4", designed_case(B, _rows(rng, n, 4), TIE_S, same_rows=(1, 2)), None, None, False, True))
    out.append(Designed("cabs1", designed_case(B, _rows(rng, n, 2), CABS1_S), None, None, False, False))
    for r, s in RECT_SHAPES:
        out.append(Designed("rect%dx%d" % (r, s), random_block(rng, n, r, s), None, None, False, False))
    return out


# ---------------------------------------------------------- structural lists --

EMPTY = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.complex128))


def to_complex(case):
    return case[0], case[1], np.asarray(case[2], dtype=np.float64) * PHASE


def complex_list(cases):
    return [to_complex(c) for c in cases]


@functools.lru_cache(maxsize=None)
def tile_lists():
    """update_cases.tile_lists() with complex values, and two lists of its own: a rank-16 case in the last lanes of a
    full tile of cases, and 1024 + 1 cases whose last tile is a single rank-16 case."""
    L = {name: (complex_list(cases), tiles) for name, (cases, tiles) in uc.tile_lists().items()}
    rng = np.random.default_rng(8200000)
    ring = uc._ring(rng, 1023, 500)
    L["rank16_last_lane"] = (complex_list(ring + [uc.light(rng, range(600, 1100, 32))]), [(0, 1024, 516, 576)])
    L["rank16_alone_behind_1024"] = (complex_list(uc._ring(rng, 1024, 300) + [uc.light(rng, range(16, 32))]),
                                     [(0, 1024, 300, 320), (1024, 1, 16, 64)])
    return L


FLAGGED_NC = uc.FLAGGED_NC


def singular_case(A, i):
    """dA = -A[i, :]: rank 1, A + dA has a zero row."""
    cols = np.flatnonzero(A[i] != 0)
    return np.full(len(cols), i), cols, -A[i, cols]


@functools.lru_cache(maxsize=None)
def flagged_lists():
    """-> (cases, twin, lanes) on base(N_PIVOT): one tile of FLAGGED_NC cases of which those at lanes 0, 63, 64 and
    nc - 1 are singular; twin: the same list with empty cases there."""
    B = base(N_PIVOT)
    rng = np.random.default_rng(8300000)
    lanes = (0, 63, 64, FLAGGED_NC - 1)
    cases = complex_list(uc._ring(rng, FLAGGED_NC, N_PIVOT))
    twin = list(cases)
    for k, lane in enumerate(lanes):
        cases[lane] = singular_case(B.A, (3, 70, 71, N_PIVOT - 1)[k])
        twin[lane] = EMPTY
    return cases, twin, lanes


def row_orders(lim):
    """n = 1 and one below / at / one above the stage and the row block of k_cupd_apply."""
    st, rb = int(lim.apply_stage), int(lim.apply_rows)
    return sorted({1, st - 1, st, st + 1, rb - 1, rb, rb + 1, 2 * rb + st + 1})


def row_list(n):
    return complex_list(uc.row_list(n))


def odd_width_lists():
    return {name: (complex_list(cases), env, tiles) for name, (cases, env, tiles) in uc.odd_width_lists().items()}


def nan_lists():
    """A rank-3 and a rank-16 case with one NaN value (real or imaginary part) in the first or the last row, between
    healthy neighbours.  -> [(cases, index of the poisoned case)]."""
    rng = np.random.default_rng(8400000)
    out = []
    for rows in (range(10, 13), range(40, 56)):
        for where in (0, -1):
            for part in (complex(np.nan, 0.0), complex(0.0, np.nan)):
                bad = to_complex(uc.light(rng, rows))
                vals = np.array(bad[2])
                vals[where] = vals[where] + part
                cases = complex_list(uc._ring(rng, 5, N_PIVOT))
                cases.insert(2, (bad[0], bad[1], vals))
                out.append((cases, 2))
    return out
