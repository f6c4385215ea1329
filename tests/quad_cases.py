"""The cases of the tests of the bilinear forms on the selected inverse (tests/test_quad_cpu.py, tests/test_gpu_quad.py).
Every size that is meant to sit at an edge of a kernel comes from cs3_quad_limits(); nothing here needs a GPU.

A case is a dict: "matrix" (m, n, Ap, Ai, Ax) as csparse3_amd.synth returns it, "kind", "Ct" = (m, indptr, indices) the rows
of C, "Bt" the rows of B or None (B = C), "Cx", "Bx" (None when B = C) the values.  The long rows sit on a dense matrix,
where any pair of columns is on the pattern.  The kernels have no grid cap, so there is no case past one; the reduction of
the normalised residuals changes path where the closing workgroup takes a second partial per thread (reduce_rows * block
rows), and normres_long() is one row past that.
"""
import functools

import numpy as np

import selinv_cases as sc
from csparse3_amd import csc_hip as hip
from csparse3_amd import synth

LIMITS = hip.quad_limits()
ND = 48                                         # order of the dense matrix: rows of up to ND * ND terms


@functools.lru_cache(maxsize=None)
def dense_matrix():
    case = synth.dense_block_matrix(ND, ND, 1)
    assert int(case[2][ND]) == ND * ND
    return case


def _rows(lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    idx = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return (len(lists), ptr, idx)


def _values(rng, operand):
    return rng.uniform(0.5, 2.0, size=len(operand[2])) * rng.choice([-1.0, 1.0], size=len(operand[2]))


def _split(nt, nmax=ND):
    """(nc, nb) with nc * nb == nt, both at most nmax, nc the smallest such factor; a count without such factors (a prime
    beyond nmax): (1, nt), a row of b that holds columns more than once."""
    for nc in range(1, nmax + 1):
        if nt % nc == 0 and nt // nc <= nmax:
            return nc, nt // nc
    return 1, nt


def edge_term_counts():
    """Term counts at each class edge and one past it, 63 / 64 / 65, 0 and 1, and the longest row of the dense matrix."""
    L = LIMITS
    counts = [0, 1, int(L.lane_chunk), int(L.lane_chunk) + 1, int(L.lane_max_terms), int(L.lane_max_terms) + 1, 63, 64, 65,
              int(L.block) - 1, int(L.block), int(L.block) + 1, int(L.wave_max_terms), int(L.wave_max_terms) + 1, 2 * ND * ND // 3,
              ND * ND]
    assert L.wave_max_terms + 1 <= ND * ND
    return counts


def _draw(rng, k):
    """k column indices of the dense matrix, unsorted, without repeats while k allows it."""
    return rng.permutation(ND)[:k] if k <= ND else rng.integers(0, ND, size=k)


@functools.lru_cache(maxsize=None)
def two_operands():
    """B with a pattern of its own: one row per edge_term_counts() entry (nc x nb terms, unsorted indices), a row with an
    empty c and a row with an empty b, a row with a repeated column on either side."""
    rng = np.random.default_rng(11)
    c_rows, b_rows = [], []
    for nt in edge_term_counts():
        nc, nb = (0, 0) if nt == 0 else _split(nt)
        c_rows.append(_draw(rng, nc)); b_rows.append(_draw(rng, nb))
    c_rows += [[], [3, 1, 4], [5, 5, 7]]
    b_rows += [[2, 7], [], [2, 9, 2]]
    Ct, Bt = _rows(c_rows), _rows(b_rows)
    return {"matrix": dense_matrix(), "kind": hip.CS3_LU, "Ct": Ct, "Bt": Bt, "Cx": _values(rng, Ct), "Bx": _values(rng, Bt)}


@functools.lru_cache(maxsize=None)
def one_operand():
    """B = C: rows of k entries (k * k terms) for k = 0 .. 7, around sqrt of the class edges, 48; a repeated column; unsorted."""
    rng = np.random.default_rng(12)
    L = LIMITS
    ks = sorted(set(list(range(0, 9)) + [int(np.sqrt(L.wave_max_terms)), int(np.sqrt(L.wave_max_terms)) + 1, ND]))
    assert any(k * k == L.wave_max_terms for k in ks) and any(L.lane_max_terms < k * k <= L.wave_max_terms for k in ks)
    rows = [_draw(rng, k) for k in ks] + [[6, 2, 6], [9, 9]]
    Ct = _rows(rows)
    return {"matrix": dense_matrix(), "kind": hip.CS3_LU, "Ct": Ct, "Bt": None, "Cx": _values(rng, Ct), "Bx": None}


def single_row():
    """m = 1."""
    rng = np.random.default_rng(13)
    Ct = _rows([[4, 1, 30]])
    return {"matrix": dense_matrix(), "kind": hip.CS3_LU, "Ct": Ct, "Bt": None, "Cx": _values(rng, Ct), "Bx": None}


def class_sizes():
    """(lane rows, wave rows) around the rows one workgroup takes of each class."""
    return [(int(LIMITS.block) + d, 4 + d) for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def class_rows(n_lane, n_wave):
    """n_lane lane rows of 0 to 3 entries, n_wave wave rows of 7 entries, 2 workgroup rows of 33, interleaved, B = C."""
    rng = np.random.default_rng(n_lane)
    assert 3 * 3 <= LIMITS.lane_max_terms < 7 * 7 <= LIMITS.wave_max_terms < 33 * 33
    sizes = [int(k) for k in rng.integers(0, 4, size=n_lane)] + [7] * n_wave + [33] * 2
    rows = [_draw(rng, sizes[i]) for i in rng.permutation(len(sizes))]
    Ct = _rows(rows)
    return {"matrix": dense_matrix(), "kind": hip.CS3_LU, "Ct": Ct, "Bt": None, "Cx": _values(rng, Ct), "Bx": None}


def batch_values(case, nb=3):
    """Values of their own for every matrix of a batch: (AX [nb, nnz], CX [nb, nnz_c], BX or None)."""
    rng = np.random.default_rng(17)
    Ax = case["matrix"][4]
    scale = lambda x: np.stack([x * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=len(x))) for _ in range(nb)])
    n = case["matrix"][1]
    cols = np.repeat(np.arange(n), np.diff(case["matrix"][2]))
    AX = scale(Ax)
    AX[:, case["matrix"][3] == cols] = Ax[case["matrix"][3] == cols] * 1.25      # (the diagonal stays dominant)
    return AX, scale(case["Cx"]), None if case["Bx"] is None else scale(case["Bx"])


def _incidence(case):
    """One row (+1 at i, -1 at j) per stored pair i < j of a structurally symmetric matrix."""
    n, Ap, Ai = case[1], case[2], case[3]
    cols = np.repeat(np.arange(n), np.diff(Ap))
    rows = np.asarray(Ai[:int(Ap[n])])
    keep = rows < cols
    i, j = rows[keep], cols[keep]
    Ct = (len(i), (2 * np.arange(len(i) + 1)).astype(np.int32), np.stack([i, j], axis=1).ravel().astype(np.int32))
    return Ct, np.tile([1.0, -1.0], len(i))


def incidence(name):
    """An incidence matrix as C (B = C) on jacobian_like and on a tridiagonal matrix: Z_ii + Z_jj - Z_ij - Z_ji per branch."""
    matrix = {"jacobian_like": synth.jacobian_like()[:5], "tridiagonal": sc.tridiagonal(40)}[name]
    Ct, Cx = _incidence(matrix)
    return {"matrix": matrix, "kind": hip.CS3_LU, "Ct": Ct, "Bt": None, "Cx": Cx, "Bx": None}


def csc_rows(m, n, Ap, Ai, Ax):
    """The rows of a CSC matrix (m x n): ((m, indptr, indices), values, entry order), a stable transpose on the host."""
    nz = int(Ap[n])
    rows, cols = np.asarray(Ai[:nz]), np.repeat(np.arange(n), np.diff(Ap))
    order = np.argsort(rows, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return (m, ptr, cols[order].astype(np.int32)), np.asarray(Ax[:nz], dtype=np.float64)[order]


SE_SEEDS = {(40, 60): 40, (300, 480): 300}
CRIT_TOL = 1e-8                                 # what the GPU test passes; test_quad_cpu.py checks the cases against it


@functools.lru_cache(maxsize=None)
def se(nbus, nedges):
    """synth.se_case with its gain matrix G = H' W H on the structural pattern of H' H (Cholesky), the rows of H as C.
    Extra keys: "H" dense, "w", "critical_rows"."""
    m, n, Hp, Hi, Hx, w, crit = synth.se_case(nbus, nedges, SE_SEEDS[(nbus, nedges)])
    H = np.zeros((m, n))
    H[Hi, np.repeat(np.arange(n), np.diff(Hp))] = Hx
    G = H.T @ (w[:, None] * H)
    pattern = ((H != 0).astype(np.int64).T @ (H != 0).astype(np.int64)) > 0
    gi, gj = np.nonzero(pattern.T)                               # column-major
    gi, gj = gj, gi
    Gp = np.concatenate([[0], np.cumsum(np.bincount(gj, minlength=n))]).astype(np.int32)
    matrix = (n, n, Gp, gi.astype(np.int32), G[gi, gj])
    Ct, Cx = csc_rows(m, n, Hp, Hi, Hx)
    return {"matrix": matrix, "kind": hip.CS3_CHOLESKY, "Ct": Ct, "Bt": None, "Cx": Cx, "Bx": None, "H": H, "w": w,
            "critical_rows": crit}


@functools.lru_cache(maxsize=None)
def normres_long():
    """One row past reduce_rows * block rows: unit rows e_(i mod n) on a tridiagonal matrix, so that thread 0 of the closing
    workgroup takes two partials.  Extra keys: "w", "r" (any positive weights, any residuals: the arithmetic is what is
    tested)."""
    rng = np.random.default_rng(19)
    matrix = sc.tridiagonal(40)
    m = int(LIMITS.reduce_rows * LIMITS.block) + 1
    Ct = (m, np.arange(m + 1, dtype=np.int32), (np.arange(m) % matrix[1]).astype(np.int32))
    return {"matrix": matrix, "kind": hip.CS3_LU, "Ct": Ct, "Bt": None, "Cx": rng.uniform(0.5, 1.5, size=m), "Bx": None,
            "w": rng.uniform(0.1, 1.0, size=m), "r": rng.standard_normal(m)}


def form_cases():
    """name -> case for the tests of plan, accuracy and bits."""
    cases = {"two_operands": two_operands(), "one_operand": one_operand(), "single_row": single_row(),
             "incidence_jacobian_like": incidence("jacobian_like"), "incidence_tridiagonal": incidence("tridiagonal"),
             "se_40_60": se(40, 60), "se_300_480": se(300, 480)}
    for n_lane, n_wave in class_sizes():
        cases["classes_%d_%d" % (n_lane, n_wave)] = class_rows(n_lane, n_wave)
    return cases


def analysed(case, batch=1):
    m = case["matrix"]
    return hip.Factorization(m[0], m[1], m[2], m[3], case["kind"], batch=batch)
