"""The engineered inputs of the GMRES refinement (cs3_gmres*), shared by tests/test_gmres_cpu.py and
tests/test_gpu_gmres.py.

diag_case: A0 = synth.grid_jacobian(n, seed) is what gets factorised (M), A is A0 with r diagonal entries multiplied by
`factor`: A M^-1 - I has rank r, so right-preconditioned GMRES from x0 = M^-1 b ends in exactly r iterations (r0 lies in
the range of that rank-r matrix) and in r + 1 from x0 = 0, while the stationary refinement x += M^-1 (b - A x) grows.

All CPU references use scipy's splu of A0 as the solve and tests/gmres_ref.py as the method.

The second half (spread_case and below) holds the deep cases of tests/test_gmres_cases_cpu.py and
tests/test_gpu_gmres_edges.py."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_ref
from csparse3_amd import csc_hip, synth
from helpers import rel_err
from perturb_cases import tiny  # noqa: F401  (the engineered tiny pivot of the perturbation tests, for the public path)

DiagCase = namedtuple("DiagCase", "mat Ax rows b A0 A")
# mat: (m, n, Ap, Ai, Ax0); Ax: the values of A; rows: the scaled diagonal entries; A0, A: scipy CSC

_CACHE = {}


def tridiagonal(n, seed):
    """A diagonally dominant tridiagonal matrix of any order n >= 1 (grid_jacobian needs more rows than its offsets)."""
    rng = np.random.default_rng(seed)
    lo, up = -rng.uniform(0.1, 1.0, max(n - 1, 0)), -rng.uniform(0.1, 1.0, max(n - 1, 0))
    d = np.ones(n)
    d[:-1] += np.abs(up)
    d[1:] += np.abs(lo)
    A = sp.diags([lo, d, up], [-1, 0, 1], shape=(n, n), format="csc") if n > 1 else sp.csc_matrix(d.reshape(1, 1))
    A.sort_indices()
    return n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def scale_diagonal(mat, rows, factor):
    """The values of `mat` with the diagonal entries `rows` multiplied by factor."""
    m, n, Ap, Ai, Ax = mat
    Ax2 = np.array(Ax, dtype=np.float64, copy=True)
    for i in rows:
        p = [p for p in range(Ap[i], Ap[i + 1]) if Ai[p] == i]
        assert len(p) == 1, "row %d has no stored diagonal entry" % i
        Ax2[p[0]] *= factor
    return Ax2


def to_scipy(mat, Ax=None):
    m, n, Ap, Ai, Ax0 = mat
    return sp.csc_matrix((np.asarray(Ax0 if Ax is None else Ax, dtype=np.float64), Ai, Ap), shape=(m, n))


def diag_case(n, seed, r, factor=4.0, mat=None):
    """grid_jacobian(n, seed) (or `mat`) with r chosen diagonal entries multiplied by factor, and one right-hand side."""
    key = ("diag", n, seed, r, factor, mat is None)
    if key not in _CACHE or mat is not None:
        base = synth.grid_jacobian(n=n, seed=seed) if mat is None else mat
        rng = np.random.default_rng(1000 * seed + r)
        rows = np.sort(rng.choice(base[1], size=r, replace=False))
        Ax = scale_diagonal(base, rows, factor)
        b = rng.standard_normal(base[1])
        case = DiagCase(base, Ax, rows, b, to_scipy(base), to_scipy(base, Ax))
        if mat is not None:
            return case
        _CACHE[key] = case
    return _CACHE[key]


def reference(case, x0=None, rtol=1e-12, restart=30, max_iters=100, trans=False, b=None):
    """tests/gmres_ref.py on a DiagCase with splu(A0) as the solve; x0=None: from M^-1 b."""
    lu = spla.splu(case.A0.tocsc())
    solve = (lambda v: lu.solve(v, trans="T")) if trans else lu.solve
    A = case.A.T.tocsr() if trans else case.A.tocsr()
    b = case.b if b is None else b
    return gmres_ref.gmres(A, solve, b, solve(b) if x0 is None else x0, rtol, restart, max_iters)


def stationary_corrections(case, rounds=6):
    """max |dx| of `rounds` rounds of x += M^-1 (b - A x) from x = M^-1 b."""
    lu = spla.splu(case.A0.tocsc())
    x, out = lu.solve(case.b), []
    for _ in range(rounds):
        d = lu.solve(case.b - case.A @ x)
        out.append(float(np.abs(d).max()))
        x = x + d
    return out


RESTART_CASES = [(3, 2), (5, 3)]              # (r, restart) on diag_case(300, 7, r)

RestartCase = namedtuple("RestartCase", "case restart rtol iters history ref")


def restart_case(r, restart):
    """diag_case(300, 7, r) under GMRES(restart): the reference's history at rtol = 1e-12, then the test's rtol = the
    geometric mean of the LAST two consecutive history values at least 10 x apart (rounding cannot move the count), and
    the reference at that rtol."""
    key = ("restart", r, restart)
    if key not in _CACHE:
        case = diag_case(300, 7, r)
        full = reference(case, rtol=1e-12, restart=restart, max_iters=100)
        h = full.history
        gaps = [i for i in range(len(h) - 1) if h[i + 1] > 0.0 and h[i] >= 10.0 * h[i + 1]]
        assert gaps, "no two consecutive residuals 10 x apart: %r" % (h,)
        i = gaps[-1]
        rtol = float(np.sqrt(h[i] * h[i + 1]))
        ref = reference(case, rtol=rtol, restart=restart, max_iters=100)
        _CACHE[key] = RestartCase(case, restart, rtol, ref.iters, h, ref)
    return _CACHE[key]


def recurrence_gap(cycles):
    """max over the cycles of |estimate - true| (both relative to ||b||): how far the recurrence's residual is from the
    true one at a cycle's end."""
    return max([abs(e - t) for e, t in cycles] or [0.0])


def reference_gap():
    """The reference's own recurrence_gap over the three finite-termination cases and the two restart cases."""
    if "gap" not in _CACHE:
        gaps = [recurrence_gap(reference(diag_case(300, 7, r)).cycles) for r in (1, 3, 5)]
        gaps += [recurrence_gap(restart_case(r, m).ref.cycles) for r, m in RESTART_CASES]
        _CACHE["gap"] = max(gaps)
    return _CACHE["gap"]


MixedBatch = namedtuple("MixedBatch", "mat AX B cases")


def mixed_batch():
    """Three matrices x k = 2 on the pattern of grid_jacobian(300, 7): matrix 0 is A0 itself, matrix 1 has r = 1, matrix 2
    r = 5.  AX [3, nnz], B [3, n, 2]; cases[b]: the DiagCase behind matrix b (b = 0: r = 0)."""
    if "mixed" not in _CACHE:
        c1, c5 = diag_case(300, 7, 1), diag_case(300, 7, 5)
        mat = c1.mat
        c0 = DiagCase(mat, np.array(mat[4], copy=True), np.zeros(0, dtype=np.int64), c1.b, c1.A0, c1.A0)
        cases = [c0, c1, c5]
        rng = np.random.default_rng(77)
        B = rng.standard_normal((3, mat[1], 2))
        AX = np.stack([c.Ax for c in cases])
        _CACHE["mixed"] = MixedBatch(mat, AX, B, cases)
    return _CACHE["mixed"]


# ---- deep cases (tests/test_gmres_cases_cpu.py, tests/test_gpu_gmres_edges.py) ----------------------------------------
# diag_case's single factor clusters the eigenvalues of A M^-1 and GMRES ends early whatever r is.  spread_case gives
# every chosen row a factor of its own, lo + q: r distinct eigenvalues, so the residual falls smoothly over about r
# iterations and an iteration cap m with rtol = 0 decides the count: x after exactly m iterations is the target.

def spread_case(n, seed, r, lo=2.0, mat=None):
    """diag_case with the q-th chosen diagonal entry multiplied by lo + q."""
    key = ("spread", n, seed, r, lo, mat is None)
    if key not in _CACHE or mat is not None:
        base = synth.grid_jacobian(n=n, seed=seed) if mat is None else mat
        rng = np.random.default_rng(1000 * seed + r)
        rows = np.sort(rng.choice(base[1], size=r, replace=False))
        Ax = np.array(base[4], dtype=np.float64, copy=True)
        for q, i in enumerate(rows):
            Ax = scale_diagonal((base[0], base[1], base[2], base[3], Ax), [i], lo + q)
        b = rng.standard_normal(base[1])
        case = DiagCase(base, Ax, rows, b, to_scipy(base), to_scipy(base, Ax))
        if mat is not None:
            return case
        _CACHE[key] = case
    return _CACHE[key]


def capped(case, m, restart=32, b=None, trans=False, keep_basis=False, solve=None):
    """The reference after exactly m iterations (rtol = 0) from x0 = M^-1 b; solve=None: splu of A0.  Cached for the
    case's own b and splu, and for any b given as (key, vector)."""
    bkey, b = (None, case.b) if b is None else b
    key = ("capped", id(case), m, restart, bkey, trans, keep_basis)
    if solve is not None or key not in _CACHE:
        if solve is None:
            lu = spla.splu(case.A0.tocsc())
            sv = (lambda v: lu.solve(v, trans="T")) if trans else lu.solve
        else:
            sv = solve
        A = case.A.T.tocsr() if trans else case.A.tocsr()
        res = gmres_ref.gmres(A, sv, b, sv(b), 0.0, restart, m, keep_basis=keep_basis)
        if solve is not None:
            return res
        _CACHE[key] = res
    return _CACHE[key]


def rel_diff(a, b):
    """max |a - b| / max |b|: helpers.rel_err, the measure the GPU tests assert on."""
    return rel_err(a, b)


def variant_bound(cases_and_caps):
    """How far two CPU variants of the same method are apart: splu of A0 as the solve, and inv(A0.toarray()) @ v.  For
    every (case, m) or (case, m, restart) both run m iterations at rtol = 0 (restart 32 unless given); -> the maxima of
    (the relative difference of x, the absolute difference of relres, recurrence_gap of either)."""
    dx = dres = gap = 0.0
    inverses = {}
    for item in cases_and_caps:
        case, m = item[0], item[1]
        restart = item[2] if len(item) > 2 else 32
        if id(case) not in inverses:
            inverses[id(case)] = np.linalg.inv(case.A0.toarray())
        inv = inverses[id(case)]
        a = capped(case, m, restart)
        c = capped(case, m, restart, solve=lambda v: inv @ v)
        dx = max(dx, rel_diff(a.x, c.x))
        dres = max(dres, abs(a.relres - c.relres))
        gap = max(gap, recurrence_gap(a.cycles), recurrence_gap(c.cycles))
    return dx, dres, gap


def basis_defect(V):
    """max |V' V - I| over the columns of V."""
    V = np.asarray(V, dtype=np.float64)
    return float(np.abs(V.T @ V - np.eye(V.shape[1])).max())


# What the GPU tests run, named here so that the CPU test checks the same inputs.
DEEP_CAPS = [8, 9, 16, 17, 24, 25, 31, 32, 33, 41]        # max_iters at restart 32: the passes of 8, the full cycle, beyond
BOUNDARY_RESTARTS = [8, 9]                                # restart at the pass boundary, max_iters = 2 restart + 1
TILE_CASES = [(5, 17), (8, 17), (8, 32), (8, 33), (9, 17), (16, 17), (17, 17), (17, 33), (32, 17), (33, 17), (33, 33)]  # (k, m)
X_FLOOR = 1e-13                                           # the factors on the GPU are not splu's


def deep_case():
    return spread_case(300, 7, 40)


def tile_rhs(k):
    """B [300, k] of the tile-width test (the CPU test checks every column's separation at the depths used)."""
    return np.random.default_rng(k).standard_normal((300, k))


def grid_cases(chunk_rows, rhs_tile):
    """Two matrices of n = chunk_rows + 1 (lo = 2 and 3) and B [2, n, rhs_tile + 1]: chunks, tiles and batch all 2."""
    n, k = chunk_rows + 1, rhs_tile + 1
    key = ("grid", n, k)
    if key not in _CACHE:
        cases = [spread_case(n, 7, 40), spread_case(n, 7, 40, lo=3.0)]
        _CACHE[key] = (cases, np.random.default_rng(n + k).standard_normal((2, n, k)))
    return _CACHE[key]


EdgeBounds = namedtuple("EdgeBounds", "x relres gap ref_x ref_relres ref_gap")


def edge_bounds():
    """The bounds of the GPU edge tests: 10 x the figures of variant_bound over every single-system (case, cap, restart)
    those tests use (x floored at X_FLOOR), and the reference's figures themselves."""
    if "edge_bounds" not in _CACHE:
        c = deep_case()
        runs = [(c, m) for m in DEEP_CAPS] + [(c, 2 * r + 1, r) for r in BOUNDARY_RESTARTS]
        lim = csc_hip.gmres_limits()
        runs += [(g, 17) for g in grid_cases(lim.chunk_rows, lim.rhs_tile)[0]]
        dx, dres, gap = variant_bound(runs)
        _CACHE["edge_bounds"] = EdgeBounds(max(10.0 * dx, X_FLOOR), 10.0 * dres, 10.0 * gap, dx, dres, gap)
    return _CACHE["edge_bounds"]


def reference_basis_defect():
    """max |V' V - I| of the reference's basis at depth 32 (deep_case, one full cycle)."""
    if "defect" not in _CACHE:
        res = capped(deep_case(), 32, keep_basis=True)
        assert res.V.shape[1] == 32 and res.ncols == 32
        _CACHE["defect"] = basis_defect(res.V)
    return _CACHE["defect"]


FreezeBatch = namedtuple("FreezeBatch", "mat AX B cases rtol refs r")


def freeze_batch():
    """Three matrices x k = 2 on the pattern of grid_jacobian(300, 7) under GMRES(32), max_iters = 32: matrix 0 is the
    spread case of the r nearest 12 in 10 .. 14 whose two systems both have, at the same place, two consecutive history
    values 10 x apart and freeze there; matrix 1 the r = 40 spread case (runs to the cap); matrix 2 A0 itself with a zero
    second column.  rtol as in restart_case, from the histories of matrix 0: the geometric mean of the larger lower and
    the smaller upper value.  refs[s]: the reference of system s = 2 b + t at that rtol, with its basis."""
    if "freeze" not in _CACHE:
        c40 = deep_case()
        mat = c40.mat
        n = mat[1]
        B = np.random.default_rng(78).standard_normal((3, n, 2))
        B[2, :, 1] = 0.0
        c0 = DiagCase(mat, np.array(mat[4], copy=True), np.zeros(0, dtype=np.int64), c40.b, c40.A0, c40.A0)
        picked = None
        for r in (12, 11, 13, 10, 14):
            c = spread_case(n, 7, r)
            hs = [reference(c, b=B[0, :, t], rtol=1e-12, restart=32, max_iters=32).history for t in range(2)]
            where = []
            for h in hs:
                gaps = [i for i in range(len(h) - 1) if h[i + 1] > 0.0 and h[i] >= 10.0 * h[i + 1]]
                where.append(gaps[-1] if gaps else None)
            if where[0] is not None and where[0] == where[1]:
                i = where[0]
                upper, lower = min(h[i] for h in hs), max(h[i + 1] for h in hs)
                if upper >= 10.0 * lower:
                    picked = (r, c, float(np.sqrt(upper * lower)))
                    break
        assert picked, "no r in 10 .. 14 has a 10 x gap shared by both systems"
        r, c, rtol = picked
        cases = [c, c40, c0]
        refs = []
        for b in range(3):
            lu = spla.splu(cases[b].A0.tocsc())
            for t in range(2):
                v = B[b, :, t]
                refs.append(gmres_ref.gmres(cases[b].A.tocsr(), lu.solve, v, lu.solve(v), rtol, 32, 32, keep_basis=True))
        _CACHE["freeze"] = FreezeBatch(mat, np.stack([x.Ax for x in cases]), B, cases, rtol, refs, r)
    return _CACHE["freeze"]
