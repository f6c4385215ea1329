"""The engineered inputs of the GMRES refinement (cs3_gmres*), shared by tests/test_gmres_cpu.py and
tests/test_gpu_gmres.py.

diag_case: A0 = synth.grid_jacobian(n, seed) is what gets factorised (M), A is A0 with r diagonal entries multiplied by
`factor`: A M^-1 - I has rank r, so right-preconditioned GMRES from x0 = M^-1 b ends in exactly r iterations (r0 lies in
the range of that rank-r matrix) and in r + 1 from x0 = 0, while the stationary refinement x += M^-1 (b - A x) grows.

All CPU references use scipy's splu of A0 as the solve and tests/gmres_ref.py as the method."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_ref
from csparse3_amd import synth
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
