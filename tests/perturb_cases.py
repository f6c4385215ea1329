"""Static pivot perturbation: the CPU reference and the engineered cases shared by tests/test_perturb_cpu.py and
tests/test_gpu_perturb.py.

The rule under test (include/csparse3_amd.h): an LU pivot p with |p| < delta is replaced by +delta.  The factors are then
those of A(q, q) + diag(E), E_kk = delta - p_k at the replaced pivots and 0 elsewhere.

reference() finds E with the CPU oracle alone: factor at tol = 0, take the first k with |U_kk| < delta, add delta - U_kk
to A's entry (q[k], q[k]), factor again -- everything before k is untouched, so the perturbed set grows front to back as
it does in the kernels.  A corrected pivot comes out as delta only to the rounding of the cancellation that forms it:
A's entry moves in steps of its own ulp, which is coarser than delta's, so U_kk == delta holds to PIVOT_SLACK u (|L||U|)_kk
and not bit for bit.  A corrected pivot that this rounding leaves just below delta is corrected again (same k, a further
round).

The matrices are those of tests/pivot_cases.py: tiny() puts a pivot of relative size rho = 1e-4 .. 1e-10 at one of its
targets, in every kernel class."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import pivot_cases as pc
from helpers import U_ROUND, backward_error_ratio, canon, permuted

MAX_ROUNDS = 8
C_BOUND = 4.0                 # |L U - A(q, q) - diag(E)|_ij <= C_BOUND k u (|L||U|)_ij, k = the largest column count of L
PIVOT_SLACK = 4.0             # |U_kk - delta| <= PIVOT_SLACK u (|L||U|)_kk at a corrected pivot: the rounding of the corrected
                              # entry of A, of the last subtraction and of delta - U_kk itself, and one to spare

Reference = namedtuple("Reference", "perturbed E Ax factors rounds")


class TooManyRounds(Exception):
    """reference() would need more than MAX_ROUNDS corrections (a cascade of small pivots): not a case for these tests."""


def diag_of_u(n, Up, Ux):
    """U_kk for every k (the oracle keeps the diagonal last in each column)."""
    return np.asarray(Ux)[np.asarray(Up[1:n + 1]) - 1]


def reference(orc, mat, q, delta):
    """-> Reference(perturbed: sorted pivot indices, E [n] in pivot order, Ax: the corrected values, factors: the oracle's
    (Lp, Li, Lx, Up, Ui, Ux) of the corrected matrix in the order q, rounds)."""
    m, n, Ap, Ai, Ax = mat
    Ax2 = np.array(Ax, dtype=np.float64, copy=True)
    q = np.asarray(q)
    hit = set()
    for rounds in range(1, MAX_ROUNDS + 2):
        L = orc.csc_lu_f(n, n, Ap, Ai, Ax2, q, 0.0)
        assert np.array_equal(L[6], np.argsort(q)), "tol = 0 keeps every diagonal"
        d = diag_of_u(n, L[3], L[5])
        small = np.flatnonzero(np.abs(d) < delta)
        if len(small) == 0:
            break
        if rounds > MAX_ROUNDS:
            raise TooManyRounds("more than %d rounds" % MAX_ROUNDS)
        k = int(small[0])
        p = pc._entry(Ap, Ai, q[k], q[k])
        assert p >= 0, "pivot %d has no stored diagonal entry" % k
        Ax2[p] += delta - d[k]
        hit.add(k)
    E = np.zeros(n)
    for k in hit:
        p = pc._entry(Ap, Ai, q[k], q[k])
        E[k] = Ax2[p] - Ax[p]
    return Reference(np.array(sorted(hit), dtype=np.int64), E, Ax2, tuple(L[:6]), rounds - 1)


def max_column_count(n, Lp):
    return int(np.diff(np.asarray(Lp[:n + 1])).max())


def abs_product_diagonal(n, L, U):
    """(|L||U|)_kk for every k."""
    Lp, Li, Lx = canon(n, *L)
    Up, Ui, Ux = canon(n, *U)
    Lm = abs(sp.csc_matrix((Lx, Li, Lp), shape=(n, n))).tocsr()
    Um = abs(sp.csc_matrix((Ux, Ui, Up), shape=(n, n))).tocsc()
    return np.asarray(Lm.multiply(Um.T).sum(axis=1)).ravel()


def bound_ratio(n, Ap, Ai, Ax_corrected, q, L, U):
    """max |L U - (A(q, q) + diag(E))|_ij / (k u (|L||U|)_ij), and the entries outside the pattern of |L||U|: the
    corrected values ARE A + diag(E), so the comparison needs no E of its own."""
    ratio, nz_bad = backward_error_ratio(n, permuted(n, Ap, Ai, Ax_corrected, q), L, U)
    return ratio / max_column_count(n, canon(n, *L)[0]), nz_bad


Tiny = namedtuple("Tiny", "target rho Ax u M weight")


def tiny(orc, case, target, rho):
    """The case's matrix with a pivot of relative size rho at `target` (pivot_cases.engineer_lu): -> Tiny(target, rho,
    Ax, u: the oracle's pivot there at tol = 0, M: the largest entry of the unnormalised column below it, weight)."""
    assert 1e-10 <= rho <= 1e-4
    m, n, Ap, Ai, Ax = case["mat"]
    q = case["FR"].q
    Ax2, _, weight = pc.engineer_lu(orc, n, Ap, Ai, Ax, q, target.k, rho, target.i)
    Lp, Li, Lx, Up, Ui, Ux, _ = orc.csc_lu_f(n, n, Ap, Ai, Ax2, q, 0.0)
    u = float(diag_of_u(n, Up, Ux)[target.k])
    M = float(np.abs(pc.column_of_l(Lp, Li, Lx, target.k)[1]).max() * abs(u))
    return Tiny(target, rho, Ax2, u, M, weight)


RHO_THRESHOLD = 1e-4          # test 1: the largest rho allowed, so that the pivot's weight stays above DECISION_WEIGHT
RHO_TINY = 1e-10              # test 2
DELTA_OF_M = 1e-3             # test 2: delta = 1e-3 M

CLASSES = [(name, cls) for name, classes in pc.LU_CASES.items() for cls in classes]
IDS = ["%s-b%d-%s" % (nm[0], nm[1], c) for nm, c in CLASSES]
_NEAR = ("near", "diag")
_FAR = ("far", "stacked", "tile", "tail", "contrib")
_PICKED = {}


def picked(hip, orc, name, cls):
    """At most two targets of pivot_cases.lu_targets for one kernel class, one with the column's maximum near the pivot
    and one with it far from it (or in the stacked rows), where the class has both: the first "near" target and the
    last "far" one of the target list (an early and a late pivot of their fronts) for which
      * the weight at RHO_THRESHOLD stays above pivot_cases.DECISION_WEIGHT (the threshold test decides at 1e-6), and
      * the CPU reference at RHO_TINY, delta = DELTA_OF_M M perturbs the engineered pivot alone and leaves every other
        |U_jj| >= 10 delta (only the engineered pivot decides).
    -> [(Tiny at RHO_THRESHOLD, Tiny at RHO_TINY, Reference at RHO_TINY)]"""
    if (name, cls) not in _PICKED:
        case = pc.lu_case(hip, orc, name)
        m, n, Ap, Ai, Ax = case["mat"]
        q = case["FR"].q
        out, kinds = [], set()
        mine = [p.target for p in case["targets"] if p.target.cls == cls]
        # (near: from the front of the list; far: from its end -- a late pivot of the front, past its block and wave edges)
        for t in [t for t in mine if t.where in _NEAR] + [t for t in mine[::-1] if t.where in _FAR]:
            kind = "near" if t.where in _NEAR else "far"
            if kind in kinds:
                continue
            lo = tiny(orc, case, t, RHO_THRESHOLD)
            if lo.weight < pc.DECISION_WEIGHT:
                continue
            hi = tiny(orc, case, t, RHO_TINY)
            try:
                ref = reference(orc, (m, n, Ap, Ai, hi.Ax), q, DELTA_OF_M * hi.M)
            except TooManyRounds:
                continue
            d = np.abs(diag_of_u(n, ref.factors[3], ref.factors[5]))
            others = np.delete(d, t.k)
            if list(ref.perturbed) != [t.k] or others.min() < 10 * DELTA_OF_M * hi.M:
                continue
            kinds.add(kind)
            out.append((lo, hi, ref))
            if len(out) == 2:
                break
        _PICKED[name, cls] = out
    return _PICKED[name, cls]


BATCH_SLOTS = {20: (7, 19), 50: (31,), 130: (63, 64)}       # where the engineered matrix sits, per target in turn


def batch_values(Ax, batch, seed):
    """The benign original, scaled, once per matrix of the batch (the threshold test's _batch_values)."""
    if batch == 1:
        return np.array(Ax, copy=True)
    scale = 1.0 + np.random.default_rng(seed).uniform(0.0, 1.0, size=(batch, 1))
    return Ax[None, :] * scale


def with_slot(AX, slot, Ax):
    if AX.ndim == 1:
        return np.array(Ax, copy=True)
    out = AX.copy()
    out[slot] = Ax
    return out


# ---- the end-to-end case: an engineered tiny pivot on grid4000, solved with refinement -------------------------------

def end_to_end(hip, orc):
    """-> (mat with the engineered values, b, the oracle's partial-pivoting solution, k*)"""
    if "e2e" not in _PICKED:
        name = ("grid4000", 1)
        case = pc.lu_case(hip, orc, name)
        m, n, Ap, Ai, Ax = case["mat"]
        t = next(p.target for p in case["targets"] if p.target.cls == "forest_wave" and p.target.i is not None)
        hi = tiny(orc, case, t, RHO_TINY)
        b = np.random.default_rng(41).standard_normal(n)
        x = orc.csc_lusol_f(1, n, Ap, Ai, hi.Ax, b, 1.0)
        _PICKED["e2e"] = ((m, n, Ap, Ai, hi.Ax), b, x, t.k)
    return _PICKED["e2e"]


def refine_loop(solve, A, b, max_refine=10):
    """Factorization.solve_refined's loop with `solve` in place of the held factors and the sparse matrix A in the
    residual: -> (x, the corrections of the rounds that ran)."""
    x = solve(b)
    prev, corrections = np.inf, []
    for _ in range(max_refine):
        d = solve(b - A @ x)
        corr = float(np.abs(d).max())
        corrections.append(corr)
        if not corr <= prev:
            break
        x = x + d
        if not corr < 0.5 * prev:
            break
        prev = corr
    return x, corrections


# ---- a matched handle: delta refers to B ------------------------------------------------------------------------------

def matched_case(hip, orc, name="kkt400"):
    """One KKT case of tests/match_cases.py on a matched handle: B, its pivot order, and a delta between two of the
    smallest |U_kk| of the oracle's factors of B: the first such delta for which the reference perturbs between 1 and 8
    pivots of B within its rounds.  -> dict(c, rowperm, dr, dc, q, B, delta, ref)"""
    import match_cases as mc
    if ("matched", name) not in _PICKED:
        c = mc.case(name)
        with hip.Factorization(c.n, c.n, c.Ap, c.Ai, match_values=c.Ax) as F:
            rowperm, dr, dc = F.matching()
            q = F.ordering()["q"]
        Bp, Bi, Bx = mc.scaled(c, c.Ax, rowperm, dr, dc)
        U = orc.csc_lu_f(c.n, c.n, Bp, Bi, Bx, q, 0.0)
        d = np.sort(np.abs(diag_of_u(c.n, U[3], U[5])))
        ref = None
        for j in range(8):                        # (|B| <= 1 and |B_jj| = 1: the pivots of B lie close together, and
            delta = float(np.sqrt(d[j] * d[j + 1]))       #  replacing one moves the ones behind it -- many deltas cascade)
            try:
                ref = reference(orc, (c.n, c.n, Bp, Bi, Bx), q, delta)
            except TooManyRounds:
                continue
            if 1 <= len(ref.perturbed) <= 8:
                break
        assert ref is not None and 1 <= len(ref.perturbed) <= 8
        _PICKED["matched", name] = dict(c=c, rowperm=rowperm, dr=dr, dc=dc, q=q, B=(Bp, Bi, Bx), delta=delta, ref=ref)
    return _PICKED["matched", name]
