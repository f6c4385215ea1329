"""Matrices whose pivot k* sits at a chosen ratio rho = |pivot| / max|column below|, for the tests of the pivot
acceptance check at its threshold (tests/test_pivot_cases_cpu.py, tests/test_gpu_pivot_threshold.py).

The construction (LU): factor with the oracle at tol = 0; u = U[k*, k*]; M = max_i |L[i, k*]| |u| is the largest entry of
the unnormalised column and does not depend on A's entry (q[k*], q[k*]) = a; that entry becomes (a - u) + rho M, so the
pivot is rho M and everything before k* is untouched.  cs_lu's rule |pivot| >= tol max|column| then accepts k* for
tol = rho (1 - 1e-6) and rejects it for tol = rho (1 + 1e-6): the margin is six orders above the construction's rounding
and above the few ulp between the kernels' |multiplier| <= 1/tol and the oracle's comparison.  To steer WHERE the column
maximum sits, A's entry (q[i*], q[k*]) is multiplied by `boost` first (only where A has such an entry).

Cholesky: a' = (a - d) + sign 1e-6 a with d the pivot L[k*, k*]^2: sign = -1 gives a negative pivot at k*; sign = +1 a tiny
positive one, after which the oracle fails at a later, well-defined step (or not at all when nothing lies below k*).

Which kernel factors a front is decided by the analysis from r (order), w (pivots), the batch and the forest; `fronts()`
reads them from a handle (no device needed) and restates the dispatch of symbolic.cpp / kernels.hip in its `cls`, so
that a change of dispatch makes the tests' class assertions fail instead of leaving a kernel silently untested.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from csparse3_amd import synth

RHOS = (0.01, 0.03, 0.1, 0.3)
MARGIN = 1e-6
BOOST = 50.0


# ------------------------------------------------------------------ construction --

def _entry(Ap, Ai, row, col):
    """Index into Ax of A's entry (row, col), or -1."""
    lo, hi = int(Ap[col]), int(Ap[col + 1])
    hit = np.flatnonzero(Ai[lo:hi] == row)
    return lo + int(hit[0]) if len(hit) else -1


def column_of_l(Lp, Li, Lx, k):
    """(rows, values) of L's column k below the diagonal (the oracle keeps the diagonal first)."""
    lo, hi = int(Lp[k]), int(Lp[k + 1])
    assert Li[lo] == k
    return Li[lo + 1:hi], Lx[lo + 1:hi]


def engineer_lu(orc, n, Ap, Ai, Ax, q, k_star, rho, i_star=None, boost=BOOST):
    """-> (Ax', i_max, weight): the values with pivot k* at ratio rho, the row (pivot order) that holds the column's
    maximum, and weight = rho M / (|a| + |u|): the new pivot is known to about u_round / weight relative, on both sides
    (it is what a cancellation leaves), so the margin of 1e-6 and the 1e-10 of the value comparison need a weight well
    above 1e-9 and 1e-5 (MIN_WEIGHT).  i_star: the pivot-order row whose entry of column k* is multiplied by `boost` first."""
    Ax = np.array(Ax, dtype=np.float64, copy=True)
    if i_star is not None:
        p = _entry(Ap, Ai, q[i_star], q[k_star])
        assert p >= 0, "A has no entry (q[%d], q[%d]) to boost" % (i_star, k_star)
        Ax[p] *= boost
    Lp, Li, Lx, Up, Ui, Ux, opinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, 0.0)
    assert np.array_equal(opinv, np.argsort(q)), "tol = 0 keeps every diagonal"
    assert Ui[Up[k_star + 1] - 1] == k_star
    u = Ux[Up[k_star + 1] - 1]
    rows, vals = column_of_l(Lp, Li, Lx, k_star)
    assert len(rows) > 0, "pivot %d has no rows below it" % k_star
    M = np.abs(vals).max() * abs(u)
    p = _entry(Ap, Ai, q[k_star], q[k_star])
    assert p >= 0
    weight = rho * M / (abs(Ax[p]) + abs(u))
    Ax[p] = (Ax[p] - u) + rho * M
    return Ax, int(rows[np.argmax(np.abs(vals))]), weight


def oracle_chol(orc, n, Ap, Ai, Ax, q):
    """cs_chol in the order q -> (Lp, Li, Lx); raises orc.NotPositiveDefinite("... at step k")."""
    pinv = orc.csc_pinv(q)
    _, _, Cp, Ci, _ = orc.csc_symperm(n, Ap, Ai, None, pinv)
    parent = orc.csc_etree_f(n, Cp, Ci)
    post = orc.csc_post_f(n, parent)
    cnt = orc.csc_counts_f(n, Cp, Ci, parent, post)
    cp = np.zeros(n + 1, dtype=np.int32)
    cp[1:] = np.cumsum(cnt)
    return orc.csc_chol_f(n, Ap, Ai, Ax, pinv, parent, cp)


def chol_fail_step(orc, n, Ap, Ai, Ax, q):
    """The step at which the oracle's Cholesky meets a non-positive pivot, or None when it succeeds."""
    try:
        oracle_chol(orc, n, Ap, Ai, Ax, q)
    except orc.NotPositiveDefinite as e:
        return int(str(e).rsplit(" ", 1)[1])
    return None


def engineer_chol(orc, n, Ap, Ai, Ax, q, k_star, sign):
    """-> Ax' with the pivot of step k* equal to sign * 1e-6 * a, a = A's entry (q[k*], q[k*])."""
    Ax = np.array(Ax, dtype=np.float64, copy=True)
    Lp, Li, Lx = oracle_chol(orc, n, Ap, Ai, Ax, q)
    assert Li[Lp[k_star]] == k_star
    d = Lx[Lp[k_star]] ** 2
    p = _entry(Ap, Ai, q[k_star], q[k_star])
    assert p >= 0
    Ax[p] = (Ax[p] - d) + sign * MARGIN * Ax[p]
    return Ax


def first_off_diagonal(orc, n, Ap, Ai, Ax, q, tol):
    """The first pivot step at which cs_lu with threshold tol leaves the diagonal, or None when it keeps every one."""
    opinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, tol)[6]
    off = np.flatnonzero(opinv[q] != np.arange(n))
    return int(off[0]) if len(off) else None


# ------------------------------------------------------- fronts and their kernels --

Fronts = namedtuple("Fronts", "c0 w r parent forest task level shared cls rows q n batch kind")


def _front_class(r, w, split_small, interleave):                  # symbolic.cpp: front_class
    if r <= 16 and interleave:
        return "il"
    if r <= 32 and split_small:
        return "r32"
    if r <= 64:
        return "r64"
    if r <= 136 and r - min(w, 16) <= 128:
        return "lds"
    return "big"


def fronts(hip, F):
    """Everything the dispatch depends on, per supernode of the handle F, and the kernel class that follows from it:
    forest_wave / forest_shared (bottom forest, one wave / four waves per front), wave (k_front_wave), mix_wave / mix_grid
    (k_front_mix: one-wave panel for w <= 32, the 16 x 16 grid above), block (k_front_block), big_step (k_big_step),
    wg (k_front_wg), il (k_front_il).  On a Schur handle the last supernode is 'schur' (FC_SCHUR: assembled, never
    eliminated, whatever its order; it neither rides nor counts on its level) and `rows` is None: such a handle refuses
    factors()."""
    lib = hip.lib()
    ns = int(F.info.nsuper)
    schur = ns - 1 if getattr(F, "ns", 0) else -1
    batch, kind, n = F.batch, F.kind, F.n
    i32p = C.POINTER(C.c_int32)
    p = lambda a: a.ctypes.data_as(i32p)                                   # noqa: E731
    lib.cs3_debug_schedule.argtypes = [C.c_void_p] + [i32p] * 3
    lib.cs3_debug_forest.argtypes = [C.c_void_p] + [i32p] * 4
    lib.cs3_debug_forest.restype = C.c_int64
    sched, fr, fw = (np.zeros(ns, dtype=np.int32) for _ in range(3))
    assert lib.cs3_debug_schedule(F._h, p(sched), p(fr), p(fw)) == 0
    r = np.zeros(ns, dtype=np.int64)
    r[sched] = fr
    sn_ptr, parent, _ = F.supernodes()
    c0, w = sn_ptr[:-1].astype(np.int64), np.diff(sn_ptr).astype(np.int64)
    wsched = np.zeros(ns, dtype=np.int64)
    wsched[sched] = fw
    assert np.array_equal(wsched, w)
    sn, task, level, tier = (np.full(ns, -1, dtype=np.int32) for _ in range(4))
    nf = int(lib.cs3_debug_forest(F._h, p(sn), p(task), p(level), p(tier)))
    forest = np.zeros(ns, dtype=bool)
    ftask, flevel = np.full(ns, -1), np.full(ns, -1)
    forest[sn[:nf]] = True
    ftask[sn[:nf]], flevel[sn[:nf]] = task[:nf], level[:nf]
    # shared by four waves: six pivots or more, on a local level of at most two fronts (symbolic.cpp: coop_w, coop_level)
    per_level = {}
    for s in np.flatnonzero(forest):
        per_level[ftask[s], flevel[s]] = per_level.get((ftask[s], flevel[s]), 0) + 1
    shared = np.array([forest[s] and w[s] >= 6 and per_level[ftask[s], flevel[s]] <= 2 for s in range(ns)], dtype=bool)
    # single matrices: the small fronts of a level that holds a big front ride its chain of block launches
    height = np.zeros(ns, dtype=np.int64)
    for s in range(ns):
        if parent[s] >= 0 and not forest[s]:
            height[parent[s]] = max(height[parent[s]], height[s] + 1)
    ride = np.zeros(ns, dtype=bool)
    if batch == 1:
        for lv in np.unique(height[~forest]):
            on = [s for s in range(ns) if not forest[s] and height[s] == lv and s != schur]
            big = [s for s in on if _front_class(r[s], w[s], False, False) == "big"]
            small = [s for s in on if s not in big]
            if big and len(small) <= 8 and (max([w[s] for s in small], default=0) + 31) // 32 <= (max(w[s] for s in big) + 31) // 32:
                ride[on] = True
    cls = []
    for s in range(ns):
        if forest[s]:
            cls.append("forest_shared" if shared[s] else "forest_wave")
            continue
        if s == schur:
            cls.append("schur")
            continue
        fc = "big" if ride[s] else _front_class(r[s], w[s], batch >= 8, batch >= 128)
        if fc == "big":
            ld = (r[s] + 1) | 1                                            # schedule.cpp: wg_lds_bytes, per front (<= per group)
            lds = (16 * 33 + (2 if kind == hip.CS3_LU else 1) * 16 * ld + (0 if kind == hip.CS3_LU else 16 * w[s])) * 8
            cls.append("wg" if batch >= 48 and lds <= 150 * 1024 else "big_step")
        else:
            cls.append({"il": "il", "r32": "wave", "lds": "block", "r64": "mix_wave" if w[s] <= 32 else "mix_grid"}[fc])
    rows = None
    if schur < 0:
        Lp, Li = F.factors(values=False)[:2]
        # (supernodes are relaxed: the front's rows are the union of its columns' patterns)
        rows = [np.unique(Li[Lp[c0[s]]:Lp[c0[s] + w[s]]]).astype(np.int64) for s in range(ns)]
        for s in range(ns):
            assert len(rows[s]) == r[s] and np.array_equal(rows[s][:w[s]], np.arange(c0[s], c0[s] + w[s]))
    return Fronts(c0, w, r, parent, forest, ftask, flevel, shared, cls, rows, F.ordering()["q"], n, batch, kind)


# ------------------------------------------------------------------------ targets --

# k: the engineered pivot; i: the row (pivot order) whose entry of column k is boosted, where: what that row is;
# front: the supernode; cls: its kernel class
Target = namedtuple("Target", "label cls front k i where")


def _has(Ap, Ai, q, i, k):
    return _entry(Ap, Ai, q[i], q[k]) >= 0


def _row_in(Ap, Ai, q, k, candidates):
    """The first of `candidates` (rows below k) at which A has an entry in column k, or None."""
    for i in candidates:
        if i > k and _has(Ap, Ai, q, int(i), k):
            return int(i)
    return None


def front_targets(FR, Ap, Ai, s, positions, regions, label):
    """Targets in front s: for every position j (pivot c0 + j) and every region name in `regions` -- a function
    (rows below the pivot, k) -> candidate rows, in order of preference -- the first candidate that A has an entry at."""
    out = []
    for j in positions:
        k = int(FR.c0[s] + j)
        below = FR.rows[s][FR.rows[s] > k]
        if len(below) == 0:
            continue
        got = []
        for where, pick in regions.items():
            i = _row_in(Ap, Ai, FR.q, k, pick(below, k))
            if i is not None and i not in got:
                got.append(i)
                out.append(Target("%s f%d p%d %s" % (label, s, j, where), FR.cls[s], int(s), k, i, where))
        if not got:                                        # A has nothing below this pivot inside the front (fill only): unsteered
            out.append(Target("%s f%d p%d any" % (label, s, j), FR.cls[s], int(s), k, None, "any"))
    return out


Prepared = namedtuple("Prepared", "target rho Ax i_max weight")
MIN_WEIGHT = 1e-4           # below it the factors are not compared (1e-10 norm-wise needs ~ 10 u / weight <= 1e-10) ...
DECISION_WEIGHT = 1e-6      # ... and below this one the target is dropped: the decision's margin of 1e-6 needs c u / weight << 1e-6


BOOSTS = (BOOST, 8.0, 2.0)


def prepare(orc, n, Ap, Ai, Ax, q, t):
    """The engineered values for target t at the first rho of RHOS for which the oracle keeps every diagonal at
    tol = rho (1 - 1e-6); rho = None: reject only (the values are then those for RHOS[0]).  Where the pivot growth
    behind a boosted entry spoils the accept side for every rho, a smaller boost is tried, as long as the column's
    maximum still sits in the steered row."""
    first = None
    for boost in BOOSTS if t.i is not None else BOOSTS[:1]:
        for rho in RHOS:
            Ax2, i_max, weight = engineer_lu(orc, n, Ap, Ai, Ax, q, t.k, rho, t.i, boost)
            if t.i is not None and i_max != t.i:
                break
            if first is None:
                first = Prepared(t, None, Ax2, i_max, weight)
            if first_off_diagonal(orc, n, Ap, Ai, Ax2, q, rho * (1 - MARGIN)) is None:
                return Prepared(t, rho, Ax2, i_max, weight)
    assert first is not None, "the boost does not move the maximum of column %d to row %d" % (t.k, t.i)
    return first


def reject_rho(prep):
    return prep.rho if prep.rho is not None else RHOS[0]


# -------------------------------------------------------------------------- cases --

def _sym(mat):
    m, n, Ap, Ai, Ax = mat
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    S = (A + A.T).tocsc()
    S.sort_indices()
    return n, n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()


def matrix(name):
    """The matrices of the tests, by name (built once)."""
    if name not in _MATRICES:
        if name == "grid4000":
            _MATRICES[name] = synth.grid_jacobian(4000, seed=7)
        elif name == "grid3000":
            _MATRICES[name] = synth.grid_jacobian(3000, seed=13)
        elif name == "spd3000":
            ei, ej = synth.spd_grid_pattern(3000, seed=21)
            _MATRICES[name] = synth.spd_grid_matrix(3000, ei, ej, seed=22)
        elif name.startswith("spd_db"):
            _MATRICES[name] = _sym(matrix(name[4:]))
        else:                                                              # "db<nd>"
            nd = int(name[2:])
            _MATRICES[name] = synth.dense_block_matrix(nd + 120, nd, seed=1000 + nd)
    return _MATRICES[name]


_MATRICES = {}

# (matrix, batch) -> the kernel classes the case is there for; the smallest matrices that reach each class
LU_CASES = {("grid4000", 1): ("forest_wave", "forest_shared", "mix_wave", "mix_grid"),
            ("db100", 1): ("block",), ("db180", 1): ("big_step",),
            ("db100", 20): ("wave", "block"), ("db48", 20): ("wave", "block"),
            ("db180", 50): ("wg",), ("grid3000", 130): ("il",)}

_NEAR = {"near": lambda below, k: below}                  # the nearest row below the pivot at which A has an entry
_FAR = {"far": lambda below, k: below[::-1]}              # the farthest (the front's last row where A has one there)


def _first(seq, n=1):
    return list(seq)[:n]


def lu_targets(FR, Ap, Ai, name):
    """The target list of one LU case: per kernel class the pivots at which its lanes, waves or tiles change hands, with the
    column's maximum steered once near the pivot and once far from it (another wave, stacked lanes, a partial tile)."""
    ns = len(FR.w)
    S = range(ns)
    both = dict(_NEAR, **_FAR)
    out = []
    top = {}
    for s in S:
        if FR.forest[s]:
            top[FR.task[s]] = max(top.get(FR.task[s], 0), FR.level[s])
    if name == ("grid4000", 1):
        # forest: a leaf and a front of its task's top local level, one wave per front and shared by four waves (those
        # own eight columns each: 7 | 8, 15 | 16 and 23 are their boundaries); the maximum near the pivot and far from it
        for lab, cond in (("leaf", lambda s: FR.level[s] == 0), ("top", lambda s: FR.level[s] == top[FR.task[s]] and FR.level[s] > 0)):
            for cls in ("forest_wave", "forest_shared"):
                cand = [s for s in S if FR.cls[s] == cls and cond(s) and FR.r[s] > FR.w[s] and FR.w[s] >= (17 if cls == "forest_shared" else 3)]
                if not cand:
                    continue
                s = max(cand, key=lambda s: (FR.w[s], -s))                   # the widest, the first of those
                w = int(FR.w[s])
                if cls == "forest_wave":
                    out += front_targets(FR, Ap, Ai, s, [0, w - 1], both, "%s %s" % (cls, lab))
                else:
                    pos = [j for j in (0, 7, 8, 15, 16, 23, w - 1) if j < w]
                    out += front_targets(FR, Ap, Ai, s, pos[0::2], _NEAR, "%s %s" % (cls, lab))
                    out += front_targets(FR, Ap, Ai, s, pos[1::2] + [0], _FAR, "%s %s" % (cls, lab))
        # above the forest, one-wave panel: first and last pivot, and the maximum in a contribution row
        for s in _first((s for s in S if FR.cls[s] == "mix_wave" and 17 <= FR.r[s] <= 32 and FR.r[s] > FR.w[s] >= 3), 2):
            w = int(FR.w[s])
            cb = {"contrib": lambda below, k, e=int(FR.c0[s] + w): below[below >= e][::-1]}
            out += front_targets(FR, Ap, Ai, s, [0], both, "mix_wave")
            out += front_targets(FR, Ap, Ai, s, [w - 1, w // 2], cb, "mix_wave")
        # the 16 x 16 grid kernel (w = 43 = r, a root: its last pivot has nothing below it, so w - 2 stands for w - 1)
        for s in (s for s in S if FR.cls[s] == "mix_grid"):
            w = int(FR.w[s])
            # (17, 33 and w - 3: columns 16, 32 and w - 2 of this matrix hold nothing but small fill below the pivot)
            out += front_targets(FR, Ap, Ai, s, [0, 16, 17, 32, 33, w - 3, w - 2], _NEAR, "mix_grid")
            out += front_targets(FR, Ap, Ai, s, [0, 15, 31], _FAR, "mix_grid")
    elif name[0] in ("db100", "db48") and name[1] in (1, 20):
        # k_front_block: pivots at the block edges and w - 2; the maximum inside the diagonal block's rows and in the
        # stacked rows (beyond the block).  Blocks of equal width: ceil(w / ceil(w / 16)).
        for s in (s for s in S if FR.cls[s] == "block"):
            w, c0 = int(FR.w[s]), int(FR.c0[s])
            bsz = -(-w // -(-w // 16))
            edge = lambda k: c0 + ((k - c0) // bsz + 1) * bsz                            # noqa: E731
            reg = {"diag": lambda below, k: below[below < min(edge(k), c0 + w)],
                   "stacked": lambda below, k: below[below >= edge(k)][::-1]}
            pos = sorted(set(j for j in (0, bsz - 1, bsz, w - 2) if 0 <= j < w))
            out += front_targets(FR, Ap, Ai, s, pos, reg, "block")
        if name[1] == 20:                                                  # k_front_wave: the fronts of order <= 32 of a batch
            for s in _first((s for s in S if FR.cls[s] == "wave" and FR.w[s] >= 3 and FR.r[s] > FR.w[s]), 2):
                w = int(FR.w[s])
                cb = {"contrib": lambda below, k, e=int(FR.c0[s] + w): below[below >= e][::-1]}
                out += front_targets(FR, Ap, Ai, s, [0], _NEAR, "wave")
                out += front_targets(FR, Ap, Ai, s, [0, w - 1], cb, "wave")
    elif name[0] == "db180":
        # k_big_step (32 pivots per block step, 64-row tiles below) / k_front_wg (16 pivots per block step): pivots at
        # the block edges and w - 2; the maximum inside the diagonal block, in the next 64-row tile, in the last partial one
        nb = 32 if name[1] == 1 else 16
        for s in (s for s in S if FR.cls[s] in ("big_step", "wg") and FR.w[s] > 136):
            w, c0, r = int(FR.w[s]), int(FR.c0[s]), int(FR.r[s])
            edge = lambda k: c0 + ((k - c0) // nb + 1) * nb                              # noqa: E731
            tail = c0 + ((r - 1) // 64) * 64
            reg = {"diag": lambda below, k: below[below < edge(k)][::-1],
                   "tile": lambda below, k: below[(below >= edge(k)) & (below < edge(k) + 64)][::-1],
                   "tail": lambda below, k: below[below >= tail][::-1]}
            pos = [0, 31, 32, 63, 64, w - 2] if nb == 32 else [0, 15, 16, w - 2]
            out += front_targets(FR, Ap, Ai, s, pos, reg, FR.cls[s])
    elif name == ("grid3000", 130):
        # k_front_il (4 pivots per block, 8-row tiles below): first pivot, the block edge 3 | 4, the last pivot; the
        # maximum inside the diagonal 4 x 4 block and in the front's last row
        got = 0
        for s in S:
            if FR.cls[s] != "il" or FR.w[s] < 5 or FR.r[s] == FR.w[s]:
                continue
            w, c0 = int(FR.w[s]), int(FR.c0[s])
            edge = lambda k: c0 + ((k - c0) // 4 + 1) * 4                                # noqa: E731
            reg = {"diag": lambda below, k: below[below < min(edge(k), c0 + w)],
                   "far": lambda below, k: below[below >= edge(k)][::-1]}
            tg = front_targets(FR, Ap, Ai, s, [0, 3, 4, w - 1], reg, "il")
            if len(tg) >= 5:
                out += tg
                got += 1
            if got == 2:
                break
    return out


def two_failure_targets(FR, Ap, Ai, classes):
    """Pairs (t1, t2), k1 < k2 in one front, per kernel class of the case: k1 at rho, then k2 at rho / 2 on the refactored
    matrix; a tolerance above both must report k1.  For k_front_il the pairs that its program order (diagonal block
    column by column, then the rows below tile by tile) would report wrongly with a first-wins rule:
    'il order': k2 = c0 + 2 fails inside the diagonal 4 x 4 block, k1 = c0 only in a row below the block;
    'il rows': both fail below the block, k1 in a later 8-row tile than k2."""
    out = []
    seen = set()
    for s in range(len(FR.w)):
        cls, w, c0, r = FR.cls[s], int(FR.w[s]), int(FR.c0[s]), int(FR.r[s])
        rows = FR.rows[s]
        if cls == "il" and "il" in classes and w >= 4 and r > w and "il order" not in seen:
            below_block = rows[rows >= c0 + 4][::-1]
            i1 = _row_in(Ap, Ai, FR.q, c0, below_block)
            if i1 is not None and _has(Ap, Ai, FR.q, c0 + 3, c0 + 2):
                seen.add("il order")
                out.append(("il order", Target("il order k1", cls, s, c0, i1, "below"), Target("il order k2", cls, s, c0 + 2, c0 + 3, "diag")))
        if cls == "il" and "il" in classes and w >= 2 and "il rows" not in seen:
            ke = c0 + min(4, w)
            tile = lambda i: (np.searchsorted(rows, i) - (ke - c0)) // 8               # noqa: E731
            late = [i for i in rows[rows >= ke][::-1] if tile(i) >= 1]
            early = [i for i in rows[rows >= ke] if tile(i) == 0]
            i1, i2 = _row_in(Ap, Ai, FR.q, c0, late), _row_in(Ap, Ai, FR.q, c0 + 1, early)
            if i1 is not None and i2 is not None:
                seen.add("il rows")
                out.append(("il rows", Target("il rows k1", cls, s, c0, i1, "late tile"), Target("il rows k2", cls, s, c0 + 1, i2, "first tile")))
        if cls not in classes or cls in seen or w < 3 or (cls.startswith("forest") and r == w):
            continue
        k1, k2 = c0 + (w // 2) - 1, c0 + w - 2 if r == w else c0 + w - 1
        if k2 <= k1:
            continue
        i1 = _row_in(Ap, Ai, FR.q, k1, rows[rows > k1][::-1])
        i2 = _row_in(Ap, Ai, FR.q, k2, rows[rows > k2])
        seen.add(cls)                                      # (i = None: A has no entry there, the maximum stays where it is)
        out.append((cls, Target(cls + " two k1", cls, s, k1, i1, "far"), Target(cls + " two k2", cls, s, k2, i2, "near")))
    return out


def prepare_two(orc, n, Ap, Ai, Ax, q, t1, t2, rho=RHOS[0], sharp=False):
    """-> (Ax', tol): k1 at rho, k2 at rho / 2 on the matrix that holds k1 already; tol = rho (1 + 1e-6) rejects both.
    sharp (the k_front_il order cases, where it matters WHICH rows fail): k2 at rho too, behind a boost of 1000, so that
    each column fails in its steered row alone -- the elimination of k1 leaves 1 / rho times row k1 in row i1, also in
    column k2, and only a larger entry keeps that from being column k2's maximum."""
    Ax1 = engineer_lu(orc, n, Ap, Ai, Ax, q, t1.k, rho, t1.i)[0]
    Ax2 = engineer_lu(orc, n, Ap, Ai, Ax1, q, t2.k, rho if sharp else rho / 2, t2.i, 1000.0 if sharp else BOOST)[0]
    return Ax2, rho * (1 + MARGIN)


# One analysis, target list and set of engineered matrices per case and process: the CPU test and the GPU tests share them.
_CACHE = {}


def lu_case(hip, orc, name):
    """-> dict(mat, FR, targets [Prepared], pairs [(label, t1, t2, Ax, tol)]) of LU_CASES entry `name`."""
    if name not in _CACHE:
        m, n, Ap, Ai, Ax = matrix(name[0])
        with hip.Factorization(m, n, Ap, Ai, batch=name[1]) as F:
            FR = fronts(hip, F)
        preps = [prepare(orc, n, Ap, Ai, Ax, FR.q, t) for t in lu_targets(FR, Ap, Ai, name)]
        # (an unsteered column that holds nothing but small fill makes the engineered pivot the rest of a cancellation)
        assert all(p.weight >= MIN_WEIGHT for p in preps if p.target.i is not None)
        preps = [p for p in preps if p.weight >= DECISION_WEIGHT]
        pairs = []
        for label, t1, t2 in two_failure_targets(FR, Ap, Ai, LU_CASES[name]):
            Ax2, tol = prepare_two(orc, n, Ap, Ai, Ax, FR.q, t1, t2, sharp=label.startswith("il "))
            pairs.append((label, t1, t2, Ax2, tol))
        _CACHE[name] = dict(mat=(m, n, Ap, Ai, Ax), FR=FR, targets=preps, pairs=pairs)
    return _CACHE[name]
