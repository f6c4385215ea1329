"""Where k_big_step checks a pivot, and a matrix that fails the check at each such place (tests/test_big_step_flag_cases_cpu.py,
tests/test_gpu_big_step_flags.py).  Built on tests/pivot_cases.py: its db180 / spd_db180 matrices, its engineered pivots.

A block step of k_big_step factors BIG_NB = 32 pivots [kb, ke) of a big front.  The diagonal tile holds rows and columns
[kb, ke) of the front: lane = row, waves 0 and 2 take the columns 0..15 and 16..31 of the block ("half" lo / hi).  A
block-column tile t >= 1 holds the 64 front rows from ke + 64 (t - 1) with the same columns: waves 0 and 2 its upper 32
rows, waves 1 and 3 its lower 32 rows, for the lo / hi columns.  A check sits where an entry is stored: `place` names
that spot for a front row and a pivot, from the host analysis alone.  The front's last block is partial (bw < 32).
"""
from collections import namedtuple

import numpy as np

import pivot_cases as pc

BIG_NB = 32
LU, CHOL = ("db180", 1), ("spd_db180", 1)

Place = namedtuple("Place", "block half partial tile rows")


def big_front(FR):
    """The one big front of the db180 matrices (class big_step)."""
    big = [s for s in range(len(FR.w)) if FR.cls[s] == "big_step" and FR.w[s] > 136]
    assert len(big) == 1
    return big[0]


def place(FR, s, k, i):
    """Where k_big_step stores (and checks) the entry of front s in pivot column k and row i >= k (pivot order)."""
    c0, w = int(FR.c0[s]), int(FR.w[s])
    j, p = k - c0, int(np.searchsorted(FR.rows[s], i))
    assert 0 <= j < w and FR.rows[s][p] == i and i >= k
    kb = j // BIG_NB * BIG_NB
    ke = min(kb + BIG_NB, w)
    half = "lo" if j - kb < 16 else "hi"
    if p < ke:
        return Place(kb // BIG_NB, half, ke - kb < BIG_NB, 0, None)
    return Place(kb // BIG_NB, half, ke - kb < BIG_NB, (p - ke) // 64 + 1, "upper" if (p - ke) % 64 < 32 else "lower")


# label -> (block, column inside the block, rows: "diag" or (tile, "upper" / "lower")): a multiplier at the threshold
MULTIPLIER_SITES = {
    "diag lo": (1, 5, "diag"), "diag hi": (1, 20, "diag"),
    "diag lo partial": (6, 3, "diag"), "diag hi partial": (6, 16, "diag"),
    "col upper lo": (1, 5, (1, "upper")), "col upper hi": (1, 20, (1, "upper")),
    "col lower lo": (1, 5, (1, "lower")), "col lower hi": (1, 20, (1, "lower")),
    "col last tile": (0, 31, (3, "lower")),
}
# label -> (k1's site, k2's site), k1 < k2 in one block: two failures of one launch
PAIR_SITES = {
    "col then diag": ((1, 3, (1, "lower")), (1, 9, "diag")),
    "diag then col": ((1, 3, "diag"), (1, 9, (1, "upper"))),
    "col then diag hi": ((1, 18, (2, "upper")), (1, 27, "diag")),
}
# label -> (block, column of k1, column of k2, rows): ONE row failing at two columns of one half, nothing else at k1
ONE_LANE_SITES = {
    "one lane diag": (1, 3, 9, "diag"), "one lane diag hi": (1, 17, 22, "diag"),
    "one lane col": (1, 3, 9, (1, "upper")),
}
# (block, column): the pivot itself -- exact zero, 1e301, NaN (LU); -+ 1e-6 a (Cholesky).  (6, 17) is the front's last pivot
DIAGONAL_SITES = [(1, 5), (1, 20), (6, 3), (6, 17)]


def _candidates(FR, s, k, rows):
    c0, w = int(FR.c0[s]), int(FR.w[s])
    kb = (k - c0) // BIG_NB * BIG_NB
    ke = min(kb + BIG_NB, w)
    fr = FR.rows[s]
    if rows == "diag":
        return fr[k - c0 + 1:ke][::-1]
    tile, part = rows
    lo = ke + 64 * (tile - 1) + (32 if part == "lower" else 0)
    return fr[lo:min(lo + 32, len(fr))][::-1]


def _target(FR, Ap, Ai, s, label, site):
    block, col, rows = site
    k = int(FR.c0[s]) + BIG_NB * block + col
    i = pc._row_in(Ap, Ai, FR.q, k, _candidates(FR, s, k, rows))
    assert i is not None, "%s: A has no entry below pivot %d in the rows %r" % (label, k, rows)
    return pc.Target(label, "big_step", s, k, i, rows)


def failing_rows(orc, n, Ap, Ai, Ax, q, k, tol):
    """(rows of column k whose multiplier lies beyond 1 / tol, the largest |multiplier| tol among the other rows), from
    the oracle's factors with every diagonal kept."""
    Lp, Li, Lx = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, 0.0)[:3]
    rows, vals = pc.column_of_l(Lp, Li, Lx, k)
    over = np.abs(vals) * tol > 1.0
    return rows[over], (np.abs(vals[~over]).max() * tol if (~over).any() else 0.0)


_CACHE = {}


def analysis(hip, kind_name=LU, batch=1):
    """-> (matrix, Fronts, big front) of db180 (LU) or spd_db180 (Cholesky), from the host analysis."""
    key = ("FR", kind_name, batch)
    if key not in _CACHE:
        m, n, Ap, Ai, Ax = pc.matrix(kind_name[0])
        kind = hip.CS3_LU if kind_name == LU else hip.CS3_CHOLESKY
        with hip.Factorization(m, n, Ap, Ai, kind=kind, batch=batch) as F:
            FR = pc.fronts(hip, F)
        _CACHE[key] = ((m, n, Ap, Ai, Ax), FR, big_front(FR))
    return _CACHE[key]


def multiplier_cases(hip, orc):
    """label -> Prepared (pivot_cases.prepare): the pivot at rho, the column's maximum in the site's row."""
    if "mult" not in _CACHE:
        (m, n, Ap, Ai, Ax), FR, s = analysis(hip)
        _CACHE["mult"] = {label: pc.prepare(orc, n, Ap, Ai, Ax, FR.q, _target(FR, Ap, Ai, s, label, site))
                          for label, site in MULTIPLIER_SITES.items()}
    return _CACHE["mult"]


def pair_cases(hip, orc):
    """label -> (t1, t2, Ax, tol): pivot_cases.prepare_two, sharp (each column fails in its steered row alone)."""
    if "pair" not in _CACHE:
        (m, n, Ap, Ai, Ax), FR, s = analysis(hip)
        out = {}
        for label, (s1, s2) in PAIR_SITES.items():
            t1, t2 = _target(FR, Ap, Ai, s, label + " k1", s1), _target(FR, Ap, Ai, s, label + " k2", s2)
            out[label] = (t1, t2) + pc.prepare_two(orc, n, Ap, Ai, Ax, FR.q, t1, t2, sharp=True)
        _CACHE["pair"] = out
    return _CACHE["pair"]


def one_lane_cases(hip, orc):
    """label -> (t1, t2, Ax, tol) with t1.i == t2.i: the same front row holds the maximum of both columns."""
    if "lane" not in _CACHE:
        (m, n, Ap, Ai, Ax), FR, s = analysis(hip)
        out = {}
        for label, (block, j1, j2, rows) in ONE_LANE_SITES.items():
            k1, k2 = (int(FR.c0[s]) + BIG_NB * block + j for j in (j1, j2))
            i = next((int(i) for i in _candidates(FR, s, k2, rows) if pc._has(Ap, Ai, FR.q, int(i), k1) and pc._has(Ap, Ai, FR.q, int(i), k2)), None)
            assert i is not None, label
            t1, t2 = pc.Target(label + " k1", "big_step", s, k1, i, rows), pc.Target(label + " k2", "big_step", s, k2, i, rows)
            out[label] = (t1, t2) + pc.prepare_two(orc, n, Ap, Ai, Ax, FR.q, t1, t2, sharp=True)
        _CACHE["lane"] = out
    return _CACHE["lane"]


def diagonal_columns(FR, s):
    return [int(FR.c0[s]) + BIG_NB * b + j for b, j in DIAGONAL_SITES]


def nan_entries(FR, Ap, Ai, s):
    """label -> (k, i): entries of A, in column k = block 1 column 5 of the big front, that the NaN cases overwrite.  Row i
    takes part in no column before k except through its own multipliers, which do not read the entry (i, k): column k is
    the first that sees the NaN, wherever it sits."""
    k = int(FR.c0[s]) + BIG_NB + 5
    return {"pivot": (k, k),
            "diag": (k, pc._row_in(Ap, Ai, FR.q, k, _candidates(FR, s, k, "diag"))),
            "col": (k, pc._row_in(Ap, Ai, FR.q, k, _candidates(FR, s, k, (2, "lower"))))}


def with_zero_column(Ap, Ai, Ax, q, k):
    """Column q[k] of A set to zero: pivot k is an exact zero whatever came before it."""
    out = np.array(Ax, dtype=np.float64, copy=True)
    out[Ap[q[k]]:Ap[q[k] + 1]] = 0.0
    return out


def with_entry(Ap, Ai, Ax, q, i, k, value):
    """A's entry (q[i], q[k]) replaced by `value`."""
    p = pc._entry(Ap, Ai, q[i], q[k])
    assert p >= 0
    out = np.array(Ax, dtype=np.float64, copy=True)
    out[p] = value
    return out
