"""The matrices of the selected-inversion tests (tests/test_selinv_cpu.py, tests/test_gpu_selinv.py).  Every size that is
meant to sit at an edge of a kernel comes from cs3_selinv_limits(); nothing here needs a GPU.

A case is (m, n, Ap, Ai, Ax) as csparse3_amd.synth returns it; Ap / Ai int32, Ax float64.
"""
import functools

import numpy as np

import sweep_cases
from csparse3_amd import csc_hip as hip
from csparse3_amd import synth

LIMITS = hip.selinv_limits()


def _csc(n, rows, cols, vals, sort=True):
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float64)
    order = np.lexsort((rows, cols)) if sort else np.argsort(cols, kind="stable")
    Ap = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, n, Ap, rows[order].astype(np.int32), vals[order]


def diagonal(n=7):
    """Every front has r = w = 1."""
    return _csc(n, np.arange(n), np.arange(n), 2.0 + np.arange(n))


def tridiagonal(n=40):
    """A chain: c = 1 at every front but the last."""
    i = np.arange(n - 1)
    rows = np.concatenate([np.arange(n), i + 1, i])
    cols = np.concatenate([np.arange(n), i, i + 1])
    vals = np.concatenate([4.0 + 0.01 * np.arange(n), -1.0 - 0.02 * i, -1.5 + 0.01 * i])
    return _csc(n, rows, cols, vals)


def tiny(n):
    """n = 1 and n = 2 (dense)."""
    A = np.array([[3.0]]) if n == 1 else np.array([[4.0, -1.0], [2.0, 5.0]])
    i, j = np.nonzero(A)
    return _csc(n, i, j, A[i, j])


def _toy_triplets():
    _, n, Ap, Ai, Ax = synth.toy10()[:5]
    return n, np.asarray(Ai[:Ap[n]]), np.repeat(np.arange(n), np.diff(Ap)), np.asarray(Ax[:Ap[n]])


def unsorted_rows():
    """toy10 with the rows of every column stored in descending order."""
    n, rows, cols, vals = _toy_triplets()
    order = np.lexsort((-rows, cols))
    return _csc(n, rows[order], cols[order], vals[order], sort=False)


def absent_diagonal():
    """toy10 without a stored (9, 9): in the natural order (ORDER below) the last pivot is fill alone."""
    n, rows, cols, vals = _toy_triplets()
    keep = ~((rows == cols) & (rows == n - 1))
    return _csc(n, rows[keep], cols[keep], vals[keep])


def one_sided():
    """toy10 with (2, 1) and (9, 8) stored but not (1, 2) and (8, 9)."""
    n, rows, cols, vals = _toy_triplets()
    keep = ~(((rows == 1) & (cols == 2)) | ((rows == 8) & (cols == 9)))
    assert keep.sum() == len(rows) - 2
    return _csc(n, rows[keep], cols[keep], vals[keep])


def _front_orders(n, Ap, Ai, kind=hip.CS3_LU):
    with hip.Factorization(n, n, Ap, Ai, kind) as F:
        ns = int(F.info.nsuper)
        sched, r, w = (np.empty(ns, dtype=np.int32) for _ in range(3))
        hip._check(hip.lib().cs3_debug_schedule(F._h, hip._pi(sched), hip._pi(r), hip._pi(w)))
        parent = F.supernodes()[1]
        return [(int(r[t]), int(w[t]), int(parent[sched[t]])) for t in range(ns)]


@functools.lru_cache(maxsize=None)
def dense_root(order):
    """synth.dense_block_matrix(n, nd, 1) whose root front has exactly `order` rows: the analysis amalgamates a few columns
    into the dense block, so (n, nd) is searched for, from nd = order downwards.  Where the analysis offers no such root
    with fronts below it (it never ends a tree in a root one row beyond the LDS), the dense matrix of that order is the case."""
    for nd in range(order, max(order - 48, 1), -1):
        for extra in range(10, 100, 5):
            case = synth.dense_block_matrix(nd + extra, nd, 1)
            roots = [r for r, w, parent in _front_orders(case[1], case[2], case[3]) if parent < 0]
            if roots == [order]:
                return case
    case = synth.dense_block_matrix(order, order, 1)
    assert [r for r, w, parent in _front_orders(case[1], case[2], case[3]) if parent < 0] == [order]
    return case


def dense_root_orders():
    """The orders at which the kernel of the root front changes, one on either side, and two beyond the LDS that are no
    multiple of the GEMM tile or of the chunk of the triangular solves."""
    L = LIMITS
    ragged = [150, 201]
    assert all(o > L.lds_max_order + 1 and o % L.gemm_tile and o % L.diag_block for o in ragged)
    return [int(L.wave_max_order), int(L.wave_max_order) + 1, int(L.lds_max_order), int(L.lds_max_order) + 1] + ragged


def w72(symmetric=False, fringe=0):
    """Two (142, 72) fronts under a (214, 214) root (sweep_cases); fringe: chains of small fronts under the big ones."""
    return sweep_cases.case_matrix("w72", symmetric=symmetric, fringe=fringe)


@functools.lru_cache(maxsize=None)
def spd_small(n=300):
    ei, ej = synth.spd_grid_pattern(n, seed=n)
    return synth.spd_grid_matrix(n, ei, ej, seed=7, shift=0.5)


ORDER = {"absent_diagonal": hip.ORDER_NATURAL}       # every other case: ORDER_AMD


def plan_cases():
    """name -> case for the tests of the plan and of the restated recurrence (small: the restatement is dense)."""
    return {"toy10": synth.toy10()[:5], "jacobian_like": synth.jacobian_like()[:5], "unsorted_rows": unsorted_rows(),
            "absent_diagonal": absent_diagonal(), "one_sided": one_sided()}


def analysed(name, case, kind=hip.CS3_LU, batch=1):
    """A handle on the case's pattern, in the order the case asks for."""
    return hip.Factorization(case[0], case[1], case[2], case[3], kind, ORDER.get(name, hip.ORDER_AMD), batch=batch)
