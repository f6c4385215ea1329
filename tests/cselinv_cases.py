"""The matrices of the complex selected-inversion tests (tests/test_cselinv_cpu.py, tests/test_gpu_cselinv.py).  Every
size that is meant to sit at an edge of a kernel comes from cs3_cplx_selinv_limits() or cs3_selinv_limits(); nothing here
needs a GPU.  A case is (n, Ap, Ai, Az, kind, rotate): kind "lu" or "chol", Az complex128 [nnz]."""
import functools

import numpy as np

import cplx_cases
from csparse3_amd import csc_hip as hip
from csparse3_amd import synth

LIMITS = hip.cplx_selinv_limits()
REAL_LIMITS = hip.selinv_limits()


def kind_of(case):
    return hip.CS3_CHOLESKY if case[4] == "chol" else hip.CS3_LU


def structural(name):
    """A structural pattern of cplx_cases with values of order 1 and an imaginary diagonal that dominates."""
    n, Ap, Ai = cplx_cases.structural_cases()[name]
    Az = cplx_cases.values_for(np.random.default_rng(len(name)), int(Ap[n]))[0]
    col = np.repeat(np.arange(n), np.diff(Ap))
    Az[Ai == col] += 6.0j
    return n, Ap, Ai, Az, "lu", True


@functools.lru_cache(maxsize=None)
def matrices():
    """name -> case: the matrices held to the restatement and to the dense inverse.  (A pattern that stores an entry twice,
    cplx_cases' "diag_twice", is the plan's business only: cs3_analyze refuses duplicates, so no handle exists for it --
    tests/test_cselinv_cpu.py pins that, and holds the restatement to the dense inverse on it.)"""
    return {
        "ybus40": synth.ybus(40, 60, 1) + ("lu", True),
        "ybus300": synth.ybus(300, 420, 3) + ("lu", True),
        "ybus300_lossless": synth.ybus(300, 420, 3, lossless=True) + ("lu", True),
        "hermitian_pd": cplx_cases.hermitian_pd(120, 180, 11) + ("chol", False),
        "unsorted": structural("unsorted"),
    }


def rotations(name, case):
    """The settings of `rotate` a case is factorised with: LU on and off, Cholesky off.  Without resistance and without
    the rotation the first pivot is Re d = 0 exactly (tests/test_gpu_cplx.py pins the SingularMatrix), so that one is left."""
    if case[4] == "chol":
        return [False]
    return [True] if name.endswith("lossless") else [True, False]


def diagonal(n, seed):
    """cplx_cases.diagonal_matrix with magnitudes in [0.5, 2] and random phases: cond = max |a| / min |a| <= 4."""
    rng = np.random.default_rng(seed)
    n, Ap, Ai, _ = cplx_cases.diagonal_matrix(n, rng)
    Az = rng.uniform(0.5, 2.0, n) * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, n))
    return n, Ap, Ai, Az.astype(np.complex128), "lu", True


def gather_edge_orders():
    """n = nnz one below, at and one above a workgroup of the getters."""
    b = int(LIMITS.block)
    return [b - 1, b, b + 1]


def grid_stride_order():
    """One number more than a full grid holds: one lane loops once more."""
    return int(LIMITS.grid_cap * LIMITS.block + 1)


def batch_values(case, batch, seed):
    """[batch, nnz]: the case's values, every matrix with its own row phases (so that the rotations differ) and its own
    perturbation of a few per cent."""
    n, Ap, Ai, Az = case[:4]
    rng = np.random.default_rng(seed)
    out = np.empty((batch, len(Az)), dtype=np.complex128)
    for b in range(batch):
        phase = np.exp(1j * rng.uniform(-0.6, 0.6, n))
        out[b] = Az * phase[Ai] * (1.0 + 0.03 * rng.standard_normal(len(Az)))
    return out


# ---- dense roots of the real form across the kernel classes of the real selected inversion

def front_orders(F):
    """[(r, w, parent)] of the fronts of a Factorization, in schedule order."""
    ns = int(F.info.nsuper)
    sched, r, w = (np.empty(ns, dtype=np.int32) for _ in range(3))
    hip._check(hip.lib().cs3_debug_schedule(F._h, hip._pi(sched), hip._pi(r), hip._pi(w)))
    parent = F.supernodes()[1]
    return [(int(r[t]), int(w[t]), int(parent[sched[t]])) for t in range(ns)]


def real_root_orders(n, Ap, Ai):
    with hip.ComplexFactorization(n, Ap, Ai) as F:
        return [r for r, w, parent in front_orders(F.real) if parent < 0]


def with_phases(case, seed):
    """A_c = D1 A D2 of a real case (m, n, Ap, Ai, Ax) with unit-modulus D1, D2: cond_1 is that of A; the phases of the
    diagonal are near pi / 2, so the rotation matters."""
    n, Ap, Ai, Ax = case[1], case[2], case[3], case[4]
    rng = np.random.default_rng(seed)
    t1 = rng.uniform(0.0, 2.0 * np.pi, n)
    t2 = 0.5 * np.pi - t1 + rng.uniform(-0.2, 0.2, n)
    col = np.repeat(np.arange(n), np.diff(Ap))
    Az = np.asarray(Ax[:Ap[n]], dtype=np.float64) * np.exp(1j * (t1[Ai[:Ap[n]]] + t2[col]))
    return n, Ap, Ai, Az.astype(np.complex128), "lu", True


@functools.lru_cache(maxsize=None)
def dense_root(order2):
    """synth.dense_block_matrix(n, nd, 1) made complex, whose REAL FORM has a root front of exactly `order2` (even) rows:
    searched for as selinv_cases.dense_root searches, on the analysis of the real form; the dense matrix of order
    order2 / 2 where the analysis offers no such root with fronts below it."""
    assert order2 % 2 == 0
    half = order2 // 2
    for nd in range(half, max(half - 24, 1), -1):
        for extra in range(10, 100, 5):
            case = synth.dense_block_matrix(nd + extra, nd, 1)
            if real_root_orders(case[1], case[2], case[3]) == [order2]:
                return with_phases(case, order2)
    case = synth.dense_block_matrix(half, half, 1)
    assert real_root_orders(case[1], case[2], case[3]) == [order2]
    return with_phases(case, order2)


def dense_root_orders():
    """The even orders of the real root on either side of the wave and of the LDS limit of cs3_selinv_limits, and one beyond
    the LDS that is no multiple of the GEMM tile."""
    L = REAL_LIMITS
    even_below = lambda v: int(v) - int(v) % 2                 # noqa: E731  the largest even order <= v
    out = []
    for lim in (L.wave_max_order, L.lds_max_order):
        out += [even_below(lim), even_below(lim) + 2]
    ragged = 150
    assert ragged > L.lds_max_order and ragged % L.gemm_tile and ragged % 2 == 0
    return out + [ragged]
