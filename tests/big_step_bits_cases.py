"""The cases of tests/test_gpu_big_step_bits.py and tests/golden/make_big_step_bits.py, and the one routine both run: the
factors and the fused one-right-hand-side solution of a matrix whose big fronts go through k_big_step (csrc/kernels.hip),
as SHA-256 digests of their bytes.

The matrices are those of tests/wide_chunk_cases.py, the smallest at which k_big_step changes what it does:

  case      root                   non-root (r, w)          what it exercises
  d129s30   288 = 9 full blocks    (159, 129)               a last block of ONE pivot and a closing launch with cw = 1
  d160s30   350, last block of 30  (190, 160) = 5 blocks    short and exact blocks
  d130s200  460                    (330, 130)               200 rows below the pivots: trailing tiles with nsl up to 4, and
                                                            a ragged last tile

Each as LU and as Cholesky (the bi < bj return, the lower-triangle stores), in batches of 1, 2 and 7 (the blockIdx.z / batch
split); one LU case with pivot perturbation on (the PivotRule<true> instance; the threshold lies far below every pivot, so
nothing is replaced and the factors are those of the plain instance)."""
import hashlib

import numpy as np

import launch_plan_cases as lp
import wide_chunk_cases as wc

NAMES = ("d129s30", "d160s30", "d130s200")
KINDS = ("lu", "chol")
BATCHES = (1, 2, 7)
LU_TOL = 1e-3
DELTA = 1e-12
# (name, kind, batch, perturbation on)
CASES = [(name, kind, batch, False) for name in NAMES for kind in KINDS for batch in BATCHES] + [("d130s200", "lu", 2, True)]


def case_id(c):
    name, kind, batch, perturb = c
    return "%s-%s-b%d%s" % (name, kind, batch, "-perturb" if perturb else "")


def has_big_block_steps(hip, F, op):
    rows = lp.plan(hip, F, op, 1)
    return bool(np.any(rows[:, lp.KIND] == lp.BIG_BLOCK))


def record(hip, case):
    """Factor, read the factors back, then one fused refactor + solve.  -> {"Lx", "Ux", "x": SHA-256 of the bytes (all
    matrices of the batch, in order), "sum_*": their sums, for a readable failure}.  Asserts that the plans of the
    factorisation and of the fused step hold BIG_BLOCK steps: the case runs k_big_step, not k_front_wg."""
    import torch
    name, kind, batch, perturb = case
    sym = kind == "chol"
    m, n, Ap, Ai, _ = wc.case_matrix(name, symmetric=sym)
    AX = wc.case_values(name, batch, symmetric=sym)
    tol = 0.0 if sym else LU_TOL
    B = np.random.default_rng(4200 + batch).standard_normal((batch, n, 1))
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY if sym else hip.CS3_LU, batch=batch) as F:
        for op in ("factor", "fused"):
            assert has_big_block_steps(hip, F, op), "%s: the %s plan holds no BIG_BLOCK step" % (case_id(case), op)
        if perturb:
            F.set_perturbation(DELTA)
        F.factor(AX, tol)
        parts = [F.factors(b) for b in range(batch)]
        Lx = np.concatenate([p[2] for p in parts])
        Ux = np.concatenate([p[5] for p in parts]) if not sym else np.zeros(0)
        if perturb:
            assert not F.perturbed().any()
        d_ax = torch.from_numpy(AX.copy()).to(dev)
        d_b = torch.from_numpy(B).to(dev)
        d_x = torch.zeros_like(d_b)
        F.factor_solve_bx_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, tol, sh)
        F.factor_status(sh)
        x = d_x.cpu().numpy()
    out = {}
    for key, a in (("Lx", Lx), ("Ux", Ux), ("x", x)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        out[key] = hashlib.sha256(a.tobytes()).hexdigest()
        out["sum_" + key] = repr(float(a.sum()))
    return out
