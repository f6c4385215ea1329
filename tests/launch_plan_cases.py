"""The launch plans that tests/test_launch_plan_cpu.py pins (csrc/schedule.cpp, printed by cs3_debug_launch_plan): the
handles, the operations on each, and the scheduler branch every operation is there for.  All of it is analysis only: no
device.  tests/golden/make_launch_plans.py records the same list from a library that still schedules by control flow."""
import ctypes as C

import numpy as np

import few_rhs_cases as fr
import forest_cases as fc
import schur_cases as shc
import sweep_cases as sc
import wide_chunk_cases as wc

# columns of a plan row (include/csparse3_amd.h: cs3_debug_launch_plan)
KIND, SLOT, FIRST, COUNT, CLS, LEVEL, MAX_R, MAX_W, ARG, EVENT = range(10)
# step kinds (cs3_device.hpp: StepKind)
FRONT_GROUP, BIG_GATHER, BIG_BLOCK, SCHUR_TAKE, SWEEP_FWD, SWEEP_BWD, FWD_PRE, FWD_CHUNK, BWD_PRE, BWD_CHUNK, RECORD, WAIT = range(12)
FACTOR_STEPS = (FRONT_GROUP, BIG_GATHER, BIG_BLOCK, SCHUR_TAKE)
FWD_STEPS = (SWEEP_FWD, FWD_PRE, FWD_CHUNK)
BWD_STEPS = (SWEEP_BWD, BWD_PRE, BWD_CHUNK)
AUX = 4                                           # stream slot of ForkJoin::aux; 1 .. 3: the side streams
FC_BIG, FC_IL, FC_SUB, FC_SCHUR = 4, 5, 6, 7      # cs3_internal.hpp: FrontClass
SK_BIG, SK_IL, SK_SUB = 3, 4, 5                   #                   SolveKind
BIG_NB = 32                                       # cs3_device.hpp: pivots per block-step launch
OPS = {"factor": 0, "fwd": 1, "bwd": 2, "fused": 3, "schur_fwd": 4, "schur_bwd": 5}

FOREST_CASE = "arena5014"     # the smallest case of forest_cases with a forest and levels above it
IL_BATCH = 128                # symbolic.cpp: CS3_IL_MIN_BATCH, from this batch on fronts of order <= 16 are FC_IL / SK_IL
IL_CASES = ("one", "ea")      # the smallest cases of forest_cases with FC_IL fronts alone / beside other fronts of a level
SCHUR_CASE = ("toy10", 3)     # the smallest case of schur_cases
FORK_CASE = "block"           # few_rhs_cases: levels of two and three launch groups (no case of the suite has more)


def matrix(name, symmetric=False):
    """-> (m, n, Ap, Ai, schur index list or None, natural order?) of handle `name`."""
    if name in wc.CASES:
        return wc.case_matrix(name, symmetric=symmetric)[:4] + (None, False)
    if name == "d300s30":
        return sc.blocks_on_separator((300,) * 4, 30, 1, symmetric=symmetric)[:4] + (None, False)
    if name in fc.CASES:
        M = fc.case_matrix(name, symmetric=symmetric)
        return M.m, M.n, M.Ap, M.Ai, None, True
    if name == FORK_CASE:
        return fr.case_matrix(name, symmetric=symmetric)[:4] + (None, False)
    if name == SCHUR_CASE[0]:
        return shc.matrix(name)[:4] + (shc.schur_set(*SCHUR_CASE), False)
    raise KeyError(name)


def handle(hip, name, batch=1, symmetric=False):
    m, n, Ap, Ai, idx, natural = matrix(name, symmetric)
    kw = dict(kind=hip.CS3_CHOLESKY if symmetric else hip.CS3_LU, batch=batch)
    if natural:
        kw["q"] = np.arange(n, dtype=np.int32)          # (as forest_cases.handle: the trees are built in elimination order)
    if idx is not None:
        kw["schur"] = idx
    return hip.Factorization(m, n, Ap, Ai, **kw)


def plan(hip, F, op, nrhs=1, trans=False):
    """cs3_debug_launch_plan -> int32 [steps, 10]."""
    f = hip.lib().cs3_debug_launch_plan
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int64]
    f.restype = C.c_int64
    n = int(f(F._h, OPS[op], nrhs, int(trans), None, 0))
    assert n >= 0, hip.lib().cs3_last_error()
    rows = np.zeros((max(n, 1), 10), dtype=np.int32)
    assert f(F._h, OPS[op], nrhs, int(trans), rows.ctypes.data_as(C.POINTER(C.c_int32)), n) == n
    return rows[:n]


# (handle, symmetric, batch, op, nrhs, trans, environment, branch): the branch is what branch_of says of the plan
CASES = []
# the dense root's chain; 8 right-hand sides: 64-column chunks of two block steps, so more of them are released
for _name, _k in (("d129s30", (0, 0, 0, 2)), ("d256s30", (1, 1, 1, 5)), ("d300s30", (2, 2, 2, 6))):
    CASES += [(_name, False, 1, "fused", _nrhs, False, {}, "root chain, %d released" % _kk) for _nrhs, _kk in zip((1, 2, 7, 8), _k)]
CASES += [
    ("d256s30", False, 1, "fused", 16, False, {}, "fork"),                     # GEMM sweeps, no root chain
    ("d256s30", False, 1, "fused", 512, False, {}, "fork"),
    ("d256s30", False, 1, "fwd", 512, False, {}, "in line"),                   # (one launch group per level: nothing to fork)
    (FORK_CASE, False, 1, "fwd", 512, False, {}, "forked levels"),
    (FORK_CASE, False, 1, "bwd", 512, False, {}, "forked levels"),
    (FORK_CASE, False, 1, "fused", 512, False, {}, "fork"),
    (FORK_CASE, False, 1, "fused", 1, False, {}, "root chain, 0 released"),
    (FORK_CASE, False, 1, "factor", 1, False, {}, "forked levels"),
    ("d256s30", False, 1, "factor", 1, False, {}, "in line"),
    ("d256s30", False, 1, "fwd", 1, True, {}, "in line"),
    ("d129s30", False, 16, "fused", 1, False, {}, "levels on aux"),
    ("d129s30", False, 48, "fused", 1, False, {}, "levels on aux"),           # big fronts in one workgroup
    ("d129s30", False, 48, "factor", 1, False, {}, "in line"),
    (IL_CASES[0], False, IL_BATCH, "fused", 1, False, {}, "levels on aux"),
    (IL_CASES[1], False, IL_BATCH, "fused", 1, False, {}, "levels on aux"),
    (IL_CASES[1], False, IL_BATCH, "bwd", 2, False, {}, "in line"),
    (FOREST_CASE, False, 1, "fused", 1, False, {}, "fork"),                    # forest schedule, fwd_in_factor
    (FOREST_CASE, False, 1, "fused", 2, False, {}, "no overlap"),              # level schedule over a forest
    (FOREST_CASE, False, 1, "fwd", 1, False, {}, "in line"),
    (FOREST_CASE, False, 1, "fwd", 1, True, {}, "in line"),                    # transposed: the level schedule
    (FOREST_CASE, False, 1, "bwd", 1, True, {}, "in line"),
    ("d256s30", True, 1, "fused", 1, False, {}, "root chain, 1 released"),
    (SCHUR_CASE[0], False, 1, "factor", 1, False, {}, "in line"),              # FC_SCHUR: gather, then take
    (SCHUR_CASE[0], False, 1, "schur_fwd", 1, False, {}, "in line"),
    (SCHUR_CASE[0], False, 1, "schur_bwd", 1, False, {}, "in line"),
    ("d256s30", False, 1, "fused", 1, False, {"CS3_NO_OVERLAP": "1"}, "no overlap"),
    ("d256s30", False, 1, "fused", 16, False, {"CS3_NO_GEMM_SWEEPS": "1"}, "fork"),
]


def case_id(c):
    name, sym, batch, op, nrhs, trans, env, _ = c
    return "%s%s-b%d-%s-k%d%s%s" % (name, "-chol" if sym else "", batch, op, nrhs, "-T" if trans else "",
                                    "".join("-" + k for k in sorted(env)))


def branch_of(rows, op):
    """The scheduler branch a plan took, read off the plan.  Factorisations and sweeps: 'forked levels' when a side
    stream is used, else 'in line'.  Fused steps: 'no overlap' (nothing on aux); 'root chain, K released' (steps on aux are
    issued between the block steps of the last level: K chunks of its forward sweep among them); 'levels on aux' (aux
    waits once per level); 'fork' (aux waits once)."""
    if op != "fused":
        return "forked levels" if np.any((rows[:, SLOT] >= 1) & (rows[:, SLOT] < AUX)) else "in line"
    aux = np.flatnonzero(rows[:, SLOT] == AUX)
    if len(aux) == 0:
        return "no overlap"
    top = rows[np.isin(rows[:, KIND], FACTOR_STEPS)][:, LEVEL].max()
    blocks = np.flatnonzero((rows[:, KIND] == BIG_BLOCK) & (rows[:, LEVEL] == top))
    if len(blocks) and np.any((aux > blocks[0]) & (aux < blocks[-1])):
        return "root chain, %d released" % np.sum((rows[aux, KIND] == FWD_CHUNK) & (rows[aux, LEVEL] == top))
    return "levels on aux" if np.sum(rows[aux, KIND] == WAIT) > 1 else "fork"
