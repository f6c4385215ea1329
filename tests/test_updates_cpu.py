"""Low-rank-modified solves (cs3_updates_*), the part that needs no GPU: the NumPy reference of the formula
(tests/updates_ref.py) pinned against the definition -- a factorisation of every modified matrix -- and the plan's
argument checks, its info and the state error of a solve before a factorisation."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from csparse3_amd import synth
from helpers import RTOL, csc_to_scipy, rel_err
import updates_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SING_TOL = 1e-10
SYMBOLS = ("cs3_updates_plan", "cs3_updates_free", "cs3_updates_info", "cs3_updates_solve_dev", "cs3_updates_solve",
           "cs3_debug_alloc_counters")


def _spd4000():
    ei, ej = synth.spd_grid_pattern(4000, seed=4000)
    return synth.spd_grid_matrix(4000, ei, ej, seed=4001)


MATRICES = {
    "toy10": (lambda: synth.toy10()[:5], None),                      # all 12 pairs
    "jacobian118": (synth.jacobian_like, 100),
    "config2": (synth.jacobian_config2, 100),
    "grid5000": (lambda: synth.grid_jacobian(5000), 40),
    "grid50000": (synth.grid_jacobian, 30),
    "spd4000": (_spd4000, 40),
    "denseblock150": (lambda: synth.dense_block_matrix(n=400, nd=150, seed=2), 100),
}


@pytest.mark.parametrize("name", list(MATRICES))
def test_reference_matches_a_factorisation_of_every_modified_matrix(name):
    """The reference alone: branch outages within RTOL of splu(A + dA_c), healthy cases far above SING_TOL and the
    constructed-singular ones far below it, so the threshold separates them before a GPU is involved."""
    make, count = MATRICES[name]
    m, n, Ap, Ai, Ax = make()
    A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()
    b = np.random.default_rng(17).standard_normal(n)
    healthy = ur.branch_outages(A, count, seed=23)
    sing = [ur.singular_case(A, int(i)) for i in np.random.default_rng(29).choice(n, size=min(n, 10), replace=False)]
    X, rpiv, cond = ur.solve_updates_ref(A, b, healthy + sing, SING_TOL)
    worst = 0.0
    for c, case in enumerate(healthy):
        err = rel_err(X[:, c], ur.direct_solve(A, case, b))
        worst = max(worst, err)
        assert err <= RTOL, "%s case %d: %.3e" % (name, c, err)
    nh = len(healthy)
    print("%s: worst error %.2e, smallest healthy rpiv %.2e, largest singular rpiv %.2e, worst cond(S) %.1f"
          % (name, worst, rpiv[:nh].min(), rpiv[nh:].max(), cond[:nh].max()))
    assert rpiv[:nh].min() >= 1e-6
    assert rpiv[nh:].max() <= 1e-13
    assert np.isnan(X[:, nh:]).all() and np.isfinite(X[:, :nh]).all()


def test_reference_adds_duplicates_and_takes_rectangular_cases():
    m, n, Ap, Ai, Ax = synth.jacobian_like()
    A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()
    b = np.random.default_rng(3).standard_normal(n)
    rng = np.random.default_rng(4)
    cases = [(np.array([5, 5, 5]), np.array([7, 7, 9]), np.array([0.25, 0.5, -0.1])),               # duplicates add
             (np.full(9, 11), np.arange(20, 29), 0.1 * rng.standard_normal(9)),                    # one row x 9 columns
             (np.arange(30, 39), np.full(9, 3), 0.1 * rng.standard_normal(9)),                     # 9 rows x one column
             (np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0))]                        # empty
    X, rpiv, _ = ur.solve_updates_ref(A, b, cases)
    for c, case in enumerate(cases):
        assert rel_err(X[:, c], ur.direct_solve(A, case, b)) <= RTOL
    assert rpiv[3] == 1.0


# ---- the plan: host only -------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_exported(hip):
    lib = hip.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libcsparse3_hip.so does not export " + name


def _toy(hip, **kw):
    m, n, Ap, Ai, Ax, b, xt = synth.toy10()
    return n, Ax, b, hip.Factorization(m, n, Ap, Ai, **kw)


def _plan_rc(hip, F, ncases, cp, ci, cj, out=True):
    lib = hip.lib()
    u = C.c_void_p()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    cp, ci, cj = arr(cp), arr(ci), arr(cj)
    rc = lib.cs3_updates_plan(F._h, ncases, hip._pi(cp), hip._pi(ci), hip._pi(cj), C.byref(u) if out else None)
    msg = lib.cs3_last_error().decode()
    if u:
        lib.cs3_updates_free(u)
    return rc, msg


def test_plan_argument_errors(hip):
    n, Ax, b, F = _toy(hip)
    with F:
        ok = ([0, 2], [1, 2], [2, 1])
        assert _plan_rc(hip, F, 1, *ok)[0] == 0
        assert _plan_rc(hip, F, 1, *ok, out=False)[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, 1, None, [1, 2], [2, 1])[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, 1, [0, 2], None, [2, 1])[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, 1, [0, 2], [1, 2], None)[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, 0, [0], [], [])[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, -3, [0], [], [])[0] == hip.CS3_ERR_ARG
        assert _plan_rc(hip, F, 2, [0, 2, 1], [1, 2], [2, 1])[0] == hip.CS3_ERR_ARG             # cp not monotone
        for bad in (-1, n):
            assert _plan_rc(hip, F, 1, [0, 2], [1, bad], [2, 1])[0] == hip.CS3_ERR_ARG
            assert _plan_rc(hip, F, 1, [0, 2], [1, 2], [bad, 1])[0] == hip.CS3_ERR_ARG
        # an error earlier in the documented order wins: a bad index in case 0 and a bad cp further on
        rc, msg = _plan_rc(hip, F, 2, [0, 1, 0], [n], [0])
        assert rc == hip.CS3_ERR_ARG and "monotone" in msg
    m, n, Ap, Ai, Ax = synth.jacobian_like()
    with hip.Factorization(m, n, Ap, Ai) as F:
        seventeen = np.arange(17)
        rc, msg = _plan_rc(hip, F, 2, [0, 1, 18], np.r_[0, seventeen], np.r_[0, np.zeros(17, dtype=int)])
        assert rc == hip.CS3_ERR_ARG and "case 1" in msg                                       # 17 distinct rows
        rc, msg = _plan_rc(hip, F, 2, [0, 1, 18], np.r_[0, np.zeros(17, dtype=int)], np.r_[0, seventeen])
        assert rc == hip.CS3_ERR_ARG and "case 1" in msg                                       # 17 distinct columns
        sixteen = np.arange(16)
        assert _plan_rc(hip, F, 1, [0, 32], np.r_[sixteen, sixteen], np.r_[sixteen, sixteen[::-1]])[0] == 0
    n, Ax, b, F = _toy(hip, batch=2)
    with F:
        assert _plan_rc(hip, F, 1, [0, 2], [1, 2], [2, 1])[0] == hip.CS3_ERR_ARG               # batched handles: out of scope


def test_plan_info_of_a_hand_made_list(hip):
    n, Ax, b, F = _toy(hip)
    cases = [((0, 1, 0, 1), (1, 0, 0, 1)),          # rows {0, 1}, columns {0, 1}
             ((1, 2), (2, 1)),                      # rows {1, 2}
             ((), ()),                              # empty
             ((5, 5, 5), (1, 2, 3)),                # one row, three columns
             ((7, 8, 9), (4, 4, 4)),                # three rows, one column
             ((0,), (0,))]
    with F, F.updates_plan(cases) as plan:
        info = plan.info
        assert (info.ncases, info.nrows_unique, info.max_rank, info.ntiles) == (6, 7, 3, 1)
    flat = (np.array([0, 4, 6, 6, 9, 12, 13]), np.array([0, 1, 0, 1, 1, 2, 5, 5, 5, 7, 8, 9, 0]),
            np.array([1, 0, 0, 1, 2, 1, 1, 2, 3, 4, 4, 4, 0]))
    with hip.Factorization(*synth.toy10()[:4]) as F, F.updates_plan(flat) as plan:
        assert plan.info.nrows_unique == 7 and plan.info.ncases == 6


def test_tile_override_is_read_at_plan_time():
    """CS3_UPD_TILE = 3: {0, 1} | {1, 2} + empty + {5} | {7, 8, 9} | {0} -- a row shared by two tiles is counted once in
    nrows_unique and solved in both.  (A child process: the switch must not leak into this one.)"""
    code = ("import numpy as np\n"
            "from csparse3_amd import csc_hip as hip, synth\n"
            "cases = [((0, 1, 0, 1), (1, 0, 0, 1)), ((1, 2), (2, 1)), ((), ()), ((5, 5, 5), (1, 2, 3)),\n"
            "         ((7, 8, 9), (4, 4, 4)), ((0,), (0,))]\n"
            "with hip.Factorization(*synth.toy10()[:4]) as F, F.updates_plan(cases) as p:\n"
            "    i = p.info\n"
            "    print(i.ncases, i.nrows_unique, i.max_rank, i.ntiles)\n")
    for tile, want in (("3", "6 7 3 4"), ("1", "6 7 3 4"), ("4", "6 7 3 2"), ("1024", "6 7 3 1")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, CS3_UPD_TILE=tile),
                             capture_output=True, text=True, check=True).stdout
        assert out.split() == want.split(), (tile, out)


def test_solve_before_a_factorisation_is_a_state_error(hip):
    n, Ax, b, F = _toy(hip)
    with F, F.updates_plan([((0, 1), (1, 0))]) as plan:
        with pytest.raises(hip.Cs3Error) as e:
            F.solve_updates(plan, np.ones(2), b)
        assert e.value.code == hip.CS3_ERR_STATE
        with pytest.raises(hip.Cs3Error) as e:
            F.solve_updates_dev(plan, 8, 8, 8)
        assert e.value.code == hip.CS3_ERR_STATE
        with pytest.raises(hip.Cs3Error) as e:                                                 # null arguments come first
            F.solve_updates_dev(plan, 0, 8, 8)
        assert e.value.code == hip.CS3_ERR_ARG
        n2, Ax2, b2, G = _toy(hip)
        with G:
            with pytest.raises(hip.Cs3Error) as e:                                             # another handle's plan
                G.solve_updates_dev(plan, 8, 8, 8)
            assert e.value.code == hip.CS3_ERR_ARG


def test_plan_and_handle_may_be_freed_in_either_order(hip):
    n, Ax, b, F = _toy(hip)
    plan = F.updates_plan([((0, 1), (1, 0))])
    F.close()
    assert plan.info.ncases == 1
    plan.close()
    n, Ax, b, F = _toy(hip)
    plan = F.updates_plan([((0, 1), (1, 0))])
    plan.close()
    F.close()
