"""The cases of tests/condest_cases.py against the traced NumPy port of dlacn2 alone (no GPU; dense LU and exact sparse
inverses do the solves): every case takes the path it is planned for, with every decision >= MARGIN away from its other
branch (generic) or with exactly the listed ties (exact); the exact family is exactly representable and stays so under
diagonal pivoting in any order; the generic ones pass the library's pivot acceptance in the handle's own order; and every
mutant of the port changes the result of some case, so the cases can see the errors they are there for."""
import itertools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import condest_cases as cc
from lacn2_ref import lacn2, lacn2_traced

ALL_GENERIC = dict(cc.GENERIC, **cc.SPD)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csparse3_amd", "csrc")


def _trace(c, **mutant):
    return lacn2_traced(c["n"], c["solve"], c["solve_t"], **mutant)


def test_the_constants_are_the_kernels():
    dev = open(os.path.join(CSRC, "cs3_device.hpp")).read()
    est = open(os.path.join(CSRC, "estimate.hip")).read()
    api = open(os.path.join(CSRC, "api.cpp")).read()
    assert re.search(r"constexpr long long EST_CHUNK = %d;" % cc.EST_CHUNK, dev)
    assert re.search(r"constexpr long long EST_NORM_COLS = %d;" % cc.EST_NORM_COLS, dev)
    assert re.search(r"constexpr int PART_NT = %d;" % cc.PART_NT, est)
    assert re.search(r"constexpr int EST_NT = %d;" % cc.SLOGDET_NT, est)
    assert "constexpr int FIXED_SLOTS = 11;" in api
    assert cc.BIG_N == 133121 and -(-cc.BIG_N // cc.EST_CHUNK) == 66


def test_the_traced_port_is_the_port():
    for name, (seed, spd, bare, _) in ALL_GENERIC.items():
        g = cc.generic_case(seed, spd, bare)
        est, solves, tr = _trace(g)
        assert (est, solves) == lacn2(g["n"], g["solve"], g["solve_t"]), name
        assert len(tr["path"]) == solves
    for name in cc.EXACT:
        c = cc.exact_case(name)
        assert _trace(c)[:2] == lacn2(c["n"], c["solve"], c["solve_t"]), name


@pytest.mark.parametrize("name", list(ALL_GENERIC))
def test_generic_case(hip, name):
    seed, spd, bare, cls = ALL_GENERIC[name]
    g = cc.generic_case(seed, spd, bare)
    n, D = g["n"], g["D"]
    A = sp.csc_matrix((g["Ax"], g["Ai"], g["Ap"]), shape=(n, n))
    b = np.random.default_rng(1).standard_normal(n)
    for fn, M in ((g["solve"], A), (g["solve_t"], A.T)):                 # the solvers are those of the stored matrix
        x = fn(b.copy())
        assert np.abs(M @ x - b).max() <= 1e-9 * (abs(M) @ np.abs(x)).max()
    est, solves, tr = _trace(g)
    assert cc.planned(tr, solves) == cls + ([],), name
    assert tr["margin"] >= cc.MARGIN and not tr["nonfinite"]
    if cls[3]:
        assert tr["t"] >= tr["est_j3"][-1] * (1.0 + 1e-3)                # J5 wins by 1e-3 at least
    if spd:
        assert np.array_equal(D, D.T) and np.linalg.eigvalsh(D).min() > 0.0
    elif bare:
        q = cc.handle_order(n, n)
        assert cc.max_multiplier(D[np.ix_(q, q)]) <= 1.0 / cc.TOL
    else:
        assert cc.lu_accepts(D, g["pad"])


def test_every_path_has_a_case():
    classes = {v[3] for v in ALL_GENERIC.values()} | {p[:4] for p in cc.PLANNED.values()}
    assert {c[0] for c in classes} >= {4, 5, 6, 7, 8, 9, 10, 11}
    # an even number of solves leaves the loop at J3, an odd one at J4: both J3 exits at 4 solves, both J4 exits at 11
    assert {(4, "same_signs", None), (4, "no_growth", None), (11, None, "repeat"), (11, None, "cap")} <= {c[:3] for c in classes}
    assert any(c[3] for c in classes)
    assert {4, 5, 7, 9, 11} <= {v[3][0] for v in cc.GENERIC.values() if not v[2]}      # one pattern: the LU batch
    assert {4, 5, 7, 9, 11} <= {v[3][0] for v in cc.SPD.values()}                      # the Cholesky batch
    assert cc.exact_case("no growth n2")["n"] == 2
    # 11 solves and J5 decides: what FIXED_SLOTS - 1 slots would get wrong (after 10 slots the estimate of "11" is final)
    assert {(11, None, "repeat", True), (11, None, "cap", True)} <= {v[3] for v in cc.GENERIC.values()}
    assert (11, None, "repeat", True) in {v[3] for v in cc.SPD.values()}


@pytest.mark.parametrize("name", list(cc.EXACT))
def test_exact_case(name):
    c = cc.exact_case(name)
    n = c["n"]
    # exactly representable: small multiples of 2^-12 in A, and (exact_matrix checked it) in A^-1
    v = c["Ax"] * 4096.0
    assert np.array_equal(v, np.round(v)) and np.abs(c["Ax"]).max() <= 4096.0
    # diagonal pivoting in ANY order stays in the family and passes the acceptance rule
    for pos, B in c["blocks"]:
        for perm in itertools.permutations(range(len(B))):
            P = B[np.ix_(perm, perm)]
            assert cc.max_multiplier(P) <= 4.0 <= 1.0 / cc.TOL
            L = np.eye(len(P))
            W = P.copy()
            for j in range(len(P) - 1):
                L[j + 1:, j] = W[j + 1:, j] / W[j, j]
                W[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], W[j, j + 1:])
            Uf = np.triu(W)
            assert np.array_equal(L @ Uf, P) and np.array_equal(L * 4096.0, np.round(L * 4096.0))
            assert np.all(np.frexp(np.abs(np.diag(Uf)))[0] == 0.5)       # the pivots are +-2^e
    est, solves, tr = _trace(c)
    assert cc.planned(tr, solves) == cc.PLANNED[name]
    assert tr["margin"] >= cc.MARGIN
    if not tr["j5_won"]:
        assert est * 4096.0 == round(est * 4096.0)                      # an exact sum
    kind, a = cc.EXACT[name]
    if kind in ("tie", "pair", "dense"):
        est_last, _, tr_last = _trace(c, last_argmax=True)
        assert est_last != est, "the tie decides nothing"
        (at, idx), = tr["ties"]
    if kind in ("tie", "pair"):                                          # the largest column of A is where it is planned
        sums = np.asarray(abs(c["A"]).sum(axis=0)).reshape(-1)
        assert np.flatnonzero(sums == sums.max()).tolist() == [a[5]] and sums.max() == 4096.0
        assert tr["path"][at][1] == idx[0] and tr_last["path"][at][1] == idx[-1]
    if kind == "straddle":
        assert a[1] < cc.EST_CHUNK <= a[1] + 2
        assert tr["sign_diff"][0] and min(tr["sign_diff"][0]) >= cc.EST_CHUNK     # only part 1 sees the change of sign
        assert est != tr["est_j3"][0]                                            # and losing it ends one round early


def test_the_ties_sit_at_the_partition_edges():
    first = {cc.PLANNED[k][4][0][1][0] for k in cc.PLANNED if k.startswith(("tie", "big"))}
    last = {cc.PLANNED[k][4][0][1][-1] for k in cc.PLANNED if k.startswith(("tie", "big"))}
    assert {0, 255, 256, 2047, 2048} <= first | {2}             # entry 0's block wins at its row 2; "ends" at row 0
    assert {256, 2047, 2048, 4096, 2046} <= last                # losers: stride 2, chunk edge, n - 1 of 2047 / 2048 / 2049 / 4097
    assert {cc.EXACT[k][1][0] for k in cc.EXACT if k.startswith("tie")} == {2047, 2048, 2049, 4097}
    w, l = cc.PLANNED["big J2 part 64"][4][0][1]
    assert w // cc.EST_CHUNK == 64 and l // cc.EST_CHUNK == 65          # both in k_est_finish's second round
    w, l = cc.PLANNED["big J2 same lane"][4][0][1]
    assert w // cc.EST_CHUNK == 1 and l // cc.EST_CHUNK == 65           # lane 1 meets the winner first, then the loser
    norm_cols = {cc.EXACT[k][1][5] for k in cc.EXACT if cc.EXACT[k][0] in ("tie", "pair")}
    assert {255, 256, 257, 258, 2047, 4095, 4096, 16384 + 255, 20000} <= norm_cols
    assert 4096 == cc.EXACT["tie J2 n4097 norm last"][1][0] - 1


MUTANTS = {
    "ITMAX = 4": dict(itmax=4),
    "last argmax": dict(last_argmax=True),
    "< for <= at J3": dict(strict_growth=True),
    "J5 dropped": dict(drop_j5=True),
    "iter starts at 1": dict(iter0=1),
}
CAUGHT_BY = {                                                   # at least these (asserted as a subset)
    "ITMAX = 4": {"11", "11 cap", "spd 11"},
    "last argmax": {"issue example", "tie J2 n2048 stride", "tie J4 n4097 straddle", "big J2 same lane", "big J4"},
    "< for <= at J3": {"no growth n2", "no growth n4"},
    "J5 dropped": {"J5 wins", "11 J5 wins", "11 cap J5 wins", "spd 11 J5 wins", "no growth n2", "no growth n4"},
    "iter starts at 1": {"11 cap"},
}


def test_every_mutant_changes_some_case():
    cases = {name: (cc.generic_case(*v[:3]), False) for name, v in ALL_GENERIC.items()}
    cases.update({name: (cc.exact_case(name), True) for name in cc.EXACT})
    base = {name: _trace(c)[0] for name, (c, _) in cases.items()}
    for mutant, kw in MUTANTS.items():
        caught = set()
        for name, (c, exact) in cases.items():
            got = _trace(c, **kw)[0]
            if (got != base[name]) if exact else (abs(got - base[name]) > 1e-6 * base[name]):
                caught.add(name)
        assert caught >= CAUGHT_BY[mutant], (mutant, sorted(caught))


@pytest.mark.parametrize("n, spd", [(k, False) for k in cc.SLOGDET_N if k > cc.SLOGDET_NT] + [(cc.SLOGDET_NT + 1, True)])
def test_slogdet_matrices_have_pure_diagonal_pivots_in_the_second_round(hip, n, spd):
    Ap, Ai, Ax, dpos = cc.slogdet_matrix(n, spd=spd)
    assert np.array_equal(Ai[dpos], np.arange(n)) and np.all(Ax > -1.0)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    if spd:
        assert abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A.toarray()).min() > 0.0
    with hip.Factorization(n, n, Ap, Ai, kind=hip.CS3_CHOLESKY if spd else hip.CS3_LU) as F:
        q = F.ordering()["q"]
    pure = cc.pure_diagonal(n)
    assert pure[q[cc.SLOGDET_NT - 1]] and pure[q[cc.SLOGDET_NT]]
    assert np.flatnonzero(pure[q])[-1] > cc.SLOGDET_NT or n == cc.SLOGDET_NT + 1


def test_slogdet_sizes_are_the_kernels_edges():
    assert set(cc.SLOGDET_N) >= {1, 63, 64, 65, cc.SLOGDET_NT - 1, cc.SLOGDET_NT, cc.SLOGDET_NT + 1, 2 * cc.SLOGDET_NT + 1}
