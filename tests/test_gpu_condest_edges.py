"""The condition estimator (estimate.hip, condest_run in api.cpp) and k_slogdet on the cases of tests/condest_cases.py:
every path of dlacn2's state machine, the fixed 11 slots and the adaptive driver on batches whose members finish after
4 .. 11 solves, ties of |x_i| and sign changes at the edges of the fixed partition (thread stride, chunk, the second
round of k_est_finish's part loop), the column-norm partition, the non-finite exit, and k_slogdet's second round.

The reference is the traced NumPy port of dlacn2 (tests/lacn2_ref.py) driven by the handle's OWN solves, F.solve(b) and
F.solve(b, trans=True): they and the estimator's internal solves are the same run_solve(h, x, 1, 0, stream, trans), so
the state machine, the reductions and the slot drivers are compared alone.  Generic cases:
|inv_gpu - inv_port| <= 2 (n + 2) 2^-53 inv_port (condest_cases.bound); exact cases: the same bits unless J5 wins.
Every test asserts the path it is there for from the trace of its own run (tests/test_condest_cases_cpu.py proves the
same plan without a device)."""
import numpy as np
import pytest

import condest_cases as cc
from lacn2_ref import lacn2_traced

pytestmark = pytest.mark.gpu

_SINGLE = {}                                                     # case name -> its single-matrix result, computed once


def _kind(gpu, spd):
    return gpu.CS3_CHOLESKY if spd else gpu.CS3_LU


def _factor(F, AX, spd):
    return F.factor(AX) if spd else F.factor(AX, cc.TOL)


def _condest_dev(F, AX):
    import torch
    dev = torch.device("cuda", 0)
    d_ax = torch.from_numpy(np.ascontiguousarray(AX, dtype=np.float64).reshape(-1).copy()).to(dev)
    d_c = torch.full((F.batch,), -1.0, dtype=torch.float64, device=dev)
    d_i = torch.full_like(d_c, -1.0)
    F.condest_dev(d_ax.data_ptr(), d_c.data_ptr(), d_i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_c.cpu().numpy(), d_i.cpu().numpy()


def _both_forms(F, AX):
    """condest, condest_dev, condest again, condest_dev again: the same bits -> (cond, inv)."""
    c1, i1 = F.condest(AX)
    c2, i2 = _condest_dev(F, AX)
    c3, i3 = F.condest(AX)
    c4, i4 = _condest_dev(F, AX)
    for c, i in ((c2, i2), (c3, i3), (c4, i4)):
        assert np.array_equal(c1, c, equal_nan=True) and np.array_equal(i1, i, equal_nan=True)
    return c1, i1


def _port(F, n, b=0):
    """The traced port on member b of the handle's batch through the handle's own solves: b's vector in its row of a
    [batch, n] right-hand side, zeros in the others (what k_est_prepare gives an idle matrix)."""
    def make(trans):
        def fn(v):
            X = np.zeros((F.batch, n))
            X[b] = v
            return F.solve(X, trans=trans)[b]
        return fn
    return lacn2_traced(n, make(False), make(True))


def _norm1(n, Ap, Ax):
    """max_j sum_i |a_ij|, every column summed in storage order."""
    a = np.abs(np.asarray(Ax, dtype=np.float64))
    best = 0.0
    for j in np.flatnonzero(np.diff(Ap) > 1):
        s = 0.0
        for v in a[Ap[j]:Ap[j + 1]]:
            s += v
        best = max(best, s)
    one = np.flatnonzero(np.diff(Ap) == 1)
    return max(best, float(a[Ap[one]].max())) if len(one) else best


def _check_norm(gpu, n, Ap, Ax, cond, inv):
    norm = _norm1(n, Ap, Ax)
    assert norm == gpu.csc_norm(n, Ap, Ax)
    assert cond == norm * inv, "cond %.17g, ||A||_1 %.17g, inv %.17g" % (cond, norm, inv)


def _generic_single(gpu, name):
    if name not in _SINGLE:
        seed, spd, bare, cls = dict(cc.GENERIC, **cc.SPD)[name]
        g = cc.generic_case(seed, spd, bare)
        n = g["n"]
        with gpu.Factorization(n, n, g["Ap"], g["Ai"], kind=_kind(gpu, spd)) as F:
            _factor(F, g["Ax"], spd)
            cond, inv = _both_forms(F, g["Ax"])
            est, solves, tr = _port(F, n)
        _SINGLE[name] = dict(g=g, cond=cond[0], inv=inv[0], est=est, solves=solves, tr=tr, cls=cls)
    return _SINGLE[name]


# 1. every path: the number of solves, the exit of J3 or J4, J5's alternative
@pytest.mark.parametrize("name", list(cc.GENERIC) + list(cc.SPD))
def test_generic_paths(gpu, name):
    r = _generic_single(gpu, name)
    g, tr = r["g"], r["tr"]
    print("%s: inv %.17g port %.17g solves %d margin %.3g" % (name, r["inv"], r["est"], r["solves"], tr["margin"]))
    assert cc.planned(tr, r["solves"]) == r["cls"] + ([],)
    assert tr["margin"] >= cc.MARGIN
    if r["cls"][3]:
        assert tr["t"] >= tr["est_j3"][-1] * (1.0 + 1e-3)
    assert abs(r["inv"] - r["est"]) <= cc.bound(g["n"], r["est"])
    _check_norm(gpu, g["n"], g["Ap"], g["Ax"], r["cond"], r["inv"])


# 2. ties of |x_i|, sign changes and the largest column at the edges of the partitions; est == estold; n = 2
@pytest.mark.parametrize("name", list(cc.EXACT))
def test_exact_cases(gpu, name):
    c = cc.exact_case(name)
    n = c["n"]
    with gpu.Factorization(n, n, c["Ap"], c["Ai"]) as F:
        F.factor(c["Ax"], cc.TOL)
        cond, inv = _both_forms(F, c["Ax"])
        est, solves, tr = _port(F, n)
    print("%s: inv %.17g port %.17g solves %d ties %r" % (name, inv[0], est, solves, tr["ties"]))
    assert cc.planned(tr, solves) == cc.PLANNED[name]
    assert tr["margin"] >= cc.MARGIN
    if tr["j5_won"]:
        assert abs(inv[0] - est) <= cc.bound(n, est)
    else:
        assert inv[0] == est
    _check_norm(gpu, n, c["Ap"], c["Ax"], cond[0], inv[0])
    kind, a = cc.EXACT[name]
    if kind in ("tie", "pair"):
        assert _norm1(n, c["Ap"], c["Ax"]) == 4096.0 and c["A"][a[5], a[5]] == 4096.0     # the largest column is where planned


# 3. slots: members with different paths in one batch, through the adaptive and the fixed driver
LU_MEMBERS = [k for k, v in cc.GENERIC.items() if not v[2]]
SPD_MEMBERS = list(cc.SPD)


@pytest.mark.parametrize("spd", [False, True])
@pytest.mark.parametrize("nb", [5, 66, 256])
def test_batches_of_different_paths(gpu, nb, spd):
    if nb == 5:
        names = ["spd 4", "spd 5", "spd 7", "spd 9", "spd 11"] if spd else ["4 same signs", "5", "7", "9", "11"]
    else:
        pool = SPD_MEMBERS if spd else LU_MEMBERS
        names = [pool[(b * 7 + b // 64) % len(pool)] for b in range(nb)]     # both sides of every 64 see every path
    single = {k: _generic_single(gpu, k) for k in set(names)}
    assert {single[k]["solves"] for k in names} >= {4, 5, 7, 9, 11}
    n = cc.GEN_N
    Ap, Ai = cc.generic_pattern()
    AX = np.stack([single[k]["g"]["Ax"] for k in names])
    with gpu.Factorization(n, n, Ap, Ai, kind=_kind(gpu, spd), batch=nb) as F:
        _factor(F, AX, spd)
        cond, inv = _both_forms(F, AX)
        members = range(nb) if nb <= 66 else sorted({0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 191, 192, nb - 1})
        for b in members:
            r = single[names[b]]
            est, solves, tr = _port(F, n, b)
            assert cc.planned(tr, solves) == r["cls"] + ([],), (b, names[b])
            assert tr["margin"] >= cc.MARGIN
            assert abs(inv[b] - est) <= cc.bound(n, est), (b, names[b], inv[b], est)
    for b in range(nb):
        r = single[names[b]]
        assert inv[b] == r["inv"] and cond[b] == r["cond"], (b, names[b], inv[b], r["inv"])


# 4. the non-finite exit
def _export(F):
    import torch
    buf = torch.empty(F.batch * (F.info.factor_bytes // 8), dtype=torch.float64, device=torch.device("cuda", 0))
    F.export_factor_dev(buf.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(F.batch, -1)


def _import(G, host):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(host).reshape(-1).copy()).to(torch.device("cuda", 0))
    G.import_factor_dev(d.data_ptr())
    torch.cuda.synchronize()
    return d


def _diag_from_factors(F, b=0):
    Lp, Li, Lx, Up, Ui, Ux = F.factors(b)
    return Lx[Lp[:-1]] if Ux is None else Ux[Up[1:] - 1]


def _unique_pivot(F, host, b=0):
    """The place in member b's exported panels of a pivot whose value occurs there once."""
    for u in _diag_from_factors(F, b):
        where = np.flatnonzero(host[b] == u)
        if len(where) == 1:
            return int(where[0])
    raise AssertionError("no pivot with a value of its own")


@pytest.mark.parametrize("bad", [0.0, np.nan])
@pytest.mark.parametrize("nb", [1, 3])
def test_a_zero_or_nan_pivot_ends_at_infinity(gpu, nb, bad):
    names = ["5", "7", "9"][:nb]
    single = [_generic_single(gpu, k) for k in names]
    n = cc.GEN_N
    Ap, Ai = cc.generic_pattern()
    AX = np.stack([r["g"]["Ax"] for r in single])
    victim = nb // 2
    with gpu.Factorization(n, n, Ap, Ai, batch=nb) as F:
        F.factor(AX, cc.TOL)
        cond0, inv0 = F.condest(AX)
        host = _export(F)
        host[victim, _unique_pivot(F, host, victim)] = bad
    with gpu.Factorization(n, n, Ap, Ai, batch=nb) as G:
        keep = _import(G, host)
        cond, inv = _both_forms(G, AX)
        est, solves, tr = _port(G, n, victim)
    del keep
    assert est == np.inf and tr["nonfinite"]
    assert inv[victim] == np.inf and cond[victim] == np.inf
    for b in range(nb):
        if b != victim:
            assert inv[b] == inv0[b] == single[b]["inv"] and cond[b] == cond0[b]


# 5. k_slogdet: n around a wave and around the workgroup, pivots that only the second round reads
def _slogdet_want(F, b=0, chol=False):
    d = _diag_from_factors(F, b)
    return (1.0 if chol or (d < 0).sum() % 2 == 0 else -1.0), (2.0 if chol else 1.0) * np.log(np.abs(d)).sum()


def _assert_logabs(got, want):
    assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (got, want)


@pytest.mark.parametrize("n", cc.SLOGDET_N)
def test_slogdet_sizes(gpu, n):
    Ap, Ai, Ax, dpos = cc.slogdet_matrix(n)
    pure = cc.pure_diagonal(n)
    with gpu.Factorization(n, n, Ap, Ai) as F:
        q = F.ordering()["q"]
        F.factor(Ax, cc.TOL)
        sign, logabs = F.slogdet()
        want_sign, want = _slogdet_want(F)
        assert sign[0] == want_sign == 1.0
        _assert_logabs(logabs[0], want)
        last = int(np.flatnonzero(pure[q])[-1])
        places = [[last]]                                        # the last pivot that is an entry of A itself
        if n > cc.SLOGDET_NT:                                    # one in the second round; two across its edge; two apart
            assert pure[q[cc.SLOGDET_NT - 1]] and pure[q[cc.SLOGDET_NT]] and last >= cc.SLOGDET_NT
            places = [[cc.SLOGDET_NT], [cc.SLOGDET_NT - 1, cc.SLOGDET_NT], [cc.SLOGDET_NT - 1, last], [last]]
        for place in places:                                    # negative pivots at these places of the pivot order
            Ax2 = Ax.copy()
            Ax2[dpos[q[place]]] *= -1.0
            F.factor(Ax2, cc.TOL)
            sign2, logabs2 = F.slogdet()
            d = _diag_from_factors(F)
            assert np.array_equal(np.flatnonzero(d < 0), np.sort(place))
            assert sign2[0] == (-1.0 if len(place) % 2 else 1.0), place
            _assert_logabs(logabs2[0], want)
        if n > cc.SLOGDET_NT:                                   # a zero pivot that only the second round reads
            Ax3 = Ax.copy()
            Ax3[dpos[q[cc.SLOGDET_NT]]] = 7.25
            F.factor(Ax3, cc.TOL)
            assert _diag_from_factors(F)[cc.SLOGDET_NT] == 7.25
            host = _export(F)
            where = np.flatnonzero(host[0] == 7.25)
            assert len(where) == 1
            host[0, where[0]] = 0.0
            with gpu.Factorization(n, n, Ap, Ai) as G:
                keep = _import(G, host)
                sign3, logabs3 = G.slogdet()
            del keep
            assert sign3[0] == 0.0 and logabs3[0] == -np.inf


def test_slogdet_cholesky_past_the_workgroup(gpu):
    n = cc.SLOGDET_NT + 1
    Ap, Ai, Ax, dpos = cc.slogdet_matrix(n, spd=True)
    with gpu.Factorization(n, n, Ap, Ai, kind=gpu.CS3_CHOLESKY) as F:
        q = F.ordering()["q"]
        assert cc.pure_diagonal(n)[q[cc.SLOGDET_NT]]
        Ax[dpos[q[cc.SLOGDET_NT]]] = 1e-3                        # the only pivot of the second round: -6.9 of the sum
        F.factor(Ax)
        sign, logabs = F.slogdet()
        want_sign, want = _slogdet_want(F, chol=True)
        d = _diag_from_factors(F)
    assert abs(d[cc.SLOGDET_NT] - np.sqrt(1e-3)) <= 1e-15
    assert sign[0] == 1.0
    _assert_logabs(logabs[0], want)


def test_slogdet_negative_pivot_in_member_64_only(gpu):
    n, nb = 65, 65
    Ap, Ai, Ax, dpos = cc.slogdet_matrix(n)
    AX = np.tile(Ax, (nb, 1))
    j = int(np.flatnonzero(cc.pure_diagonal(n))[-1])
    AX[64, dpos[j]] *= -1.0
    with gpu.Factorization(n, n, Ap, Ai, batch=nb) as F:
        F.factor(AX, cc.TOL)
        sign, logabs = F.slogdet()
        for b in (0, 63, 64):
            want_sign, want = _slogdet_want(F, b)
            assert sign[b] == want_sign
            _assert_logabs(logabs[b], want)
    assert np.array_equal(sign, np.where(np.arange(nb) == 64, -1.0, 1.0))
    assert np.all(logabs == logabs[0]) or np.abs(logabs - logabs[0]).max() <= 1e-13 * max(1.0, abs(logabs[0]))
