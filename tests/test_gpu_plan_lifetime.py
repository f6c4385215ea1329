"""The four kinds of plans on held factors -- cs3_updates_plan, cs3_sens_plan, cs3_cplx_updates_plan, cs3_cplx_sens_plan
-- on ONE handle: the real form (order 24) of a complex matrix of order 12 (real plans are legal on any handle).  What
their common lifetime rules promise, counted in device blocks (cs3_debug_live_device_buffers) and in the handle's
allocation and synchronisation counters (cs3_debug_alloc_counters):
  - the second solve with every plan neither allocates nor synchronises, and returns the bits of the first;
  - plans may go before the handle or after it: freeing the handle takes the device blocks of the plans it still has with
    it, so that only the complex plan's own tables are left;
  - a plan that outlived its handle makes every solve entry point return CS3_ERR_ARG without touching the device, and can
    be freed."""
import ctypes as C
import gc

import numpy as np
import pytest

import csens_cases as cc

pytestmark = pytest.mark.gpu

N = 12
ALIGNED = 0x10000                                    # a device address that no check follows


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64).copy()


def test_four_kinds_of_plans_on_one_handle(gpu):
    hip = gpu
    L = hip.lib()
    n, Ap, Ai, Az = cc.banded(N, 7)                  # tridiagonal: every row has a stored diagonal
    r = np.random.default_rng(12)
    gc.collect()                                     # (handles that earlier tests dropped without closing go now, not below)
    live0 = hip.debug_live_device_buffers()
    F = hip.ComplexFactorization(n, Ap, Ai)
    G = hip.ComplexFactorization(n, Ap, Ai)          # a second handle of the same shape, never factorised: nothing on the device
    F.plan.upload()
    own = hip.debug_live_device_buffers() - live0    # the complex plan's own tables
    assert own > 0
    F.factor(Az)
    R = F.real
    assert R.n == 2 * n

    # one plan of each kind; the real ones index the order-24 real form
    upd = R.updates_plan([([0, 5], [0, 5]), ([3, 23], [7, 3]), ([], []), ([11], [12])])
    sens = R.sens_plan((3, [0, 1, 3, 4], [4, 0, 23, 9]), (2, [0, 2, 3], [1, 22, 7]))
    cupd = F.updates_plan([([0, 5], [0, 5]), ([3, 11], [7, 3]), ([], [])])
    csens = F.sens_plan((3, [0, 1, 3, 4], [4, 0, 11, 9]), (2, [0, 2, 3], [1, 10, 7]), trans="H")
    cx, b = r.standard_normal(5), r.standard_normal(2 * n)
    bx, ctx = r.standard_normal(4), r.standard_normal(3)
    cz, bz = r.standard_normal(4) + 1j * r.standard_normal(4), r.standard_normal(n) + 1j * r.standard_normal(n)
    bzx, ctz = r.standard_normal(4) + 1j * r.standard_normal(4), r.standard_normal(3) + 1j * r.standard_normal(3)

    def solve_all():
        X, rpiv = R.solve_updates(upd, cx, b)
        Y = R.sens_solve(sens, bx, ctx)
        Xz, rpz = F.solve_updates(cupd, cz, bz)
        Yz = F.sens_solve(csens, bzx, ctz)
        return [_bits(a) for a in (X, rpiv, Y, Xz, rpz, Yz)]

    first = solve_all()
    assert all(np.isfinite(a.view(np.float64)).all() for a in first)
    live1, counters1 = hip.debug_live_device_buffers(), R.debug_alloc_counters()
    assert live1 > live0 + own
    second = solve_all()
    assert hip.debug_live_device_buffers() == live1
    assert R.debug_alloc_counters() == counters1
    for a, b2 in zip(first, second):
        assert np.array_equal(a, b2)

    # one real and one complex plan go before the handle: each takes its own device blocks along
    upd.close()
    live2 = hip.debug_live_device_buffers()
    assert live2 < live1
    csens.close()
    live3 = hip.debug_live_device_buffers()
    assert live3 < live2
    # the handle takes its own blocks and those of the two plans it still has: the complex plan's tables are what is left
    R.close()
    assert hip.debug_live_device_buffers() == live0 + own

    # the survivors: every solve entry point refuses them, whatever live handle they are offered, and nothing is allocated
    p, g = F.plan._p, G.real._h
    dev = C.c_void_p(ALIGNED)
    Y, Xz, rp = np.empty((2, 3)), np.empty((n, 3), dtype=np.complex128), np.empty(3)
    calls = {
        "cs3_sens_solve": lambda: L.cs3_sens_solve(g, sens._u, hip._pf(bx), hip._pf(ctx), hip._pf(Y)),
        "cs3_sens_solve_dev": lambda: L.cs3_sens_solve_dev(g, sens._u, dev, dev, dev, None),
        "cs3_debug_sens_parts": lambda: L.cs3_debug_sens_parts(g, sens._u, 7, dev, dev, dev, None),
        "cs3_cplx_updates_solve": lambda: L.cs3_cplx_updates_solve(p, g, cupd._u, hip._pc(cz), hip._pc(bz), C.c_double(0.0), hip._pc(Xz),
                                                                   hip._pf(rp)),
        "cs3_cplx_updates_solve_dev": lambda: L.cs3_cplx_updates_solve_dev(p, g, cupd._u, dev, dev, C.c_double(0.0), dev, None, None),
        "cs3_debug_cplx_updates_parts": lambda: L.cs3_debug_cplx_updates_parts(p, g, cupd._u, 7, dev, dev, C.c_double(0.0), dev, None, None),
    }
    for name, call in calls.items():
        rc = call()
        msg = L.cs3_last_error().decode()
        assert rc == hip.CS3_ERR_ARG and msg == name + ": the plan was made for another handle", (name, rc, msg)
        assert hip.debug_live_device_buffers() == live0 + own, name
    assert sens.info.k == 3 and cupd.info.ncases == 3           # they can still be asked ...
    sens.close()                                                # ... and freed
    cupd.close()
    assert hip.debug_live_device_buffers() == live0 + own
    G.close()
    assert hip.debug_live_device_buffers() == live0 + own       # (G's plan was never uploaded)
    F.plan.close()
    assert hip.debug_live_device_buffers() == live0
