"""Selected inversion (cs3_selinv_*) without a GPU: the argument and state checks of the ABI in the header's order, limits
and info, the plan (order of the fronts, launches, extraction maps) against the restatement in tests/selinv_ref.py, the
restated recurrence against the dense inverse, and CscMat's refusal of complex data."""
import ctypes as C

import numpy as np
import pytest

import selinv_cases as sc
import selinv_ref as ref
from csparse3_amd import synth
from csparse3_amd.csc import CscMat

PLAN_CASES = sorted(sc.plan_cases())


def _code(hip, rc):
    with pytest.raises(hip.Cs3Error) as e:
        hip._check(rc)
    return e.value.code, str(e.value)


def _toy(hip, **kw):
    m, n, Ap, Ai, Ax = synth.toy10()[:5]
    return n, int(Ap[n]), Ax, hip.Factorization(m, n, Ap, Ai, **kw)


def _calls(hip, h, n, nnz):
    """Every entry point that takes a handle, with outputs that are not null (device pointers are never followed before the
    checks are through): name -> a function returning the status."""
    L = hip.lib()
    info = hip.SelinvInfo()
    zx, d = np.empty(max(nnz, 1)), np.empty(max(n, 1))
    somewhere = C.c_void_p(zx.ctypes.data)
    return {"cs3_selinv_dev": lambda: L.cs3_selinv_dev(h, None),
            "cs3_selinv_info": lambda: L.cs3_selinv_info(h, C.byref(info)),
            "cs3_selinv_entries_dev": lambda: L.cs3_selinv_entries_dev(h, 0, somewhere, None),
            "cs3_selinv_diag_dev": lambda: L.cs3_selinv_diag_dev(h, somewhere, None),
            "cs3_selinv_entries": lambda: L.cs3_selinv_entries(h, 0, hip._pf(zx)),
            "cs3_selinv_diag": lambda: L.cs3_selinv_diag(h, hip._pf(d)),
            "cs3_selinv_factors": lambda: L.cs3_selinv_factors(h, 0, hip._pf(zx), None)}


PLAN_ONLY = ("cs3_selinv_info",)                  # need no factorisation


def test_null_handle_and_null_outputs(hip):
    L = hip.lib()
    for name, call in _calls(hip, None, 10, 34).items():
        assert _code(hip, call())[0] == hip.CS3_ERR_ARG, name
    assert L.cs3_debug_selinv_plan(None, None, None, None, None) == -1
    assert _code(hip, L.cs3_selinv_limits(None))[0] == hip.CS3_ERR_ARG
    n, nnz, _, F = _toy(hip)
    with F:
        null_out = {"cs3_selinv_info": lambda: L.cs3_selinv_info(F._h, None),
                    "cs3_selinv_entries_dev": lambda: L.cs3_selinv_entries_dev(F._h, 0, None, None),
                    "cs3_selinv_diag_dev": lambda: L.cs3_selinv_diag_dev(F._h, None, None),
                    "cs3_selinv_entries": lambda: L.cs3_selinv_entries(F._h, 0, None),
                    "cs3_selinv_diag": lambda: L.cs3_selinv_diag(F._h, None),
                    "cs3_selinv_factors": lambda: L.cs3_selinv_factors(F._h, 0, None, None)}
        for name, call in null_out.items():
            code, text = _code(hip, call())
            assert code == hip.CS3_ERR_ARG and "null" in text, name             # (not CS3_ERR_STATE: nothing is factorised)


@pytest.mark.parametrize("why", ["schur", "matched", "interleaved"])
def test_refused_handles_name_the_reason(hip, why):
    """Before the state check: these handles are analysed only, and the answer is CS3_ERR_ARG with the reason."""
    m, n, Ap, Ai, Ax = synth.toy10()[:5]
    kw = {"schur": {"schur": [3, 7]}, "matched": {"match_values": Ax}, "interleaved": {"batch": 128}}[why]
    word = {"schur": "Schur", "matched": "matched", "interleaved": "interleaved"}[why]
    with hip.Factorization(m, n, Ap, Ai, **kw) as F:
        for name, call in _calls(hip, F._h, n, int(Ap[n])).items():
            code, text = _code(hip, call())
            assert code == hip.CS3_ERR_ARG and word in text, (name, text)
        assert hip.lib().cs3_debug_selinv_plan(F._h, None, None, None, None) == -1


def test_no_factorisation_is_a_state_error(hip):
    n, nnz, _, F = _toy(hip)
    with F:
        for name, call in _calls(hip, F._h, n, nnz).items():
            if name in PLAN_ONLY:
                assert call() == 0, name
            else:
                code, text = _code(hip, call())
                assert code == hip.CS3_ERR_STATE and "factorisation" in text, (name, text)
        with pytest.raises(hip.Cs3Error) as e:                                  # arguments come before the state
            hip._check(hip.lib().cs3_selinv_factors(F._h, 1, hip._pf(np.empty(nnz)), None))
        assert e.value.code == hip.CS3_ERR_ARG
    with _toy(hip, kind=hip.CS3_CHOLESKY)[3] as F:
        code, text = _code(hip, hip.lib().cs3_selinv_factors(F._h, 0, hip._pf(np.empty(nnz)), hip._pf(np.empty(nnz))))
        assert code == hip.CS3_ERR_ARG and "Cholesky" in text


def test_limits_and_info(hip):
    lim = hip.selinv_limits()
    assert 0 < lim.wave_max_order <= 64 and lim.wave_max_order < lim.lds_max_order
    assert (lim.lds_max_order | 1) * lim.lds_max_order * 8 <= 160 * 1024         # the image of the largest LDS front
    assert lim.gemm_tile == 16 and lim.diag_block % lim.gemm_tile == 0
    case = sc.w72()
    with sc.analysed("w72", case) as F:
        info = F.selinv_info()
        orders = np.array([r for r, w, parent in sc._front_orders(case[1], case[2], case[3])])
        assert info.zpool_doubles == int((orders.astype(np.int64) ** 2).sum())
        assert info.nfronts_big == int((orders > lim.lds_max_order).sum()) == 3
        assert info.nfronts_small + info.nfronts_big == len(orders)
        front, launch, _, _ = F.selinv_plan()
        assert info.nlaunches == int(launch.max()) + 3                           # the last group is big too: the index of its first launch, and three


@pytest.mark.parametrize("name", PLAN_CASES + ["w72_fringe", "grid"])
def test_plan_runs_parents_first_in_earlier_launches(hip, name):
    case = {"w72_fringe": sc.w72(fringe=40), "grid": synth.grid_jacobian(n=2000, seed=3)[:5]}.get(name) or sc.plan_cases()[name]
    with sc.analysed(name, case) as F:
        front, launch, _, _ = F.selinv_plan()
        _, parent, _ = F.supernodes()
        assert sorted(front) == list(range(len(parent)))
        at = np.empty(len(front), dtype=np.int64)
        at[front] = np.arange(len(front))
        assert (np.diff(launch) >= 0).all()
        for s, p in enumerate(parent):
            if p >= 0:
                assert at[p] < at[s] and launch[at[p]] < launch[at[s]], "front %d and its parent %d" % (s, p)


@pytest.mark.parametrize("name", PLAN_CASES)
def test_maps_equal_the_restated_positions(hip, name):
    case = sc.plan_cases()[name]
    n = case[1]
    with sc.analysed(name, case) as F:
        front, _, entry, diag = F.selinv_plan()
        want_entry, want_diag, total = ref.restated_positions(hip, F, case[2], case[3], front)
        assert total == F.selinv_info().zpool_doubles
        assert np.array_equal(entry, want_entry)
        assert np.array_equal(diag, want_diag)
        # the diagonal map is a bijection onto the diagonals of the pivot blocks
        sn_ptr, _, _, st = ref.fronts(hip, F)
        z_off = dict(zip(front.tolist(), np.concatenate([[0], np.cumsum([len(st[s]) ** 2 for s in front])])[:-1].tolist()))
        pivots = sorted(z_off[s] + k * (len(st[s]) + 1) for s in range(len(st)) for k in range(int(sn_ptr[s + 1] - sn_ptr[s])))
        assert sorted(diag.tolist()) == pivots and len(set(pivots)) == n


@pytest.mark.parametrize("name", PLAN_CASES)
def test_restated_recurrence_equals_the_dense_inverse(hip, name):
    case = sc.plan_cases()[name]
    n = case[1]
    Zref, cond = ref.dense_inverse(n, case[2], case[3], case[4])
    assert cond <= ref.COND_MAX
    with sc.analysed(name, case) as F:
        L, U = ref.host_factors(F, ref.dense(n, case[2], case[3], case[4]))
        Z = ref.restated_inverse(hip, F, L, U)
        q = F.ordering()["q"]
        on = np.isfinite(Z)
        assert ref.max_error(Z[on], Zref[np.ix_(q, q)][on]) <= ref.BOUND
        pinv = F.ordering()["pinv"]
        cols = np.repeat(np.arange(n), np.diff(case[2]))
        assert on[pinv[case[3]], pinv[cols]].all() and on[pinv[cols], pinv[case[3]]].all() and on.diagonal().all()


def test_cholesky_restatement(hip):
    case = sc.spd_small()
    n = case[1]
    Zref, cond = ref.dense_inverse(n, case[2], case[3], case[4])
    assert cond <= ref.COND_MAX
    with sc.analysed("spd", case, kind=hip.CS3_CHOLESKY) as F:
        L, U = ref.host_factors(F, ref.dense(n, case[2], case[3], case[4]), cholesky=True)
        Z = ref.restated_inverse(hip, F, L, U)
        q = F.ordering()["q"]
        on = np.isfinite(Z)
        assert ref.max_error(Z[on], Zref[np.ix_(q, q)][on]) <= ref.BOUND


def test_cscmat_refuses_complex_data():
    m, n, Ap, Ai, Ax = synth.toy10()[:5]
    A = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax.astype(np.complex128))
    with pytest.raises(NotImplementedError, match="selected_inverse"):
        A.selected_inverse()
    with pytest.raises(NotImplementedError, match="inverse_diagonal"):
        A.inverse_diagonal()
