"""Selected inversion (cs3_selinv_*) on the GPU against the dense inverse (tests/selinv_ref.py):
max |Z - Z_ref| <= 1e-10 max |Z_ref| over the extracted positions, on matrices with cond_1 <= 1e4 (asserted per test).
Small structures, the synthetic matrices, a dense root block at every order where the kernel changes, big fronts below the
root, batches, the getters, the sensitivities route, state and memory."""
import numpy as np
import pytest

import selinv_cases as sc
import selinv_ref as ref
import sweep_cases
from csparse3_amd import synth

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(name, case):
    """(Z_ref, cond) of a case, computed once."""
    if name not in _REF:
        _REF[name] = ref.dense_inverse(case[1], case[2], case[3], case[4])
        _REF[name][0].setflags(write=False)
    return _REF[name]


def _check_handle(hip, F, name, case, Zref, what=""):
    """Entries, transposed entries, the diagonal and the entries on the factors of a factorised handle against Z_ref."""
    n, Ap, Ai = case[1], case[2], case[3]
    for trans in (False, True):
        err = ref.max_error(F.inverse_entries(trans=trans), ref.entries_of(Zref, n, Ap, Ai, trans))
        print("%s%s entries trans=%d: %.3e" % (name, what, trans, err))
        assert err <= ref.BOUND, (name, what, trans, err)
    err = ref.max_error(F.inverse_diagonal(), Zref.diagonal())
    print("%s%s diagonal: %.3e" % (name, what, err))
    assert err <= ref.BOUND, (name, what, err)
    q = F.ordering()["q"]
    Zp = Zref[np.ix_(q, q)]
    Lp, Li, _, Up, Ui, _ = F.factors(values=False)
    Zl, Zu = F.inverse_on_factors()
    err = ref.max_error(Zl, ref.entries_of(Zp, n, Lp, Li))
    if Zu is not None:
        err = max(err, ref.max_error(Zu, ref.entries_of(Zp, n, Up, Ui)))
    else:
        assert Up is None
    print("%s%s on the factors: %.3e" % (name, what, err))
    assert err <= ref.BOUND, (name, what, err)


def _run(gpu, name, case, kind=None, tol=0.0):
    kind = gpu.CS3_LU if kind is None else kind
    Zref, cond = _reference(name, case)
    assert cond <= ref.COND_MAX, (name, cond)
    with sc.analysed(name, case, kind=kind) as F:
        F.factor(case[4], tol)
        _check_handle(gpu, F, name, case, Zref, " kind=%d tol=%g" % (kind, tol))
        return F.selinv_info()


# -- 1. small structures

@pytest.mark.parametrize("name", ["n1", "n2", "diagonal", "tridiagonal"])
def test_small_structures(gpu, name):
    case = {"n1": sc.tiny(1), "n2": sc.tiny(2), "diagonal": sc.diagonal(), "tridiagonal": sc.tridiagonal(40)}[name]
    _run(gpu, name, case)


# -- 2. synthetic matrices

def test_toy10(gpu):
    _run(gpu, "toy10", synth.toy10()[:5])


@pytest.mark.parametrize("tol", [1e-3, 0.0])
def test_jacobian_like(gpu, tol):
    _run(gpu, "jacobian_like", synth.jacobian_like()[:5], tol=tol)


def test_grid_jacobian_2000(gpu):
    """Amalgamated fronts with explicit zeros, forest fronts and level fronts."""
    info = _run(gpu, "grid2000", synth.grid_jacobian(n=2000, seed=3)[:5])
    assert info.nfronts_small > 100


def test_spd_grid_cholesky(gpu):
    _run(gpu, "spd_small", sc.spd_small(), gpu.CS3_CHOLESKY)


# -- 3. a dense root block at the orders where the kernel changes

@pytest.mark.parametrize("order", sc.dense_root_orders())
@pytest.mark.parametrize("kind", ["lu", "chol"])
def test_dense_root(gpu, order, kind):
    case = sc.dense_root(order)
    if kind == "chol":                                      # the same pattern with symmetric, diagonally dominant values
        A = ref.dense(case[1], case[2], case[3], case[4])
        S = 0.5 * (A + A.T)
        cols = np.repeat(np.arange(case[1]), np.diff(case[2]))
        case = case[:4] + (S[case[3], cols],)
    info = _run(gpu, "dense_root_%d_%s" % (order, kind), case, gpu.CS3_LU if kind == "lu" else gpu.CS3_CHOLESKY)
    assert (info.nfronts_big > 0) == (order > sc.LIMITS.lds_max_order)


# -- 4. big fronts below the root

@pytest.mark.parametrize("variant", ["lu", "chol", "lu_fringe"])
def test_big_fronts_below_the_root(gpu, variant):
    case = sc.w72(symmetric=variant == "chol", fringe=40 if variant == "lu_fringe" else 0)
    info = _run(gpu, "w72_" + variant, case, gpu.CS3_CHOLESKY if variant == "chol" else gpu.CS3_LU)
    orders = [r for r, w, parent in sc._front_orders(case[1], case[2], case[3])]
    assert info.nfronts_big == sum(r > sc.LIMITS.lds_max_order for r in orders) >= 3
    if variant == "lu_fringe":                              # small fronts under big ones
        assert info.nfronts_small > 0


# -- 5. batch

def test_batch_of_three_equals_each_alone(gpu):
    case = sc.w72(fringe=40)
    n, Ap, Ai = case[1], case[2], case[3]
    AX = sweep_cases.case_values("w72", 3, fringe=40)
    with sc.analysed("w72", case, batch=3) as F:
        F.factor(AX)
        Zx, d = F.inverse_entries(), F.inverse_diagonal()
        assert Zx.shape == (3, int(Ap[n])) and d.shape == (3, n)
        for b in range(3):
            Zref, cond = ref.dense_inverse(n, Ap, Ai, AX[b])
            assert cond <= ref.COND_MAX
            assert ref.max_error(Zx[b], ref.entries_of(Zref, n, Ap, Ai)) <= ref.BOUND, b
            assert ref.max_error(d[b], Zref.diagonal()) <= ref.BOUND, b
            with sc.analysed("w72", case) as F1:
                F1.factor(AX[b])
                assert np.array_equal(F1.inverse_entries(), Zx[b]), "matrix %d differs from the same matrix alone" % b
                assert np.array_equal(F1.inverse_diagonal(), d[b]), b


# -- 6. getters

def test_entries_of_a_one_sided_pattern(gpu):
    case = sc.one_sided()
    n, Ap, Ai = case[1], case[2], case[3]
    Zref, cond = _reference("one_sided", case)
    assert cond <= ref.COND_MAX and not np.allclose(Zref, Zref.T)
    with sc.analysed("one_sided", case) as F:
        F.factor(case[4])
        assert ref.max_error(F.inverse_entries(), Zref[Ai, np.repeat(np.arange(n), np.diff(Ap))]) <= ref.BOUND
        assert ref.max_error(F.inverse_entries(trans=True), Zref[np.repeat(np.arange(n), np.diff(Ap)), Ai]) <= ref.BOUND


def test_diagonal_without_a_stored_diagonal(gpu):
    case = sc.absent_diagonal()
    Zref, cond = _reference("absent_diagonal", case)
    assert cond <= ref.COND_MAX
    with sc.analysed("absent_diagonal", case) as F:
        F.factor(case[4])
        assert ref.max_error(F.inverse_diagonal(), Zref.diagonal()) <= ref.BOUND
        _check_handle(gpu, F, "absent_diagonal", case, Zref)


def test_unsorted_rows(gpu):
    _run(gpu, "unsorted_rows", sc.unsorted_rows())


def test_cscmat_methods(gpu):
    from csparse3_amd.csc import CscMat
    m, n, Ap, Ai, Ax = synth.jacobian_like()[:5]
    Zref, _ = _reference("jacobian_like", (m, n, Ap, Ai, Ax))
    A = CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    for trans in (False, True):
        Zs = A.selected_inverse(trans=trans)
        assert np.array_equal(Zs.indptr, Ap) and np.array_equal(Zs.indices[:Ap[n]], Ai[:Ap[n]])
        assert ref.max_error(Zs.data, ref.entries_of(Zref, n, Ap, Ai, trans)) <= ref.BOUND
    assert ref.max_error(A.inverse_diagonal(), Zref.diagonal()) <= ref.BOUND


# -- 7. the sensitivities route

def test_diagonal_equals_the_sensitivities_route(gpu):
    """diag(A^-1) from sens_solve with unit columns (B = I as a sparse operand, C = I), the route this replaces."""
    m, n, Ap, Ai, Ax = synth.jacobian_like()[:5]
    Zref, cond = _reference("jacobian_like", (m, n, Ap, Ai, Ax))
    assert cond <= ref.COND_MAX
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax)
        with F.sens_plan((n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)), None) as plan:
            Y = F.sens_solve(plan, np.ones(n), None)
        d = F.inverse_diagonal()
        assert ref.max_error(Y.diagonal(), Zref.diagonal()) <= ref.BOUND
        assert ref.max_error(d, Y.diagonal()) <= ref.BOUND


# -- 8. state

def _getter_dev(gpu, F, which, torch):
    """(status, result) of a device-pointer getter on the current stream."""
    out = torch.full((F.batch, F.n if which == "diag" else F.nnz), -7.0, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    L = gpu.lib()
    rc = L.cs3_selinv_diag_dev(F._h, out.data_ptr(), st) if which == "diag" else L.cs3_selinv_entries_dev(F._h, 0, out.data_ptr(), st)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[0]


def test_state(gpu):
    import torch
    m, n, Ap, Ai, Ax = synth.jacobian_like()[:5]
    Zref, _ = _reference("jacobian_like", (m, n, Ap, Ai, Ax))
    with gpu.Factorization(m, n, Ap, Ai) as F:
        F.factor(Ax)
        for which in ("diag", "entries"):                   # a getter before selinv()
            rc, _ = _getter_dev(gpu, F, which, torch)
            assert rc == gpu.CS3_ERR_STATE
        F.selinv(torch.cuda.current_stream().cuda_stream)
        rc, d0 = _getter_dev(gpu, F, "diag", torch)
        assert rc == 0 and ref.max_error(d0, Zref.diagonal()) <= ref.BOUND
        rc, e0 = _getter_dev(gpu, F, "entries", torch)
        assert rc == 0 and ref.max_error(e0, ref.entries_of(Zref, n, Ap, Ai)) <= ref.BOUND
        # a solve with fewer right-hand sides than any before and a condest leave Z alone
        F.solve(np.ones((n, 4)))
        F.solve(np.ones(n))
        F.condest(Ax)
        rc, d1 = _getter_dev(gpu, F, "diag", torch)
        assert rc == 0 and np.array_equal(d1, d0)
        F.selinv()                                          # two runs, the same bits
        rc, d2 = _getter_dev(gpu, F, "diag", torch)
        assert rc == 0 and np.array_equal(d2, d0)
        # new values: the old Z is refused, the new one follows them
        Ax2 = Ax * (1.0 + 0.25 * np.cos(np.arange(len(Ax))))
        Zref2, cond2 = ref.dense_inverse(n, Ap, Ai, Ax2)
        assert cond2 <= ref.COND_MAX
        F.factor(Ax2)
        rc, _ = _getter_dev(gpu, F, "diag", torch)
        assert rc == gpu.CS3_ERR_STATE
        d3 = F.inverse_diagonal()                           # (the host form computes)
        assert ref.max_error(d3, Zref2.diagonal()) <= ref.BOUND and not np.array_equal(d3, d0)
        rc, d4 = _getter_dev(gpu, F, "diag", torch)
        assert rc == 0 and np.array_equal(d4, d3)
        # the fused step invalidates as well
        x = torch.ones(n, dtype=torch.float64, device="cuda:0")
        F.factor_solve_dev(torch.from_numpy(Ax).to("cuda:0").data_ptr(), x.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rc, _ = _getter_dev(gpu, F, "diag", torch)
        assert rc == gpu.CS3_ERR_STATE
        assert np.array_equal(F.inverse_diagonal(), d0)


# -- 9. memory

def test_memory_goes_with_the_handle(gpu):
    live = gpu.debug_live_device_buffers()
    case = sc.w72(fringe=40)
    F = sc.analysed("w72", case)
    F.factor(case[4])
    F.inverse_diagonal()
    F.inverse_on_factors()
    assert gpu.debug_live_device_buffers() > live
    F.close()
    assert gpu.debug_live_device_buffers() == live
