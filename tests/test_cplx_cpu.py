"""Complex plans without a GPU: the argument checks in their order, the real pattern and the doubled order against the
NumPy restatement (tests/cplx_ref.py), the restatement against dense complex solves (so that what the GPU tests compare
with bit for bit is itself right), and what the analysis of the real form is expected to keep: pairs adjacent in the
pivot order, no supernode boundary inside a pair, nnz(L) within 4 x the complex count + n.

Not covered: the size limit (4 nnz >= 2^31 - 1024).  It comes after the row-index check in the stated order, so reaching
it takes a valid index array of 2 GiB."""
import ctypes as C

import numpy as np
import pytest

import cplx_cases as cases
import cplx_ref as ref
from csparse3_amd import synth

STRUCT = cases.structural_cases()


def create_rc(hip, n, Ap, Ai, batch=1, rotate=1, out=True):
    """(return code, message) of cs3_cplx_plan_create; a plan that was made is freed."""
    p = C.c_void_p()
    L = hip.lib()
    rc = L.cs3_cplx_plan_create(n, hip._pi(Ap), hip._pi(Ai), batch, rotate, C.byref(p) if out else None)
    msg = L.cs3_last_error().decode() if rc else ""
    if p:
        L.cs3_cplx_plan_free(p)
    return rc, msg


def test_argument_checks_come_in_the_stated_order(hip):
    good_p, good_i = np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    bad_p = np.array([1, 1, 2], dtype=np.int32)
    E = hip.CS3_ERR_ARG
    assert create_rc(hip, 2, good_p, good_i) == (0, "")
    # every call is wrong in everything that comes later in the order as well
    rc, msg = create_rc(hip, -1, bad_p, None, batch=0, rotate=7, out=False)
    assert rc == E and "null output" in msg
    rc, msg = create_rc(hip, -1, bad_p, None, batch=0, rotate=7)
    assert rc == E and "batch" in msg
    rc, msg = create_rc(hip, -1, bad_p, None, batch=1, rotate=7)
    assert rc == E and "rotate" in msg
    rc, msg = create_rc(hip, -1, bad_p, None, rotate=-1)
    assert rc == E and "rotate" in msg
    for n in (-1, 1 << 29):
        rc, msg = create_rc(hip, n, bad_p, None)
        assert rc == E and "order n" in msg
    rc, msg = create_rc(hip, 2, bad_p, None)
    assert rc == E and "Ap[0] != 0" in msg
    rc, msg = create_rc(hip, 2, np.array([0, 2, 1], dtype=np.int32), None)
    assert rc == E and "decreases at column 1" in msg
    rc, msg = create_rc(hip, 2, good_p, None)
    assert rc == E and "null row indices" in msg
    for bad_row in (-1, 2):
        rc, msg = create_rc(hip, 2, good_p, np.array([0, bad_row], dtype=np.int32))
        assert rc == E and "out of range at entry 1" in msg
    assert create_rc(hip, (1 << 29) - 1, None, None)[0] == E                 # (the largest n passes the range check: null Ap is next)
    assert "null column pointers" in create_rc(hip, (1 << 29) - 1, None, None)[1]


def test_the_python_classes_refuse_what_cannot_work(hip):
    n, Ap, Ai = STRUCT["n2"]
    with pytest.raises(AssertionError):
        hip.ComplexFactorization(n, Ap, Ai, kind=hip.CS3_CHOLESKY, rotate=True)
    with hip.ComplexPlan(n, Ap, Ai) as plan:
        with pytest.raises(hip.Cs3Error) as e:
            plan.order(q=[0, 0])
        assert e.value.code == hip.CS3_ERR_ARG
        with pytest.raises(AssertionError):
            hip.cplx_op("X")
    assert [hip.cplx_op(t) for t in ("N", "T", "H", "h", False, True, 2)] == [0, 1, 2, 2, 0, 1, 2]
    lim = hip.cplx_limits()
    assert lim.block == 256 and lim.grid_cap >= 1


@pytest.mark.parametrize("name", sorted(STRUCT))
def test_pattern_and_order_match_the_restatement(hip, name):
    n, Ap, Ai = STRUCT[name]
    Rp, Ri = ref.real_pattern(n, Ap, Ai)
    with hip.ComplexPlan(n, Ap, Ai, batch=2, rotate=False) as plan:
        gp, gi = plan.pattern()
        assert gp.dtype == np.int32 and np.array_equal(gp, Rp)
        assert gi.dtype == np.int32 and np.array_equal(gi, Ri)
        inf = plan.info
        nnz = int(Ap[n])
        assert (inf.n, inf.nnz, inf.batch, inf.rotate, inf.n_real, inf.nnz_real) == (n, nnz, 2, 0, 2 * n, 4 * nnz)
        col = ref.entry_columns(n, Ap)
        assert inf.rows_without_diagonal == n - len(np.unique(col[Ai[:nnz] == col]))
        q = hip.csc_amd_f(hip.ORDER_AMD, n, n, Ap, Ai) if n else np.zeros(0, dtype=np.int32)
        assert np.array_equal(plan.order(hip.ORDER_AMD), ref.doubled_order(q))
        assert np.array_equal(plan.order(hip.ORDER_NATURAL), np.arange(2 * n))
        rev = np.arange(n)[::-1]
        assert np.array_equal(plan.order(q=rev), ref.doubled_order(rev))
    # the pattern written out by hand, entry by entry
    want_rows = []
    for j in range(n):
        rows = [int(r) for r in Ai[Ap[j]:Ap[j + 1]]]
        for half in range(2):
            want_rows += [v for r in rows for v in (2 * r, 2 * r + 1)]
        assert Rp[2 * j + 1] - Rp[2 * j] == 2 * len(rows) == Rp[2 * j + 2] - Rp[2 * j + 1]
    assert want_rows == Ri.tolist()


def test_the_restated_values_are_the_two_by_two_blocks(hip):
    n, Ap, Ai = STRUCT["diag_twice"]
    Az = cases.values_for(np.random.default_rng(1), int(Ap[n]))
    Azr, Azi = ref.split(Az)
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate=False)
    M = ref.dense_real(n, Ap, Ai, ref.values(n, Ap, Ai, Azr, Azi, sr, si)[0])
    A = ref.dense_complex(n, Ap, Ai, Az[0])
    want = np.zeros((2 * n, 2 * n))
    want[0::2, 0::2], want[0::2, 1::2], want[1::2, 0::2], want[1::2, 1::2] = A.real, -A.imag, A.imag, A.real
    assert np.allclose(M, want, rtol=0, atol=1e-15)
    # a zero keeps its mirrored sign: -(+0) = -0 and -(-0) = +0
    one = ref.values(1, np.array([0, 1]), np.array([0]), np.array([[2.0]]), np.array([[0.0]]), np.ones((1, 1)), np.zeros((1, 1)))[0]
    assert np.array_equal(np.signbit(one), [False, False, True, False])


def _cases_for_the_dense_proof():
    yield "ybus40", synth.ybus(40, 60, seed=40)
    yield "ybus40_lossless", synth.ybus(40, 60, seed=40, lossless=True)
    n, Ap, Ai = STRUCT["diag_twice"]
    rng = np.random.default_rng(5)
    Az = cases.values_for(rng, int(Ap[n]))[0]
    Az[[0, 2, 3, 5]] += 4.0j                                                 # an imaginary diagonal that dominates
    yield "diag_twice", (n, Ap, Ai, Az)


@pytest.mark.parametrize("name,mat", list(_cases_for_the_dense_proof()), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("op", [ref.N, ref.T, ref.H])
def test_the_restatement_solves_what_the_dense_complex_solve_does(name, mat, rotate, op):
    n, Ap, Ai, Az = mat
    rng = np.random.default_rng(7)
    b = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    want = np.linalg.solve(ref.apply_op(op, ref.dense_complex(n, Ap, Ai, Az)), b)
    got = ref.solve_through_real_form(op, n, Ap, Ai, Az, b, rotate)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_rotation_makes_the_real_diagonal_positive_and_the_lossless_one_zero():
    n, Ap, Ai, Az = synth.ybus(40, 60, seed=40, lossless=True)
    assert not Az.real.any() and not np.signbit(Az.real).any()
    Azr, Azi = ref.split(Az, (1, -1))
    for rotate in (False, True):
        sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate)
        d = np.diag(ref.dense_real(n, Ap, Ai, ref.values(n, Ap, Ai, Azr, Azi, sr, si)[0]))
        assert np.all(d > 0.5) if rotate else not d.any()
    assert np.all((np.hypot(sr, si) >= 1.0) & (np.hypot(sr, si) <= np.sqrt(2.0) * (1 + 1e-15)))


def test_the_real_form_of_a_hermitian_positive_definite_matrix_is_spd():
    n, Ap, Ai, Az = cases.hermitian_pd(40, 60, seed=3)
    A = ref.dense_complex(n, Ap, Ai, Az)
    assert np.array_equal(A, A.conj().T) and np.linalg.eigvalsh(A).min() > 0
    Azr, Azi = ref.split(Az, (1, -1))
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate=False)
    M = ref.dense_real(n, Ap, Ai, ref.values(n, Ap, Ai, Azr, Azi, sr, si)[0])
    assert np.array_equal(M, M.T)
    assert np.linalg.eigvalsh(M).min() > 0


# (an entry stored twice is the plan's business only: cs3_analyze refuses duplicates)
@pytest.mark.parametrize("name", ["n1", "n2", "unsorted", "absent_diagonal", "empty_column", "ybus40", "ybus300"])
@pytest.mark.parametrize("order", ["amd", "natural"])
def test_the_analysis_keeps_pairs_together(hip, name, order):
    n, Ap, Ai = STRUCT[name] if name in STRUCT else synth.ybus(300, 480, seed=300)[:3]
    code = hip.ORDER_AMD if order == "amd" else hip.ORDER_NATURAL
    with hip.ComplexPlan(n, Ap, Ai) as plan:
        Rp, Ri = plan.pattern()
        q2 = plan.order(code)
    with hip.Factorization(2 * n, 2 * n, Rp, Ri, q=q2) as F, hip.Factorization(n, n, Ap, Ai, order=code) as Fc:
        assert F.info.n == 2 * n
        q = F.ordering()["q"]
        assert np.all(q[0::2] % 2 == 0) and np.array_equal(q[1::2], q[0::2] + 1), "a pair was separated by the postorder"
        assert np.array_equal(q[0::2] // 2, Fc.ordering()["q"]), "the pairs do not follow the complex pivot order"
        sn_ptr = F.supernodes()[0]
        assert np.all(sn_ptr % 2 == 0), "a supernode boundary falls inside a pair"
        assert F.info.nnz_l <= 4 * Fc.info.nnz_l + n


def test_ybus_is_what_it_says():
    n, Ap, Ai, Az = synth.ybus(40, 60, seed=40)
    assert Az.dtype == np.complex128 and Ap.dtype == np.int32 and Ai.dtype == np.int32 and Ap[n] == n + 2 * 60
    A = ref.dense_complex(n, Ap, Ai, Az)
    assert np.array_equal(A, A.T) and not np.array_equal(A, A.conj().T)
    d = np.diag(A)
    assert np.all(np.abs(d.imag) > np.abs(d.real)), "the diagonal of an admittance matrix is mostly imaginary"
    for j in range(n):
        assert np.all(np.diff(Ai[Ap[j]:Ap[j + 1]]) > 0)
    assert 1e2 < np.linalg.cond(A) < 1e6
    again = synth.ybus(40, 60, seed=40)
    assert all(np.array_equal(x, y) for x, y in zip((Ap, Ai, Az), again[1:]))


def test_cscmat_dispatches_on_the_dtype_and_names_what_is_out_of_scope(hip):
    from csparse3_amd import csc
    n, Ap, Ai, Az = synth.ybus(40, 60, seed=40)
    A = csc.CscMat(n, n, indptr=Ap, indices=Ai, data=Az)
    D = A.todense()
    assert D.dtype == np.complex128 and np.array_equal(D, ref.dense_complex(n, Ap, Ai, Az))
    R = csc.CscMat(n, n, indptr=Ap, indices=Ai, data=Az.imag.copy())
    assert R.todense().dtype == np.float64
    b = np.ones(n, dtype=np.complex128)
    for call in (lambda: A.lu(match=True), lambda: A.lu(perturb=True), lambda: A.lu(schur=[0, 1]), lambda: A.chol(schur=[0]),
                 lambda: A.solve(b, refine="extra"), lambda: A.solve(b, refine="gmres"), lambda: A.solve(b, match=True),
                 lambda: A.solve(b, perturb=1e-8), lambda: csc.lusol(A, b, refine="extra"), lambda: csc.lusol(A, b, match=True),
                 lambda: A.schur_complement([0, 1]), lambda: A.condest(), lambda: A.slogdet(),
                 lambda: A.solve_modified(b, []), lambda: A.sensitivities(A)):
        with pytest.raises(NotImplementedError, match="complex matrices"):
            call()
