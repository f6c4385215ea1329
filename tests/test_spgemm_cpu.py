"""Sparse products without a GPU: the Python restatement (tests/spgemm_ref.py) against the reference's recorded outputs,
the generators of the engineered cases, the argument checks of cs3_spgemm_plan_create (they run before the device check;
where the outcome depends on a device being visible, both outcomes are asserted) and the operands of CscMat.__mul__ that
must behave as before."""
import ctypes as C

import numpy as np
import pytest

import spgemm_cases as cases
import spgemm_ref as ref
from csparse3_amd import csc as csc_mod


@pytest.mark.parametrize("tag", cases.GOLD_CASES)
def test_restatement_matches_the_reference_bit_for_bit(tag):
    args, ta, (Cp, Ci, Cx) = cases.golden(tag)
    assert args[0] <= args[6] or ta                      # Am <= Bn: all the reference can do
    got = (ref.multiply_t if ta else ref.multiply)(*args)
    assert got[0] == (args[1] if ta else args[0]) and got[1] == args[6] and got[5] == int(Cp[-1])
    assert got[2].dtype == np.int32 and np.array_equal(got[2], Cp)
    assert got[3].dtype == np.int32 and np.array_equal(got[3], Ci)
    assert np.array_equal(ref.bits(got[4]), ref.bits(Cx))


def test_golden_file_holds_what_the_issue_lists():
    assert set(cases.GOLD_CASES) == {"r1", "r2", "r3", "r4", "r3s", "emp", "dup", "negzero", "t1", "tdup"}
    shape = lambda t: tuple(int(cases.GOLD[t + "_" + k]) for k in ("Am", "An", "Bm", "Bn"))     # noqa: E731
    assert [shape(t) for t in ("r1", "r2", "r3", "r4")] == [(40, 40, 40, 40), (25, 57, 57, 31), (31, 60, 60, 31), (64, 64, 64, 64)]
    for t in ("r1", "r2", "r3", "r4"):                    # every random case has unsorted columns in C
        Cp, Ci = cases.GOLD[t + "_Cp"], cases.GOLD[t + "_Ci"]
        assert any(np.any(np.diff(Ci[Cp[j]:Cp[j + 1]]) < 0) for j in range(len(Cp) - 1)), t
    assert np.array_equal(cases.GOLD["dup_Cp"], [0, 4, 4, 7, 7]) and np.array_equal(cases.GOLD["dup_Ci"], [3, 0, 2, 1, 1, 2, 0])
    assert cases.GOLD["negzero_Cx"].tobytes() == np.array([-0.0]).tobytes()
    assert np.any(np.diff(cases.GOLD["emp_Bp"]) == 0)     # B with empty columns ...
    Ap, Bi = cases.GOLD["emp_Ap"], cases.GOLD["emp_Bi"]
    assert np.any(Ap[Bi + 1] == Ap[Bi])                   # ... and B selecting empty columns of A
    assert int(cases.GOLD["t1_ta"]) == 1 and int(cases.GOLD["tdup_ta"]) == 1


def test_engineered_generators_hit_their_counts(hip):
    lim = hip.spgemm_limits()
    assert lim.slice_width == 64 and lim.lds_table_rows >= lim.lds_products > 64 and lim.long_list >= 2
    rng = np.random.default_rng(5)
    Am = 4 * int(lim.lds_table_rows) + 7
    for per_col in (1, 3, 7):
        specs = cases.symbolic_edge_specs(lim) + cases.chunk_edge_specs()
        args, built = cases.engineered_columns(rng, specs, per_col, Am)
        Cm, Cn, Cp, Ci, Cx, nz = ref.multiply(*args)
        assert [int(d) for d in np.diff(Cp)] == [D for _, D in built]
        Ap, Bp, Bi = args[2], args[7], args[8]
        prods = [int(sum(Ap[k + 1] - Ap[k] for k in Bi[Bp[j]:Bp[j + 1]])) for j in range(Cn)]
        assert prods == [T for T, _ in built]
        assert max(prods) > lim.lds_products >= min(prods)
    L = int(lim.long_list)
    for length in (L - 1, L, L + 1):
        Cm, Cn, Cp, Ci, Cx, nz = ref.multiply(*cases.one_long_list(rng, length))
        assert nz == 64
    args = cases.dot_product(rng, 193)
    total = None
    for k in range(193):
        v = float(args[9][k]) * float(args[4][k])
        total = v if total is None else total + v
    assert ref.multiply(*args)[4].tolist() == [total]


def _create(hip, Am, An, Ap, Ai, Bm, Bn, Bp, Bi, ta=0, out=True):
    plan = C.c_void_p()
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    Ap, Ai, Bp, Bi = i32(Ap), i32(Ai), i32(Bp), i32(Bi)
    rc = hip.lib().cs3_spgemm_plan_create(Am, An, hip._pi(Ap), hip._pi(Ai), Bm, Bn, hip._pi(Bp), hip._pi(Bi), ta,
                                          C.byref(plan) if out else None)
    msg = hip.lib().cs3_last_error().decode()
    if rc == 0:
        hip.lib().cs3_spgemm_plan_free(plan)
    return rc, msg


GOOD_A = (3, 2, [0, 2, 3], [0, 2, 1])                     # 3 x 2
GOOD_B = (2, 2, [0, 1, 3], [1, 0, 1])                     # 2 x 2


def test_argument_errors_come_before_the_device_check(hip):
    bad = {
        "inner dimensions": ((3, 2, [0, 2, 3], [0, 2, 1]), (3, 2, [0, 1, 3], [1, 0, 1]), 0),
        "inner dimensions, transposed": (GOOD_A, GOOD_B, 1),
        "index of A too large": ((3, 2, [0, 2, 3], [0, 3, 1]), GOOD_B, 0),
        "index of A negative": ((3, 2, [0, 2, 3], [0, -1, 1]), GOOD_B, 0),
        "index of B too large": (GOOD_A, (2, 2, [0, 1, 3], [1, 0, 2]), 0),
        "index of B negative": (GOOD_A, (2, 2, [0, 1, 3], [-1, 0, 1]), 0),
        "indptr of A decreases": ((3, 2, [0, 2, 1], [0, 2, 1]), GOOD_B, 0),
        "indptr of B decreases": (GOOD_A, (2, 2, [0, 3, 2], [1, 0, 1]), 0),
        "indptr of B does not start at 0": (GOOD_A, (2, 2, [1, 1, 3], [1, 0, 1]), 0),
        "null indices of A": ((3, 2, [0, 2, 3], None), GOOD_B, 0),
        "null indices of B": (GOOD_A, (2, 2, [0, 1, 3], None), 0),
        "null indptr of A": ((3, 2, None, [0, 2, 1]), GOOD_B, 0),
        "negative dimension": ((-1, 2, [0, 2, 3], [0, 2, 1]), GOOD_B, 0),
        "dimension above INT_MAX": ((2 ** 31, 2, [0, 2, 3], [0, 2, 1]), GOOD_B, 0),
    }
    for what, (A, B, ta) in bad.items():
        rc, msg = _create(hip, *A, *B, ta)
        assert rc == hip.CS3_ERR_ARG, what
        assert msg.startswith("cs3_spgemm_plan_create: "), what
    rc, msg = _create(hip, *GOOD_A, *GOOD_B, out=False)
    assert rc == hip.CS3_ERR_ARG
    # a valid call runs on the GPU or says there is none
    rc, msg = _create(hip, *GOOD_A, *GOOD_B)
    if hip.device_count() < 1:
        assert rc == hip.CS3_ERR_HIP and "no HIP device" in msg
    else:
        assert rc == 0
    # the same through the Python class
    with pytest.raises(hip.Cs3Error) as e:
        hip.SpgemmPlan(3, 2, [0, 2, 3], [0, 3, 1], *GOOD_B)
    assert e.value.code == hip.CS3_ERR_ARG
    with pytest.raises(AssertionError):                           # the reference asserts An == Bm (csc_numba.py:240)
        hip.csc_multiply_ff(3, 2, [0, 2, 3], [0, 2, 1], np.ones(3), 3, 2, [0, 1, 3], [1, 0, 1], np.ones(3))


def test_a_product_of_two_to_the_31_multiplications_is_refused(hip):
    """46341 entries in the one column of A (duplicates of row 0), selected by each of B's 46341 columns: 46341^2 products."""
    k = 46341
    assert k * k >= 2 ** 31 - 1024 > (k - 1) * (k - 1)
    Ap, Ai = [0, k], np.zeros(k, dtype=np.int32)
    Bp, Bi = np.arange(k + 1, dtype=np.int32), np.zeros(k, dtype=np.int32)
    rc, msg = _create(hip, 1, 1, Ap, Ai, 1, k, Bp, Bi)
    assert rc == hip.CS3_ERR_ARG and "2^31 - 1024" in msg


def test_plan_calls_refuse_null_plans(hip):
    lib = hip.lib()
    info = hip.SpgemmInfo()
    assert lib.cs3_spgemm_plan_info(None, C.byref(info)) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_plan_pattern(None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_plan_pattern_dev(None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_values_dev(None, None, None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_values(None, None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_limits(None) == hip.CS3_ERR_ARG
    assert lib.cs3_spgemm_plan_free(None) == 0


def test_scalar_and_array_operands_of_mul_are_unchanged(hip):
    Ap = np.array([0, 2, 3], dtype=np.int32)
    Ai = np.array([0, 2, 1], dtype=np.int32)
    Ax = np.array([1.5, -2.0, 4.0])
    A = csc_mod.CscMat(3, 2, indptr=Ap, indices=Ai, data=Ax)
    B = A * 2.0
    assert isinstance(B, csc_mod.CscMat) and B.shape == (3, 2)
    assert np.array_equal(B.data, 2.0 * Ax) and np.array_equal(A.data, Ax)
    assert np.array_equal(B.indptr, Ap) and np.array_equal(B.indices, Ai)
    assert np.array_equal((A * 3).data, 3 * Ax) and np.array_equal((-A).data, -Ax)
    with pytest.raises(Exception, match="Type not supported"):
        A * "x"
    x = np.array([1.0, 2.0])
    if hip.device_count() < 1:
        with pytest.raises(hip.Cs3Error) as e:
            A * x
        assert e.value.code == hip.CS3_ERR_HIP
        with pytest.raises(hip.Cs3Error) as e:
            A * csc_mod.CscMat(2, 2, indptr=np.array([0, 1, 3], dtype=np.int32), indices=np.array([1, 0, 1], dtype=np.int32),
                               data=np.ones(3))
        assert e.value.code == hip.CS3_ERR_HIP
    else:
        assert np.array_equal(A * x, [1.5, 8.0, -2.0])
    assert callable(csc_mod.CscMat.dot) and callable(csc_mod.CscMat.multiply_plan)
