"""Bilinear forms on the selected inverse (cs3_quad_*) without a GPU: the plan against the restated term map and classes,
the refusals in the header's order, the restated sums against the dense reference (the reference stays inside the bound
the GPU test sets), the designed critical measurements of synth.se_case, and CscMat's refusal of complex data."""
import ctypes as C

import numpy as np
import pytest

import quad_cases as qc
import quad_ref as ref
import selinv_ref
from csparse3_amd import synth
from csparse3_amd.csc import CscMat

FORM_CASES = sorted(qc.form_cases())


def _code(hip, rc):
    with pytest.raises(hip.Cs3Error) as e:
        hip._check(rc)
    return e.value.code, str(e.value)


def _plan_rc(hip, F, Ct, Bt=None, m=None):
    """The status of cs3_quad_plan (and a plan that must not exist)."""
    u = C.c_void_p()
    i32 = lambda a: None if a is None else hip._i32(a)
    arrays = [i32(Ct[1]), i32(Ct[2])] + ([None, None] if Bt is None else [i32(Bt[1]), i32(Bt[2])])
    rc = hip.lib().cs3_quad_plan(None if F is None else F._h, Ct[0] if m is None else m, *[hip._pi(a) for a in arrays], C.byref(u))
    assert rc != 0 and not u
    return rc


def test_limits(hip):
    L = hip.quad_limits()
    assert 0 < L.lane_chunk <= L.lane_max_terms < 64 < L.wave_max_terms and L.lane_max_terms % L.lane_chunk == 0
    assert L.block == 256 and L.reduce_rows == L.block
    assert _code(hip, hip.lib().cs3_quad_limits(None))[0] == hip.CS3_ERR_ARG


@pytest.mark.parametrize("name", FORM_CASES)
def test_plan_equals_the_restated_map(hip, name):
    case = qc.form_cases()[name]
    with qc.analysed(case) as F:
        want = ref.restated_plan(hip, F, case["Ct"], case["Bt"], qc.LIMITS)
        assert len(want) == 3 and not isinstance(want[0], int), "the case pairs columns outside the pattern: %r" % (want,)
        with F.quad_plan(case["Ct"], case["Bt"]) as plan:
            row_class, term_ptr, term_pos = plan.debug_plan()
            info = plan.info
        assert np.array_equal(term_ptr, want[1]) and np.array_equal(row_class, want[0])
        assert np.array_equal(term_pos, want[2])
        assert 0 <= term_pos.min() and term_pos.max() < F.selinv_info().zpool_doubles
        assert info.m == case["Ct"][0] and info.nterms == term_ptr[-1] and info.same_operand == (case["Bt"] is None)
        assert [info.rows_lane, info.rows_wave, info.rows_workgroup] == [int((row_class == c).sum()) for c in range(3)]
        assert info.nnz_c == len(case["Ct"][2]) and info.nnz_b == len((case["Bt"] or case["Ct"])[2])


def test_every_class_is_met(hip):
    for name in ("two_operands", "one_operand") + tuple("classes_%d_%d" % s for s in qc.class_sizes()):
        case = qc.form_cases()[name]
        cls = ref.classes(qc.LIMITS, ref.term_counts(case["Ct"], case["Bt"]))
        assert set(cls.tolist()) == {0, 1, 2}, name
    counts = ref.term_counts(qc.two_operands()["Ct"], qc.two_operands()["Bt"])
    assert counts[:len(qc.edge_term_counts())].tolist() == qc.edge_term_counts()
    for n_lane, n_wave in qc.class_sizes():
        case = qc.class_rows(n_lane, n_wave)
        cls = ref.classes(qc.LIMITS, ref.term_counts(case["Ct"], None))
        assert [(cls == c).sum() for c in range(3)] == [n_lane, n_wave, 2]


def _off_pattern_pair(hip, F):
    """(i, j) in the caller's labels with Z(i, j) outside the pattern of L + U."""
    position = ref.position_function(hip, F)
    pinv = F.ordering()["pinv"]
    for i in range(F.n):
        for j in range(F.n):
            if position(int(pinv[i]), int(pinv[j])) is None:
                return i, j
    raise AssertionError("the factors are dense")


def test_refusals_in_their_order(hip):
    m, n, Ap, Ai, Ax = synth.jacobian_like()[:5]
    good = (2, np.array([0, 1, 2], dtype=np.int32), np.array([3, 5], dtype=np.int32))
    bad_index = (2, good[1], np.array([3, n], dtype=np.int32))
    not_monotone = (2, np.array([0, 2, 1], dtype=np.int32), good[2])
    huge = (1, np.array([0, 46341], dtype=np.int32), (np.arange(46341) % n).astype(np.int32))      # 46341^2 >= 2^31 - 1024
    assert 46341 ** 2 >= 2 ** 31 - 1024 > 46340 ** 2
    # 1. null arguments, m out of range
    assert _code(hip, _plan_rc(hip, None, good))[0] == hip.CS3_ERR_ARG
    with hip.Factorization(m, n, Ap, Ai, schur=[3, 7]) as S, hip.Factorization(m, n, Ap, Ai) as F:
        assert hip.lib().cs3_quad_plan(F._h, 2, hip._pi(good[1]), hip._pi(good[2]), None, None, None) == hip.CS3_ERR_ARG
        code, text = _code(hip, _plan_rc(hip, S, (2, None, good[2])))
        assert code == hip.CS3_ERR_ARG and "null" in text
        code, text = _code(hip, _plan_rc(hip, S, bad_index, m=0))
        assert code == hip.CS3_ERR_ARG and "m must be" in text
        # 2. the pointer arrays, before the indices
        code, text = _code(hip, _plan_rc(hip, S, (2, not_monotone[1], bad_index[2])))
        assert code == hip.CS3_ERR_ARG and "monotone" in text
        code, text = _code(hip, _plan_rc(hip, S, good, Bt=not_monotone))
        assert code == hip.CS3_ERR_ARG and "Btp" in text
        # 3. an index outside [0, n), of either operand, before the handle is looked at
        code, text = _code(hip, _plan_rc(hip, S, bad_index))
        assert code == hip.CS3_ERR_ARG and "index out of range" in text and "column 1" in text
        code, text = _code(hip, _plan_rc(hip, S, good, Bt=(2, good[1], np.array([-1, 2], dtype=np.int32))))
        assert code == hip.CS3_ERR_ARG and "index out of range" in text and "B'" in text
        # 4. the handles selected inversion refuses, before the terms are counted
        code, text = _code(hip, _plan_rc(hip, S, huge))
        assert code == hip.CS3_ERR_ARG and "Schur" in text
        for kw, word in (({"match_values": Ax}, "matched"), ({"batch": 128}, "interleaved")):
            with hip.Factorization(m, n, Ap, Ai, **kw) as R:
                code, text = _code(hip, _plan_rc(hip, R, good))
                assert code == hip.CS3_ERR_ARG and word in text
        # 5. the term count, before any pair is looked up
        i, j = _off_pattern_pair(hip, F)
        off = (3, np.array([0, 1, 1, 3], dtype=np.int32), np.array([2, i, j], dtype=np.int32))
        code, text = _code(hip, _plan_rc(hip, F, (2, np.array([0, 2, 46343], dtype=np.int32), np.concatenate([[i, j], huge[2]]).astype(np.int32))))
        assert code == hip.CS3_ERR_ARG and "2^31 - 1024" in text
        # 6. a pair outside the pattern: the row and the two columns
        code, text = _code(hip, _plan_rc(hip, F, off))
        assert code == hip.CS3_ERR_ARG and "row 2" in text and ("columns %d and %d" % (i, j) in text or "columns %d and %d" % (j, i) in text)
        assert isinstance(ref.restated_plan(hip, F, off, None, qc.LIMITS)[0], int)
        only_b = (3, np.array([0, 1, 1, 2], dtype=np.int32), np.array([2, j], dtype=np.int32))
        only_c = (3, np.array([0, 1, 1, 2], dtype=np.int32), np.array([2, i], dtype=np.int32))
        code, text = _code(hip, _plan_rc(hip, F, only_c, Bt=only_b))
        assert code == hip.CS3_ERR_ARG and "row 2" in text and "columns %d and %d" % (i, j) in text
        assert hip.debug_live_device_buffers() >= 0 and hip.lib().cs3_quad_free(None) == 0


def test_calls_check_arguments_before_state(hip):
    """No device is needed to be refused: null arguments, another handle's plan, then the state."""
    L = hip.lib()
    case = qc.single_row()
    x = np.ones(8)
    p = C.c_void_p(x.ctypes.data)
    with qc.analysed(case) as F, qc.analysed(case) as F2, F.quad_plan(case["Ct"]) as plan, \
            F.quad_plan(case["Ct"], case["Ct"]) as plan2:
        assert _code(hip, L.cs3_quad_dev(None, plan._u, p, p, p, None))[0] == hip.CS3_ERR_ARG
        for rc in (L.cs3_quad_dev(F._h, None, p, p, p, None), L.cs3_quad_dev(F._h, plan._u, None, None, p, None),
                   L.cs3_quad_dev(F._h, plan._u, p, None, None, None), L.cs3_quad_dev(F._h, plan2._u, p, None, p, None),
                   L.cs3_quad(F._h, plan._u, hip._pf(x), None, None),
                   L.cs3_quad_normres_dev(F._h, plan._u, p, p, p, 0.0, None, None, None, None, None),
                   L.cs3_quad_normres_dev(F._h, plan._u, p, None, p, 0.0, None, None, None, p, None),
                   L.cs3_quad_normres(F._h, plan._u, hip._pf(x), hip._pf(x), None, 0.0, None, None, None, hip._pf(x))):
            code, text = _code(hip, rc)
            assert code == hip.CS3_ERR_ARG and "null" in text
        code, text = _code(hip, L.cs3_quad_dev(F2._h, plan._u, p, None, p, None))
        assert code == hip.CS3_ERR_ARG and "another handle" in text
        for rc in (L.cs3_quad_dev(F._h, plan._u, p, None, p, None), L.cs3_quad(F._h, plan._u, hip._pf(x), None, hip._pf(x)),
                   L.cs3_quad_normres_dev(F._h, plan._u, p, p, p, 0.0, None, None, None, p, None),
                   L.cs3_quad_normres_dev(F._h, plan2._u, p, p, p, 0.0, None, None, None, p, None)):
            code, text = _code(hip, rc)
            assert code == hip.CS3_ERR_STATE and "factorisation" in text
        assert plan.info.same_operand == 1 and plan2.info.same_operand == 0
    # a plan whose handle went first can only be freed
    F = qc.analysed(case)
    plan = F.quad_plan(case["Ct"])
    F.close()
    assert _code(hip, L.cs3_quad_dev(F2._h, plan._u, p, None, p, None))[0] == hip.CS3_ERR_ARG
    plan.close()


@pytest.mark.parametrize("name", FORM_CASES)
def test_restated_sums_stay_inside_the_bound(hip, name):
    """The three summation orders on the dense inverse's own entries against the plain sums."""
    case = qc.form_cases()[name]
    mat = case["matrix"]
    Zref, cond = selinv_ref.dense_inverse(mat[1], mat[2], mat[3], mat[4])
    assert cond <= ref.COND_MAX, (name, cond)
    t_ref, scale = ref.dense_forms(Zref, case["Ct"], case["Bt"], case["Cx"], case["Bx"])
    cls = ref.classes(qc.LIMITS, ref.term_counts(case["Ct"], case["Bt"]))
    t = ref.restated_forms(case["Ct"], case["Bt"], case["Cx"], case["Bx"], ref.z_at_terms(Zref, case["Ct"], case["Bt"]), cls)
    assert (np.abs(t - t_ref) <= ref.BOUND * scale).all(), name
    assert (np.abs(t - t_ref) <= 4096 * 2.0 ** -52 * scale).all(), name          # (a sum of at most 2304 terms, reordered)
    assert (t[ref.term_counts(case["Ct"], case["Bt"]) == 0] == 0.0).all()


def test_incidence_form_is_the_thevenin_sum(hip):
    case = qc.incidence("tridiagonal")
    mat = case["matrix"]
    Z, _ = selinv_ref.dense_inverse(mat[1], mat[2], mat[3], mat[4])
    t_ref, _ = ref.dense_forms(Z, case["Ct"], None, case["Cx"], None)
    i, j = case["Ct"][2][0::2], case["Ct"][2][1::2]
    assert np.allclose(t_ref, Z[i, i] + Z[j, j] - Z[i, j] - Z[j, i], rtol=1e-12, atol=0)


@pytest.mark.parametrize("size", sorted(qc.SE_SEEDS))
def test_se_case_has_its_designed_critical_rows(hip, size):
    """From the dense inverse: 1 - w t of the designed critical rows is below the crit_tol the GPU test passes, that of
    every other row above 100 times it."""
    case = qc.se(*size)
    H, w, crit = case["H"], case["w"], case["critical_rows"]
    m, n = H.shape
    assert m == size[1] + size[0] - len(crit) and n == size[0] and len(crit) >= 1
    nnz_row = (H != 0).sum(axis=1)
    assert (nnz_row[:size[1]] == 2).all() and set(nnz_row[size[1]:].tolist()) >= {1, 3} and nnz_row.min() == 1
    assert w.max() / w.min() > 50 and w.max() / w.min() <= 100
    for row in crit:                                       # a pendant bus seen by that row only
        pendant = [c for c in np.flatnonzero(H[row]) if (H[:, c] != 0).sum() == 1]
        assert len(pendant) == 1
    mat = case["matrix"]
    Z, cond = selinv_ref.dense_inverse(mat[1], mat[2], mat[3], mat[4])
    assert cond <= ref.COND_MAX
    s = 1.0 - w * np.einsum("ij,jk,ik->i", H, Z, H)
    others = np.setdiff1d(np.arange(m), crit)
    assert (s[crit] < qc.CRIT_TOL).all() and (s[others] > 100 * qc.CRIT_TOL).all(), (s[crit], s[others].min())


def test_restated_normres_orders_ties_and_nans():
    L = qc.LIMITS
    t, w = np.array([0.5, 0.5, 1.0, 0.5]), np.ones(4)
    _, rn, s = ref.restated_normres(t, w, np.array([1.0, -2.0, 5.0, 2.0]), 1e-8, L)
    assert rn[2] == 0.0 and s.tolist() == [rn[1], 1.0, 34.0, 1.0]              # row 2 is critical; rows 1 and 3 tie
    _, rn, s = ref.restated_normres(t, w, np.array([1.0, 9.0, 5.0, np.nan]), 1e-8, L)
    assert np.isnan(s[0]) and s[1] == 3.0 and np.isnan(s[2])
    rng = np.random.default_rng(3)
    x = rng.standard_normal(70000)
    J = ref._group_sums(x, 256)
    assert abs(J - np.sum(x)) <= 70000 * 2.0 ** -52 * np.abs(x).sum() and J != np.cumsum(x)[-1]


def test_cscmat_refuses_complex_data():
    n, Ap, Ai, Az = synth.ybus(12, 16, 3)
    A = CscMat(n, n, indptr=Ap, indices=Ai, data=Az)
    for call in (lambda: A.quad_forms(A), lambda: A.normalized_residuals(A, np.ones(n), np.ones(n))):
        with pytest.raises(NotImplementedError):
            call()
