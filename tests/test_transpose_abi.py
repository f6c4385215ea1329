"""Transposed solves: argument and state errors of the new entry points, and trans=False as the default everywhere.
Nothing here needs a GPU; where the outcome depends on one being visible, both outcomes are checked."""
import inspect

import numpy as np
import pytest

from csparse3_amd import csc as csc_mod
from csparse3_amd import synth


def _toy(hip, kind=None):
    m, n, Ap, Ai, Ax, b, xt = synth.toy10()
    if kind is None:
        kind = hip.CS3_LU
    return m, n, Ap, Ai, Ax, hip.Factorization(m, n, Ap, Ai, kind=kind)


def test_transposed_solves_before_a_factorisation_are_state_errors(hip):
    m, n, Ap, Ai, Ax, F = _toy(hip)
    with F:
        for call in (lambda: F.solve(np.ones(n), trans=True), lambda: F.utsolve(np.ones(n)),
                     lambda: F.ltsolve(np.ones(n)), lambda: F.solve_dev(0, 1, 0, trans=True),
                     lambda: F.utsolve_dev(0, 1), lambda: F.ltsolve_dev(0, 1)):
            with pytest.raises(hip.Cs3Error) as e:
                call()
            assert e.value.code == hip.CS3_ERR_STATE


def test_utsolve_on_a_cholesky_handle_is_an_argument_error(hip):
    n = 60
    ei, ej = synth.spd_grid_pattern(n, seed=1)
    m, n, Ap, Ai, Ax = synth.spd_grid_matrix(n, ei, ej, seed=2)
    with hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY) as F:
        for call in (lambda: F.utsolve(np.ones(n)), lambda: F.utsolve_dev(0, 1)):
            with pytest.raises(hip.Cs3Error) as e:
                call()
            assert e.value.code == hip.CS3_ERR_ARG


def test_transposed_products_check_their_arguments(hip):
    m, n, Ap, Ai, Ax, F = _toy(hip)
    with F:
        for call in (lambda: F.matvec_dev(0, 0, 0, 1, trans=True),
                     lambda: F.residual_dev(0, 0, 0, 0, 1, trans=True),
                     lambda: F.refine_dev(0, 0, 0, 1, 1, trans=True),
                     lambda: F.refine_dev(8, 8, 8, 0, 1, trans=True)):
            with pytest.raises(hip.Cs3Error) as e:
                call()
            assert e.value.code == hip.CS3_ERR_ARG
        with pytest.raises(hip.Cs3Error) as e:                    # a factorisation is needed before refining
            F.refine_dev(8, 8, 8, 1, 1, trans=True)
        assert e.value.code == hip.CS3_ERR_STATE


def test_general_transposed_triangular_solves(hip):
    """Bad shapes and misplaced diagonals are argument errors; a valid call runs on the GPU or says there is none."""
    L_p = np.array([0, 2, 3], dtype=np.int32)
    L_i = np.array([0, 1, 1], dtype=np.int32)
    L_x = np.array([2.0, 1.0, 4.0])
    U_p, U_i, U_x = L_p, np.array([0, 0, 1], dtype=np.int32), np.array([2.0, 1.0, 4.0])
    with pytest.raises(hip.Cs3Error) as e:
        hip.csc_ltsolve_f(2, U_p, U_i, U_x, np.ones(2))           # upper: the diagonal is not first
    assert e.value.code == hip.CS3_ERR_ARG
    with pytest.raises(hip.Cs3Error) as e:
        hip.csc_utsolve_f(2, L_p, L_i, L_x, np.ones(2))           # lower: the diagonal is not last
    assert e.value.code == hip.CS3_ERR_ARG
    x = np.array([4.0, 8.0])
    if hip.device_count() < 1:
        with pytest.raises(hip.Cs3Error) as e:
            hip.csc_ltsolve_f(2, L_p, L_i, L_x, x)
        assert e.value.code == hip.CS3_ERR_HIP and "no HIP device" in str(e.value)
    else:
        hip.csc_ltsolve_f(2, L_p, L_i, L_x, x)                   # L' = [[2, 1], [0, 4]]
        assert np.array_equal(x, [1.0, 2.0])


def test_trans_defaults_to_false_everywhere(hip):
    for fn in (hip.Factorization.solve, hip.Factorization.solve_dev, hip.Factorization.matvec_dev,
               hip.Factorization.residual_dev, hip.Factorization.refine_dev, csc_mod.CscMat.solve):
        assert inspect.signature(fn).parameters["trans"].default is False, fn.__qualname__
    assert callable(csc_mod.ltsolve) and callable(csc_mod.utsolve)


def test_live_device_buffers_stays_zero_without_a_device(hip):
    """cs3_debug_live_device_buffers counts the device blocks held: none before and after the no-device error returns."""
    if hip.device_count() > 0:
        return                                                    # (tests/test_gpu_lifetime.py covers a process with a device)
    assert hip.debug_live_device_buffers() == 0
    test_general_transposed_triangular_solves(hip)
    m, n, Ap, Ai, Ax, F = _toy(hip)
    with F:
        with pytest.raises(hip.Cs3Error) as e:
            F.factor(Ax)
        assert e.value.code == hip.CS3_ERR_HIP
    with pytest.raises(hip.Cs3Error) as e:
        hip.csc_transpose(m, n, Ap, Ai, Ax)
    assert e.value.code == hip.CS3_ERR_HIP
    assert hip.debug_live_device_buffers() == 0
