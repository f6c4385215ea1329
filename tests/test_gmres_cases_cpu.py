"""The conditions on the inputs of tests/test_gpu_gmres_edges.py, on the CPU: with them a failure of a GPU test can only be
the kernels'.  The cases are those of tests/gmres_cases.py (spread_case and what is built on it), the method is
tests/gmres_ref.py, every run is from x0 = M^-1 b with rtol = 0 and an iteration cap m unless it says otherwise.

Measured with this file on spread_case(300, 7, 40) (cond A = 2.4e2, cond A0 = 9.9), GMRES(32):

    m                          8       9       16      17      24      25      31      32      33      41
    true relres                6.7e-2  4.5e-2  2.7e-3  2.0e-3  1.5e-5  4.7e-6  2.1e-8  5.8e-9  2.1e-9  1.5e-11
    max|x_m - x_{m-1}| / max|x_m|  3.6e-2  1.8e-2  2.1e-3  9.9e-4  9.8e-6  1.4e-6  6.5e-9  5.2e-9  4.7e-10 2.5e-12

(the second row is helpers.rel_err, the measure the GPU tests assert on).  The two CPU variants (splu of A0, and
inv(A0.toarray()) @ v as the solve) over every single-system run the GPU tests make: x differs by at most 7.6e-16, relres
by 1.0e-15 .. 1.2e-15 (absolute; the figure depends on the host's BLAS), |estimate - true| at a cycle's end is at most
1.0e-15 .. 1.2e-15; the reference's basis at depth 32 has max |V'V - I| = 5.6e-16.  The GPU gets 10 x each (x floored at
1e-13)."""
import numpy as np
import pytest

import gmres_cases as gc
from csparse3_amd import csc_hip


def _monotone(h):
    return all(b <= a * (1 + 1e-12) for a, b in zip(h, h[1:]))


def _check_run(res, m):
    assert res.iters == m, (res.iters, m)
    assert np.isfinite(res.relres) and res.relres > 0.0
    assert len(res.history) == m and _monotone(res.history), res.history


def test_spread_case_is_diag_case_with_a_factor_per_row():
    c, d = gc.deep_case(), gc.diag_case(300, 7, 40)
    assert np.array_equal(c.rows, d.rows) and np.array_equal(c.b, d.b) and len(c.rows) == 40
    ratio = c.A.diagonal() / c.A0.diagonal()
    assert np.allclose(ratio[c.rows], 2.0 + np.arange(40), rtol=1e-15)
    rest = np.setdiff1d(np.arange(300), c.rows)
    assert np.array_equal(ratio[rest], np.ones(260))
    assert (c.A - c.A0).nnz == 40
    # GMRES(32) at 1e-12 fills a cycle and restarts, with a smooth history: no count to assert on
    full = gc.reference(c, rtol=1e-12, restart=32, max_iters=100)
    print("cond A %.2e cond A0 %.2e; GMRES(32) at 1e-12: %d iterations"
          % (np.linalg.cond(c.A.toarray()), np.linalg.cond(c.A0.toarray()), full.iters))
    assert full.iters > 32 and full.relres <= 1e-12


def test_bounds_come_from_the_two_cpu_variants():
    eb = gc.edge_bounds()
    print("variants: x %.3e relres %.3e |estimate - true| %.3e; bounds x %.3e relres %.3e gap %.3e"
          % (eb.ref_x, eb.ref_relres, eb.ref_gap, eb.x, eb.relres, eb.gap))
    assert 0.0 < eb.ref_x <= 1e-14 and 0.0 < eb.ref_relres <= 1e-14 and 0.0 < eb.ref_gap <= 1e-14
    assert eb.x == max(10.0 * eb.ref_x, gc.X_FLOOR) and eb.relres == 10.0 * eb.ref_relres and eb.gap == 10.0 * eb.ref_gap


@pytest.mark.parametrize("m", gc.DEEP_CAPS)
def test_deep_caps_run_exactly_m_iterations_and_separate_x(m):
    c = gc.deep_case()
    res = gc.capped(c, m)
    _check_run(res, m)
    assert len(res.cycles) == -(-m // 32)
    sep = gc.rel_diff(gc.capped(c, m - 1).x, res.x)
    print("m=%d relres %.3e |x_m - x_(m-1)| / |x_m| %.3e" % (m, res.relres, sep))
    if m <= 33:                                            # m = 41 serves the relres, gap and stale-memory checks only
        assert sep >= 1000.0 * gc.edge_bounds().x, (sep, gc.edge_bounds().x)


@pytest.mark.parametrize("restart", gc.BOUNDARY_RESTARTS)
def test_restart_at_the_pass_boundary(restart):
    c, m = gc.deep_case(), 2 * restart + 1
    res = gc.capped(c, m, restart)
    _check_run(res, m)
    assert len(res.cycles) == 3
    sep = gc.rel_diff(gc.capped(c, m - 1, restart).x, res.x)
    print("restart=%d m=%d relres %.3e separation %.3e" % (restart, m, res.relres, sep))
    assert sep >= 1000.0 * gc.edge_bounds().x


@pytest.mark.parametrize("k,m", gc.TILE_CASES)
def test_tile_cases(k, m):
    c, B = gc.deep_case(), gc.tile_rhs(k)
    for t in range(k):
        res = gc.capped(c, m, b=(("tile", k, t), B[:, t]))
        _check_run(res, m)
        sep = gc.rel_diff(gc.capped(c, m - 1, b=(("tile", k, t), B[:, t])).x, res.x)
        assert sep >= 1000.0 * gc.edge_bounds().x, (t, sep)


def test_grid_cases():
    lim = csc_hip.gmres_limits()
    cases, B = gc.grid_cases(lim.chunk_rows, lim.rhs_tile)
    n, k = lim.chunk_rows + 1, lim.rhs_tile + 1
    assert B.shape == (2, n, k) and all(c.mat[1] == n for c in cases)
    assert np.array_equal(cases[0].mat[2], cases[1].mat[2]) and not np.array_equal(cases[0].Ax, cases[1].Ax)
    for b, c in enumerate(cases):
        for t in range(k):
            res = gc.capped(c, 17, b=(("grid", b, t), B[b, :, t]))
            _check_run(res, 17)
            sep = gc.rel_diff(gc.capped(c, 16, b=(("grid", b, t), B[b, :, t])).x, res.x)
            if t in (0, k - 1):
                print("matrix %d column %d: relres %.3e separation %.3e" % (b, t, res.relres, sep))
            assert sep >= 1000.0 * gc.edge_bounds().x


def test_transposed_deep():
    c = gc.deep_case()
    res = gc.capped(c, 17, trans=True)
    _check_run(res, 17)
    sep = gc.rel_diff(gc.capped(c, 16, trans=True).x, res.x)
    assert sep >= 1000.0 * gc.edge_bounds().x
    assert gc.rel_diff(res.x, gc.capped(c, 17).x) > 1e-3, "the transposed system is another system"


def test_freeze_batch_freezes_where_stated():
    fb = gc.freeze_batch()
    iters = [r.iters for r in fb.refs]
    print("r=%d rtol %.3e iters %s relres %s" % (fb.r, fb.rtol, iters, ["%.2e" % r.relres for r in fb.refs]))
    assert 10 <= fb.r <= 14
    # matrix 0: past the first pass of 8 basis vectors, inside the second; a 10 x gap around rtol in both systems
    for s in (0, 1):
        r = fb.refs[s]
        assert 9 <= r.iters <= 16 and r.ncols == r.iters and r.relres <= fb.rtol
        h = r.history
        assert h[-2] >= 10.0 * h[-1] and h[-2] > fb.rtol > h[-1]
        assert h[-2] >= 3.0 * fb.rtol and h[-1] <= fb.rtol / 3.0
        assert min(x for x in h[:-1]) >= 3.0 * fb.rtol
        assert r.V.shape[1] == r.ncols
    assert iters[0] == iters[1]
    # matrix 1 goes on to the cap, nowhere near rtol
    for s in (2, 3):
        r = fb.refs[s]
        assert r.iters == 32 and r.ncols == 32 and r.relres >= 100.0 * fb.rtol and min(r.history) >= 100.0 * fb.rtol
        assert gc.basis_defect(r.V) <= 1e-14
    # matrix 2: nothing to do, and a zero right-hand side
    assert iters[4:] == [0, 0] and 0.0 < fb.refs[4].relres <= fb.rtol / 100.0
    assert fb.refs[5].relres == 0.0 and not fb.refs[5].x.any() and not fb.B[2, :, 1].any()


def test_reference_basis_is_orthonormal_at_depth_32():
    d = gc.reference_basis_defect()
    print("reference: max |V'V - I| at depth 32 = %.3e" % d)
    assert 0.0 < d <= 1e-14
