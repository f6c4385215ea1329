"""The kernels of csrc/krylov.hip past 8 basis vectors, at restart 32 and at every tile width (cs3_gmres on the deep cases
of tests/gmres_cases.py; tests/test_gmres_cases_cpu.py holds the conditions on these inputs).

Every run is capped: rtol = 0 and max_iters = m, so the iteration count is m by construction and x after exactly m
iterations is the target -- it moves by >= 1000 x the x bound per iteration up to m = 33 (CPU test), so a dropped or
wrong basis vector cannot hide.  Bounds (gmres_cases.edge_bounds): 10 x what two CPU variants of the same method differ by
-- x 7.6e-16 (floored: bound 1e-13), relres 1.0e-15 .. 1.2e-15 by host, |estimate - true| at a cycle's end the same -- and
for the basis 10 x the reference's max |V'V - I| = 5.6e-16 at depth 32.  Every test prints the GPU's figures before it
asserts; the largest over the module: x 2.9e-15, relres 3.4e-15, |estimate - true| 1.4e-15, max |V'V - I| 4.4e-16
(DESIGN.md section 7).

test_freezing_past_a_pass_boundary is also the regression test of the work memory's size: before ensure_krylov (api.cpp)
counted both Gram-Schmidt passes' sums, it returned iterations [24, 0, 0, 19, 0, 0] for [12, 12, 32, 32, 0, 0].

The basis comes through debug_gmres_basis.  Its vector 0 is rewritten by the call's closing residual check (zeros once
every system is finished), so v_0 is rebuilt on the host from the same x0: (b - A x0) / ||b - A x0||."""
import numpy as np
import pytest

import gmres_cases as gc
from helpers import rel_err

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def lim(gpu):
    out = gpu.gmres_limits()
    assert (out.max_restart, out.rhs_tile, out.chunk_rows) == (32, 64, 1024), "the cases below sit at these edges"
    return out


@pytest.fixture(scope="module")
def held(gpu):
    """Handles factorised from A0, one per (n, pattern, batch), shared by the tests of this module."""
    made = {}

    def get(case, batch=1):
        key = (case.mat[1], case.mat[2].tobytes(), batch)
        if key not in made:
            m, n, Ap, Ai, Ax0 = case.mat
            F = gpu.Factorization(m, n, Ap, Ai, batch=batch)
            F.factor(np.tile(Ax0, (batch, 1)) if batch > 1 else Ax0)
            made[key] = F
        return made[key]

    yield get
    for F in made.values():
        F.close()


def _figures(x, iters, relres, est, ref):
    """(iters, x error, |relres - reference|, |estimate - relres|) of one system against its reference."""
    return int(iters), rel_err(x, ref.x), abs(float(relres) - ref.relres), abs(float(est) - float(relres))


def _assert_system(tag, fig, m, rows=""):
    eb = gc.edge_bounds()
    it, ex, er, eg = fig
    assert it == m, "%s: %d iterations, want %d" % (tag, it, m)
    assert ex <= eb.x, "%s: x differs by %.3e (bound %.3e)%s" % (tag, ex, eb.x, rows)
    assert er <= eb.relres, "%s: relres differs by %.3e (bound %.3e)" % (tag, er, eb.relres)
    assert eg <= eb.gap, "%s: |estimate - true| = %.3e (bound %.3e)" % (tag, eg, eb.gap)


def _report(tag, figs):
    eb = gc.edge_bounds()
    print("%s: x %.3e (bound %.3e) relres %.3e (%.3e) |estimate - true| %.3e (%.3e)"
          % (tag, max(f[1] for f in figs), eb.x, max(f[2] for f in figs), eb.relres, max(f[3] for f in figs), eb.gap))


def _capped_single(F, case, m, restart, trans=False):
    x0 = F.solve(case.b, trans)
    x, iters, relres = F.gmres(case.Ax, case.b, x0=x0, rtol=0.0, restart=restart, max_iters=m, trans=trans)
    est = F.debug_gmres_estimates(1)
    fig = _figures(x, iters[0], relres[0], est[0], gc.capped(case, m, restart, trans=trans))
    tag = "restart=%d m=%d%s" % (restart, m, " trans" if trans else "")
    _report(tag, [fig])
    _assert_system(tag, fig, m)


def _v0(case, b, x0):
    r = b - case.A @ x0
    return r / np.sqrt(np.dot(r, r))


def _defect(tag, v0, V):
    """max |V'V - I| of [v0, the columns V [nvec, n]], printed and held against 10 x the reference's."""
    d, bound = gc.basis_defect(np.column_stack([v0] + list(V))), 10.0 * gc.reference_basis_defect()
    print("%s: max |V'V - I| over %d vectors = %.3e (bound %.3e)" % (tag, 1 + len(V), d, bound))
    assert d <= bound, tag


# 1. the passes of 8 basis vectors of the multi-dot, the full cycle of 32, the iteration after it (basis vector 33 written,
#    h filled to its last row), and a second cycle of 9 columns over the 32 of the first
@pytest.mark.parametrize("m", gc.DEEP_CAPS)
def test_pass_and_restart_edges(gpu, held, lim, m):
    assert lim.max_restart + 1 in gc.DEEP_CAPS
    case = gc.deep_case()
    _capped_single(held(case), case, m, lim.max_restart)


# 2. the restart at the pass boundary: three cycles, the last of one column
@pytest.mark.parametrize("restart", gc.BOUNDARY_RESTARTS)
def test_restart_at_the_pass_boundary(gpu, held, lim, restart):
    case = gc.deep_case()
    _capped_single(held(case), case, 2 * restart + 1, restart)


# 3. every tile width TX = 8, 16, 32, 64 (and 64 + 1 column), deep enough that the strided loads of h and y wrap
#    (j + 1 = 17 > 256 / TX for TX >= 16; k = 8 at m = 32 puts i = 31 on the last ty without wrapping)
@pytest.mark.parametrize("k,m", gc.TILE_CASES)
def test_tile_widths(gpu, held, lim, k, m):
    case, B = gc.deep_case(), gc.tile_rhs(k)
    F = held(case)
    x, iters, relres = F.gmres(case.Ax, B, x0=F.solve(B), rtol=0.0, restart=lim.max_restart, max_iters=m)
    est = F.debug_gmres_estimates(k)
    figs = [_figures(x[:, t], iters[t], relres[t], est[t], gc.capped(case, m, b=(("tile", k, t), B[:, t]))) for t in range(k)]
    _report("k=%d m=%d" % (k, m), figs)
    for t in range(k):
        _assert_system("k=%d m=%d column %d" % (k, m, t), figs[t], m)


# 4. two systems freeze at column 12, inside the second pass of 8, while their neighbours go on to column 32 or never start
def test_freezing_past_a_pass_boundary(gpu, held, lim):
    fb = gc.freeze_batch()
    F = held(fb.cases[0], batch=3)
    n, restart = fb.mat[1], lim.max_restart
    x0 = F.solve(fb.B)
    x, iters, relres = F.gmres(fb.AX, fb.B, x0=x0, rtol=fb.rtol, restart=restart, max_iters=restart)
    V = F.debug_gmres_basis(restart + 1, 2)
    want = [r.iters for r in fb.refs]
    print("r=%d rtol %.3e: iters %s reference %s relres %s" % (fb.r, fb.rtol, iters, want, relres))
    assert list(iters) == want
    eb = gc.edge_bounds()
    for s, ref in enumerate(fb.refs):
        b, t = divmod(s, 2)
        if not fb.B[b, :, t].any():
            assert not x[b, :, t].any() and relres[s] == 0.0
            continue
        err = rel_err(x[b, :, t], ref.x)
        print("system %d: x %.3e (bound %.3e) relres %.3e" % (s, err, eb.x, relres[s]))
        assert err <= eb.x, s
        assert relres[s] <= fb.rtol if want[s] < restart else abs(relres[s] - ref.relres) <= eb.relres, s
    assert V.shape == (restart + 1, 3, n, 2)
    assert not _bits(V[0]).any(), "the closing residual check leaves zeros in vector 0 of finished systems"
    for t in range(2):
        c = want[t]                                        # matrix 0: columns 1 .. c - 1 built, exact zeros from c on
        assert 8 < c < 16
        assert all(V[i, 0, :, t].any() for i in range(1, c)), t
        assert not _bits(V[c:, 0, :, t]).any(), "system %d: the basis behind column %d is not exact zeros" % (t, c)
        _defect("frozen system %d" % t, _v0(fb.cases[0], fb.B[0, :, t], x0[0, :, t]), V[1:c, 0, :, t])
        assert not _bits(V[restart, 1, :, t]).any()        # matrix 1: out of iterations at column 32
        _defect("system %d" % (2 + t), _v0(fb.cases[1], fb.B[1, :, t], x0[1, :, t]), V[1:restart, 1, :, t])
    assert not _bits(V[:, 2]).any(), "matrix 2 never iterates: no basis vector of it may be non-zero"
    x2, iters2, relres2 = F.gmres(fb.AX, fb.B, x0=x0, rtol=fb.rtol, restart=restart, max_iters=restart)
    assert _same_bits(x, x2) and np.array_equal(iters, iters2) and _same_bits(relres, relres2)


# 5. chunks, tiles of right-hand sides and matrices all 2: tile_of splits blockIdx.x three ways
def test_all_three_grid_factors(gpu, held, lim):
    cases, B = gc.grid_cases(lim.chunk_rows, lim.rhs_tile)
    n, k, m, cr = lim.chunk_rows + 1, lim.rhs_tile + 1, 17, lim.chunk_rows
    F = held(cases[0], batch=2)
    AX = np.stack([c.Ax for c in cases])
    x0 = F.solve(B)
    x, iters, relres = F.gmres(AX, B, x0=x0, rtol=0.0, restart=lim.max_restart, max_iters=m)
    est = F.debug_gmres_estimates(2 * k)
    V = F.debug_gmres_basis(m + 1, k)
    refs = [gc.capped(cases[b], m, b=(("grid", b, t), B[b, :, t])) for b in range(2) for t in range(k)]
    figs = [_figures(x[s // k, :, s % k], iters[s], relres[s], est[s], refs[s]) for s in range(2 * k)]
    _report("n=%d k=%d batch=2 m=%d" % (n, k, m), figs)
    for s in range(2 * k):
        b, t = divmod(s, k)
        d = np.abs(x[b, :, t] - refs[s].x) / np.abs(refs[s].x).max()
        named = [i for i in (cr - 1, cr, n - 1) if d[i] > gc.edge_bounds().x]
        _assert_system("matrix %d column %d" % (b, t), figs[s], m, "; chunk-edge rows that differ: %s" % named if named else "")
    assert V.shape == (m + 1, 2, n, k)
    for s in sorted({0, lim.rhs_tile - 1, k - 1, k, 2 * k - 1}):
        b, t = divmod(s, k)
        assert not _bits(V[m, b, :, t]).any()
        _defect("system %d" % s, _v0(cases[b], B[b, :, t], x0[b, :, t]), V[1:m, b, :, t])


# 6. the transposed system: the column view feeds the same vector kernels
def test_transposed_deep(gpu, held, lim):
    case = gc.deep_case()
    _capped_single(held(case), case, 17, lim.max_restart, trans=True)
