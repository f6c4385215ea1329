"""Complex matrices on the GPU: the glue kernels of the complex plan (rotation, values, pack, unpack, residual) bit for
bit against the NumPy restatement (tests/cplx_ref.py) through every branch of the rotation and at the edge of the
grid-stride loop; ComplexFactorization bit for bit against a plain handle fed by the restatement (the glue adds nothing);
its accuracy against the definition, in NumPy complex arithmetic; what the rotation buys; lifetime; CscMat / lusol.

"Bit for bit" is equality of the 64-bit words, with one exception that the formats force: where BOTH sides hold a NaN
(a NaN or infinite input times a zero), its sign and payload are not compared (canon_bits)."""
import gc

import numpy as np
import pytest

import cplx_cases as cases
import cplx_ref as ref
from csparse3_amd import synth

pytestmark = pytest.mark.gpu

OPS = {"N": ref.N, "T": ref.T, "H": ref.H}


def canon_bits(a):
    """The bit patterns of `a` with every NaN replaced by one NaN: IEEE 754 leaves the sign and payload of a NaN that an
    operation produces (0 * inf, inf - inf) to the implementation, and the host's differ from the device's.  Everything
    that is not a NaN is compared bit for bit, signed zeros included."""
    f = np.array(ref.bits(a).view(np.float64), copy=True)
    f[np.isnan(f)] = np.nan
    return f.view(np.uint64)


def same(got, want, quiet=False):
    g, w = canon_bits(got), canon_bits(want)
    if g.shape == w.shape and np.array_equal(g, w):
        return True
    if quiet:
        return False
    if g.shape != w.shape:
        print("shapes differ: %s against %s" % (g.shape, w.shape))
    else:
        bad = np.flatnonzero(g != w)
        print("%d of %d words differ; first: %s" % (len(bad), len(g), [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad[:6]]))
    return False


def dev_array(a, pad=1):
    """A device copy of `a` followed by `pad` NaN guard numbers.  -> (tensor, count)."""
    import torch
    a = np.ascontiguousarray(a)
    guard = np.full(pad, np.nan, dtype=a.dtype)
    return torch.from_numpy(np.concatenate([a.reshape(-1), guard])).to("cuda:0"), a.size


def guard_intact(t, count):
    return bool(np.isnan(t[count:].cpu().numpy()).all())


def glue_against_the_restatement(hip, n, Ap, Ai, Az, ks, rotate=True, ops=("N", "T", "H"), host_forms=True):
    """Every kernel of the plan, `_dev` form and host form, against the restatement.  Az [batch, nnz].  -> s."""
    import torch
    batch, nnz = Az.shape
    st = torch.cuda.current_stream().cuda_stream
    Azr, Azi = ref.split(Az)
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate)
    want_rx = ref.values(n, Ap, Ai, Azr, Azi, sr, si)
    rng = np.random.default_rng(n + 7 * batch)
    with hip.ComplexPlan(n, Ap, Ai, batch=batch, rotate=rotate) as plan:
        assert same(plan.rotation(), np.ones((batch, n), dtype=np.complex128)), "s before the first values call is not (1, +0)"
        d_az, _ = dev_array(Az)
        d_rx, cnt = dev_array(np.full((batch, 4 * nnz), np.nan))
        plan.values_dev(d_az.data_ptr(), d_rx.data_ptr(), st)
        torch.cuda.synchronize()
        assert guard_intact(d_rx, cnt)
        got_rx = d_rx[:cnt].cpu().numpy()
        if np.isfinite(Az.view(np.float64)).all():
            assert not np.isnan(want_rx).any()                               # (the restatement fills every entry: so must the kernel)
        assert same(got_rx, want_rx), "values_dev differs from the restatement"
        assert same(plan.rotation(), ref.join(sr, si)), "the rotation differs from the restatement"
        assert plan.rotation_dev() % 16 == 0
        if host_forms:
            assert same(plan.values(Az), want_rx), "values differs from values_dev"
        for k in ks:
            Z = rng.standard_normal((batch, n, k)) + 1j * rng.standard_normal((batch, n, k))
            Z.reshape(-1)[::5] = complex(0.0, -0.0)
            X = rng.standard_normal((batch, n, k)) + 1j * rng.standard_normal((batch, n, k))
            Zr, Zi = ref.split(Z)
            Xr, Xi = ref.split(X)
            Y = rng.standard_normal((batch, 2 * n, k))
            d_z, zc = dev_array(Z)
            d_x, _ = dev_array(X)
            d_yin, _ = dev_array(Y)
            for name in ops:
                op = OPS[name]
                # pack
                want = ref.pack(op, Zr, Zi, sr, si)
                d_y, yc = dev_array(np.full((batch, 2 * n, k), np.nan))
                plan.pack_dev(d_z.data_ptr(), d_y.data_ptr(), k, name, st)
                torch.cuda.synchronize()
                assert guard_intact(d_y, yc) and same(d_y[:yc].cpu().numpy(), want), "pack_dev %s k=%d" % (name, k)
                # unpack, stored and accumulated
                want_u = ref.join(*ref.unpack(op, Y, sr, si))
                want_a = ref.join(*ref.unpack(op, Y, sr, si, Xr, Xi))
                d_o, oc = dev_array(np.full((batch, n, k), np.nan + 0j))
                plan.unpack_dev(d_yin.data_ptr(), d_o.data_ptr(), k, name, False, st)
                d_acc, _ = dev_array(X)
                plan.unpack_dev(d_yin.data_ptr(), d_acc.data_ptr(), k, name, True, st)
                torch.cuda.synchronize()
                assert guard_intact(d_o, oc) and same(d_o[:oc].cpu().numpy(), want_u), "unpack_dev %s k=%d" % (name, k)
                assert guard_intact(d_acc, oc) and same(d_acc[:oc].cpu().numpy(), want_a), "unpack_dev accumulate %s k=%d" % (name, k)
                # residual, on the caller's values
                want_r = ref.join(*ref.residual(op, n, Ap, Ai, Azr, Azi, Zr, Zi, Xr, Xi))
                d_r, rc = dev_array(np.full((batch, n, k), np.nan + 0j))
                plan.residual_dev(d_az.data_ptr(), d_z.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), k, name, st)
                torch.cuda.synchronize()
                assert guard_intact(d_r, rc) and same(d_r[:rc].cpu().numpy(), want_r), "residual_dev %s k=%d" % (name, k)
                if host_forms:
                    shape = (batch, n, k) if batch > 1 else (n, k)
                    assert same(plan.pack(Z.reshape(shape), name), want), "pack %s k=%d" % (name, k)
                    assert same(plan.unpack(Y, name), want_u), "unpack %s k=%d" % (name, k)
                    assert same(plan.unpack(Y, name, into=X), want_a), "unpack accumulate %s k=%d" % (name, k)
                    assert same(plan.residual(Az, Z.reshape(shape), X.reshape(shape), name), want_r), "residual %s k=%d" % (name, k)
        return ref.join(sr, si)


@pytest.mark.parametrize("rotate", [True, False])
def test_every_branch_of_the_rotation(gpu, rotate):
    n, Ap, Ai, Az, kinds = cases.diag_zoo(np.random.default_rng(11))
    s = glue_against_the_restatement(gpu, n, Ap, Ai, Az, ks=(1, 2, 3, 17), rotate=rotate)[0]
    if not rotate:
        assert same(s, np.ones(n, dtype=np.complex128))
        return
    at = {kind: s[j] for j, kind in enumerate(kinds)}
    one = complex(1.0, 0.0)
    assert at["re"] == complex(1.0, 1.25 / 3.0) and at["im"] == complex(0.125, -1.0)
    assert at["tie"] == complex(1.0, 1.0) and at["tie_neg"] == complex(-1.0, 1.0) and at["neg"] == complex(-1.0, -0.05)
    for kind in ("zero", "neg_zero", "nan", "nan_im", "inf", "absent", "twice_cancel"):
        assert same(at[kind], one), kind
    assert at["twice"] == complex(1.0, 2.0 / (1e16 + 1.0))                    # (1e16 + 1) + j(1 - 3): both entries, added


def test_a_batch_rotates_every_matrix_by_its_own_diagonal(gpu):
    n, Ap, Ai, Az, kinds = cases.diag_zoo(np.random.default_rng(12), batch=3)
    s = glue_against_the_restatement(gpu, n, Ap, Ai, Az, ks=(1, 3))
    assert not same(s[0], s[1], quiet=True) and not same(s[1], s[2], quiet=True)


def test_order_one(gpu):
    n, Ap, Ai = cases.structural_cases()["n1"]
    for z in (0.5 - 2.0j, complex(-0.0, 0.0), -3.0 + 0.0j):
        glue_against_the_restatement(gpu, n, Ap, Ai, np.array([[z]]), ks=(1, 2))


@pytest.mark.parametrize("name", ["unsorted", "absent_diagonal", "diag_twice", "empty_column"])
def test_structural_cases(gpu, name):
    n, Ap, Ai = cases.structural_cases()[name]
    Az = cases.values_for(np.random.default_rng(13), int(Ap[n]), batch=2)
    glue_against_the_restatement(gpu, n, Ap, Ai, Az, ks=(1, 3))


def test_one_entry_past_the_grid_takes_a_second_pass(gpu):
    """grid_cap * block + 1 entries (values), rows (rotation) and right-hand-side numbers (pack, unpack, residual)."""
    lim = gpu.cplx_limits()
    n, Ap, Ai, Az = cases.diagonal_matrix(int(lim.grid_cap * lim.block) + 1, np.random.default_rng(14))
    glue_against_the_restatement(gpu, n, Ap, Ai, Az, ks=(1,), host_forms=False)


def test_arrays_that_are_not_aligned_are_refused(gpu):
    import torch
    n, Ap, Ai = cases.structural_cases()["n2"]
    with gpu.ComplexPlan(n, Ap, Ai) as plan:
        buf = torch.zeros(64, dtype=torch.float64, device="cuda:0")
        p = buf.data_ptr()
        for call in (lambda: plan.values_dev(p + 8, p + 128), lambda: plan.values_dev(p, p + 136), lambda: plan.pack_dev(p + 8, p + 128),
                     lambda: plan.pack_dev(p, p + 132), lambda: plan.unpack_dev(p + 128, p + 8),
                     lambda: plan.residual_dev(p, p + 128, p + 256, p + 392), lambda: plan.pack_dev(p, p + 128, 1, 3)):
            with pytest.raises((gpu.Cs3Error, AssertionError)):
                call()
        plan.pack_dev(p, p + 136, 1)                                         # Y needs 8 bytes only
        torch.cuda.synchronize()


# ------------------------------------------------------------------ the glue adds nothing --

YBUS = {"ybus40": synth.ybus(40, 60, seed=40), "ybus300": synth.ybus(300, 480, seed=300)}
BATCH = 2


def batch_values(Az, lossless=False):
    """[BATCH, nnz]: the matrix and a second one with other values on the same pattern."""
    rng = np.random.default_rng(len(Az))
    scale = 1.0 + 0.2 * rng.uniform(-1.0, 1.0, len(Az))
    other = Az * scale if lossless else Az * scale + 0.01 * rng.uniform(0.0, 1.0, len(Az))
    return np.stack([Az, other])


def rhs(n, k, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((BATCH, n, k)) + 1j * rng.standard_normal((BATCH, n, k))


def residual_bound(n, Ap, Az, x, b):
    return 1e-12 * (cases.norm1(n, Ap, Az) * np.abs(x).max() + np.abs(b).max())


def assert_solves(n, Ap, Ai, Az2, x, b, op, what=""):
    """max |b - op(A) x| <= 1e-12 (||A||_1 max|x| + max|b|) per matrix, in NumPy complex arithmetic.  (||A||_1 is that of A
    for every op: the bound of tests/test_gpu_parity.py:59.)"""
    worst = 0.0
    for m in range(len(Az2)):
        A = ref.apply_op(op, ref.dense_complex(n, Ap, Ai, Az2[m]))
        res = np.abs(b[m] - A @ x[m]).max()
        bound = residual_bound(n, Ap, Az2[m], x[m], b[m])
        print("%s matrix %d: residual %.3e, bound %.3e" % (what, m, res, bound))
        assert res <= bound, "%s matrix %d: residual %.3e > %.3e" % (what, m, res, bound)
        worst = max(worst, res / bound)
    return worst


@pytest.fixture(scope="module")
def solved(gpu):
    """name -> (Az2, F factorised): ONE ComplexFactorization per matrix for the tests below; closed at the end."""
    made = {}
    for name, (n, Ap, Ai, Az) in YBUS.items():
        Az2 = batch_values(Az)
        made[name] = (Az2, gpu.ComplexFactorization(n, Ap, Ai, batch=BATCH).factor(Az2))
    yield made
    for _, F in made.values():
        F.close()


@pytest.mark.parametrize("name", sorted(YBUS))
@pytest.mark.parametrize("k", [1, 3])
def test_solve_is_a_plain_handle_on_the_restated_arrays(gpu, solved, name, k):
    n, Ap, Ai, _ = YBUS[name]
    Az2, F = solved[name]
    Azr, Azi = ref.split(Az2)
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, True)
    Rp, Ri = ref.real_pattern(n, Ap, Ai)
    q2 = ref.doubled_order(gpu.csc_amd_f(gpu.ORDER_AMD, n, n, Ap, Ai))
    b = rhs(n, k)
    Br, Bi = ref.split(b)
    with gpu.Factorization(2 * n, 2 * n, Rp, Ri, q=q2, batch=BATCH) as P:
        P.factor(ref.values(n, Ap, Ai, Azr, Azi, sr, si))
        for opname, op in OPS.items():
            want = ref.join(*ref.unpack(op, P.solve(ref.pack(op, Br, Bi, sr, si), trans=op != ref.N), sr, si))
            got = F.solve(b, trans=opname)
            assert got.shape == b.shape and got.dtype == np.complex128
            assert same(got, want), "%s k=%d op %s: the glue changed the bits" % (name, k, opname)
            assert_solves(n, Ap, Ai, Az2, got, b, op, "%s k=%d op %s" % (name, k, opname))


@pytest.mark.parametrize("name", sorted(YBUS))
@pytest.mark.parametrize("k", [1, 3])
def test_factor_solve_dev_gives_the_bits_of_factor_and_solve(gpu, solved, name, k):
    import torch
    n, Ap, Ai, _ = YBUS[name]
    Az2, F = solved[name]
    b = rhs(n, k, seed=6)
    want = F.solve(b)
    st = torch.cuda.current_stream().cuda_stream
    d_az, d_b = torch.from_numpy(Az2).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    with gpu.ComplexFactorization(n, Ap, Ai, batch=BATCH) as G:
        d_x, xc = dev_array(np.full(b.shape, np.nan + 0j))
        G.factor_solve_dev(d_az.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), k, 0.0, st)
        G.factor_status(st)
        assert guard_intact(d_x, xc) and same(d_x[:xc].cpu().numpy(), want)
        assert same(d_b.cpu().numpy(), b), "the right-hand side was overwritten"
        for opname in OPS:                                                   # solve_dev on the same factors, in place too
            d_y = d_b.clone()
            G.solve_dev(d_y.data_ptr(), d_y.data_ptr(), k, st, trans=opname)
            torch.cuda.synchronize()
            assert same(d_y.cpu().numpy(), F.solve(b, trans=opname)), opname


@pytest.mark.parametrize("name", sorted(YBUS))
def test_one_refinement_step_stays_within_the_bound(gpu, solved, name):
    n, Ap, Ai, _ = YBUS[name]
    Az2, F = solved[name]
    b = rhs(n, 3, seed=8)
    for opname, op in OPS.items():
        x = F.solve(b, trans=opname)
        r = F.residual(Az2, b, x, trans=opname)
        for m in range(BATCH):                                               # (the kernel's bits are checked above: this is the definition)
            want_r = b[m] - ref.apply_op(op, ref.dense_complex(n, Ap, Ai, Az2[m])) @ x[m]
            assert np.abs(r[m] - want_r).max() <= residual_bound(n, Ap, Az2[m], x[m], b[m])
        x1 = F.refine(Az2, b, x, steps=1, trans=opname)
        assert x1.shape == x.shape and not same(x1, x, quiet=True)
        assert_solves(n, Ap, Ai, Az2, x1, b, op, "%s refined, op %s" % (name, opname))


# ------------------------------------------------------------------ the rotation earns its place --

def test_a_lossless_network_needs_the_rotation(gpu):
    n, Ap, Ai, Az = synth.ybus(40, 60, seed=40, lossless=True)
    Az2 = batch_values(Az, lossless=True)
    assert not Az2.real.any()
    b = rhs(n, 3, seed=9)
    with gpu.ComplexFactorization(n, Ap, Ai, batch=BATCH, rotate=False) as F:
        with pytest.raises(gpu.SingularMatrix):                                # the first pivot is Re d = 0, exactly
            F.factor(Az2)
    with gpu.ComplexFactorization(n, Ap, Ai, batch=BATCH, rotate=True) as F:
        F.factor(Az2)
        for opname, op in OPS.items():
            assert_solves(n, Ap, Ai, Az2, F.solve(b, trans=opname), b, op, "lossless, op %s" % opname)


def test_the_rotated_matrix_passes_the_pivot_test(gpu):
    n, Ap, Ai, Az = YBUS["ybus300"]
    Az2 = batch_values(Az)
    b = rhs(n, 1, seed=10)
    with gpu.ComplexFactorization(n, Ap, Ai, batch=BATCH) as F:
        x = F.factor(Az2, tol=1e-3).solve(b)
        assert_solves(n, Ap, Ai, Az2, x, b, ref.N, "tol 1e-3")
        # the real handle stays reachable: log|det| of the real form is twice that of diag(s) A
        sign, logabs = F.real.slogdet()
        s = F.plan.rotation()
        for m in range(BATCH):
            want = np.linalg.slogdet(ref.dense_complex(n, Ap, Ai, Az2[m]))[1]
            assert abs(logabs[m] / 2 - np.log(np.abs(s[m])).sum() - want) <= 1e-9 * abs(want) and sign[m] == 1.0


def test_hermitian_positive_definite_through_cholesky(gpu):
    from csparse3_amd import csc
    n, Ap, Ai, Az = cases.hermitian_pd(300, 480, seed=3)
    rng = np.random.default_rng(4)
    b = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    A = csc.CscMat(n, n, indptr=Ap, indices=Ai, data=Az)
    F = A.chol()
    assert isinstance(F, gpu.ComplexFactorization) and F.kind == gpu.CS3_CHOLESKY and not F.plan.rotate
    for opname, op in OPS.items():
        assert_solves(n, Ap, Ai, Az[None], F.solve(b, trans=opname)[None], b[None], op, "chol, op %s" % opname)
    x = csc.cholsol(A, b[:, 0].copy())
    assert same(x, F.solve(b[:, 0].copy()))
    assert A._factorization[1] is F, "cholsol did not reuse the analysis"
    F.close()


# ------------------------------------------------------------------ lifetime --

def test_buffers_go_back_and_a_repeated_call_allocates_nothing(gpu):
    import torch
    gc.collect()
    start = gpu.debug_live_device_buffers()
    n, Ap, Ai, Az = YBUS["ybus40"]
    st = torch.cuda.current_stream().cuda_stream
    d_az = torch.from_numpy(Az).to("cuda:0")
    for k in (2, 5):
        b = rhs(n, k, seed=k)[0]
        d_b = torch.from_numpy(b).to("cuda:0")
        d_x = torch.empty_like(d_b)
        with gpu.ComplexPlan(n, Ap, Ai) as plan:
            plan.values(Az)
            plan.pack(b)
            assert gpu.debug_live_device_buffers() > start
        assert gpu.debug_live_device_buffers() == start
        with gpu.ComplexFactorization(n, Ap, Ai) as F:
            F.factor_solve_dev(d_az.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), k, 0.0, st)
            F.factor_status(st)
            first = d_x.cpu().numpy()
            live, counters = gpu.debug_live_device_buffers(), F.real.debug_alloc_counters()
            F.factor_solve_dev(d_az.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), k, 0.0, st)
            assert F.real.debug_alloc_counters() == counters, "a second call with the same k allocated or synchronised"
            F.factor_status(st)
            assert gpu.debug_live_device_buffers() == live
            assert same(d_x.cpu().numpy(), first)
            assert live > start
        assert gpu.debug_live_device_buffers() == start


# ------------------------------------------------------------------ CscMat / lusol --

def test_cscmat_and_lusol_with_complex_data(gpu):
    from csparse3_amd import csc
    n, Ap, Ai, Az = YBUS["ybus40"]
    A = csc.CscMat(n, n, indptr=Ap, indices=Ai, data=Az.copy())
    D = A.todense()
    rng = np.random.default_rng(15)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    tol = lambda want: 1e-10 * np.abs(want).max()                           # noqa: E731  (cond about 8e2: 1e3 x cond x 2^-53)
    x = csc.lusol(A, b)
    assert x.dtype == np.complex128 and x.shape == (n,)
    want = np.linalg.solve(D, b)
    assert np.abs(x - want).max() <= tol(want)
    F = A._factorization[1]
    assert isinstance(F, gpu.ComplexFactorization)
    for trans, M in (("N", D), ("T", D.T), ("H", D.conj().T), (True, D.T), (False, D)):
        want = np.linalg.solve(M, b)
        assert np.abs(A.solve(b, trans=trans) - want).max() <= tol(want)
    B = rng.standard_normal((n, 4)) + 1j * rng.standard_normal((n, 4))
    want = np.linalg.solve(D, B)
    assert np.abs(A.solve(B) - want).max() <= tol(want)
    assert A._factorization[1] is F
    # new values on the same pattern: a refactorisation on the analysis at hand
    A.data[:] = Az * (1.0 + 0.1 * rng.uniform(-1, 1, len(Az)))
    D2 = A.todense()
    want = np.linalg.solve(D2, b)
    assert np.abs(A.solve(b) - want).max() <= tol(want)
    assert A.lu() is F and A._factorization[1] is F
    assert A.lu(rotate=False) is not F                                        # (another plan: another analysis)
    A._factorization[1].close()


def test_real_data_takes_the_path_it_took(gpu):
    from csparse3_amd import csc
    m, n, Ap, Ai, Ax = synth.jacobian_config2()
    b = np.random.default_rng(16).standard_normal(n)
    A = csc.CscMat(m, n, indptr=Ap, indices=Ai, data=Ax)
    with gpu.Factorization(m, n, Ap, Ai) as P:
        want = P.factor(Ax, 1e-3).solve(b)
        want_t = P.solve(b, trans=True)
    F = A.lu(1e-3)
    assert type(F) is gpu.Factorization
    assert same(A.solve(b, tol=1e-3), want) and same(A.solve(b, tol=1e-3, trans=True), want_t)
    assert same(csc.lusol(A, b, tol=1e-3), want)
    assert A.todense().dtype == np.float64
    F.close()
