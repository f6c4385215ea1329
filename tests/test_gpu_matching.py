"""Matched handles (cs3_analyze_matched) on the GPU: matrices that a plain handle rejects (zero diagonals, scrambled
scalings, saddle-point systems) factor after matching + scaling, and every entry point keeps speaking in terms of A.

References: the oracle (cs_lu) on the scaled matrix B rebuilt on the host bit for bit, with the library's q, where
tests/test_matching_cpu.py has shown that it keeps every diagonal; the oracle with partial pivoting (tol = 1) on A itself;
dense NumPy for the scalar results.  One set of references per case and process (_ref)."""
import ctypes as C
import gc

import numpy as np
import pytest

import match_cases as mc
import pivot_cases as pc
from csparse3_amd import synth
from helpers import RTOL, assert_factor_equal, csc_to_scipy, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3
KS = (1, 3, 16, 64, 256)                  # 256: beyond the width at which a plain handle fuses its permutations


def _poison(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


def _oracle_solver(orc, n, Ap, Ai, Ax, q, tol):
    """What orc.csc_lusol_f does after its ordering, with the factors kept: -> (solve(B [n, k]) -> X, pinv)."""
    Lp, Li, Lx, Up, Ui, Ux, pinv = orc.csc_lu_f(n, n, Ap, Ai, Ax, q, tol)

    def solve(B):
        B = B.reshape(n, -1)
        X = np.empty_like(B)
        for c in range(B.shape[1]):
            x = np.empty(n)
            x[pinv] = B[:, c]
            orc.csc_lsolve_f(n, Lp, Li, Lx, x)
            orc.csc_usolve_f(n, Up, Ui, Ux, x)
            X[q, c] = x
        return X
    return solve, pinv


def _transposed(n, Ap, Ai, Ax):
    T = csc_to_scipy(n, n, Ap, Ai, Ax).T.tocsc()
    T.sort_indices()
    return T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()


_REF = {}


def _ref(gpu, orc, name):
    """Per case: the matching and q of a matched handle, B, right-hand sides [n, 256], and the oracle's answers."""
    if name not in _REF:
        c = mc.case(name)
        with gpu.Factorization(c.n, c.n, c.Ap, c.Ai, batch=c.batch, match_values=c.Ax) as F:
            rowperm, dr, dc = F.matching()
            q = F.ordering()["q"]
        _REF[name] = dict(c=c, rowperm=rowperm, dr=dr, dc=dc, q=q, B=mc.scaled(c, c.Ax, rowperm, dr, dc),
                          rhs=np.random.default_rng(11).standard_normal((c.n, KS[-1])))
    return _REF[name]


def _ref_solutions(gpu, orc, name):
    """+ y = B^-1 (dr b)[rowperm] and z = B^-T (dc b) by the oracle's static-order factors of B, x = A^-1 b and A^-T b by the
    oracle with partial pivoting on A and A' themselves (orc.csc_lusol_f's computation, factors kept for all columns)."""
    R = _ref(gpu, orc, name)
    if "y" not in R:
        c, b = R["c"], R["rhs"]
        Bp, Bi, Bx = R["B"]
        solve_b, pinv = _oracle_solver(orc, c.n, Bp, Bi, Bx, R["q"], TOL)
        assert np.array_equal(pinv[R["q"]], np.arange(c.n))
        R["y"] = solve_b((R["dr"][:, None] * b)[R["rowperm"]])
        solve_bt, _ = _oracle_solver(orc, c.n, *_transposed(c.n, Bp, Bi, Bx), R["q"], TOL)
        R["z"] = solve_bt(R["dc"][:, None] * b)
        qa = orc.csc_amd_f(1, c.n, c.n, c.Ap, c.Ai)
        R["x"] = _oracle_solver(orc, c.n, c.Ap, c.Ai, c.Ax, qa, 1.0)[0](b)
        assert np.array_equal(R["x"][:, 0], orc.csc_lusol_f(1, c.n, c.Ap, c.Ai, c.Ax, b[:, 0], 1.0))
        Tp, Ti, Tx = _transposed(c.n, c.Ap, c.Ai, c.Ax)
        R["xt"] = _oracle_solver(orc, c.n, Tp, Ti, Tx, orc.csc_amd_f(1, c.n, c.n, Tp, Ti), 1.0)[0](b)
    return R


def _pattern_is_symmetric(n, Ap, Ai):
    P = csc_to_scipy(n, n, Ap, Ai, np.ones(len(Ai)))
    return (P != P.T).nnz == 0


def _assert_factors(n, B, got, want, what):
    """L and U against the oracle's: patterns bit-exact, values within RTOL norm-wise (helpers.assert_factor_equal).

    The library analyses the pattern of B + B' (DESIGN.md section 1), so on a structurally unsymmetric B -- the KKT cases
    after matching -- cs3_get_factors stores the positions of that structure which the unsymmetric elimination never
    fills as explicit zeros (kkt400: 27103 entries of L against the oracle's 20245).  There the comparison is made after
    dropping the entries that are exactly 0.0 from the library's arrays: what is left must be the oracle's pattern bit
    for bit.  On a structurally symmetric B (every scramble case) nothing may be dropped."""
    Lp, Li, Lx, Up, Ui, Ux = got
    if not _pattern_is_symmetric(n, B[0], B[1]):
        kept = []
        for Gp, Gi, Gx in ((Lp, Li, Lx), (Up, Ui, Ux)):
            G = csc_to_scipy(n, n, Gp, Gi, Gx).copy()
            G.eliminate_zeros()
            kept.append((G.indptr, G.indices, G.data))
        (Lp, Li, Lx), (Up, Ui, Ux) = kept
    el = assert_factor_equal(n, (Lp, Li, Lx), want[0:3], what + " L")
    eu = assert_factor_equal(n, (Up, Ui, Ux), want[3:6], what + " U")
    return el, eu


def _matched(gpu, c, **kw):
    return gpu.Factorization(c.n, c.n, c.Ap, c.Ai, batch=c.batch, match_values=c.Ax, **kw)


# 1. contrast: what a plain handle does with these matrices, and the matched one
@pytest.mark.parametrize("name", mc.SINGLE)
def test_plain_handle_rejects_what_the_matched_handle_factors(gpu, name):
    c = mc.case(name)
    _poison(gpu)
    with gpu.Factorization(c.n, c.n, c.Ap, c.Ai) as P:
        with pytest.raises(gpu.SingularMatrix):
            P.factor(c.Ax, TOL)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        assert F.info.fail_col == -1


# 2. factors of B
@pytest.mark.parametrize("name", mc.SINGLE)
def test_factors_are_the_oracles_factors_of_the_scaled_matrix(gpu, orc, name):
    R = _ref(gpu, orc, name)
    c = R["c"]
    _poison(gpu)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        FR = pc.fronts(gpu, F)
        Lp, Li, Lx, Up, Ui, Ux = F.factors()
    for cls in c.classes:
        assert cls in FR.cls
    oL = orc.csc_lu_f(c.n, c.n, *R["B"], R["q"], TOL)
    assert np.array_equal(oL[6][R["q"]], np.arange(c.n))
    assert _pattern_is_symmetric(c.n, *R["B"][:2]) == (not name.startswith("kkt"))
    el, eu = _assert_factors(c.n, R["B"], (Lp, Li, Lx, Up, Ui, Ux), oL, name)
    print("%s: L %.2e, U %.2e" % (name, el, eu))


# 3. solves, plain and transposed, few and many right-hand sides
@pytest.mark.parametrize("name", mc.SINGLE)
def test_solves_with_a_and_its_transpose(gpu, orc, name):
    R = _ref_solutions(gpu, orc, name)
    c, b = R["c"], R["rhs"]
    rowinv = np.argsort(R["rowperm"])
    _poison(gpu)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        for k in KS:
            bk = np.ascontiguousarray(b[:, :k])
            x = F.solve(bk).reshape(c.n, k)
            e_y = rel_err(x / R["dc"][:, None], R["y"][:, :k])
            e_x = rel_err(x, R["x"][:, :k])
            xt = F.solve(bk, trans=True).reshape(c.n, k)
            e_z = rel_err((xt / R["dr"][:, None])[R["rowperm"]], R["z"][:, :k])          # z[rowinv[i]] = x[i] / dr[i]
            e_xt = rel_err(xt, R["xt"][:, :k])
            print("%s k=%d: y %.2e, x %.2e, z %.2e, x' %.2e" % (name, k, e_y, e_x, e_z, e_xt))
            assert max(e_y, e_x, e_z, e_xt) <= RTOL
    assert np.array_equal(rowinv[R["rowperm"]], np.arange(c.n))


# 4. the fused step equals factor + solve, bit for bit, also from the graph that holds the closing permutation
@pytest.mark.parametrize("name", mc.SINGLE)
def test_fused_step_equals_factor_then_solve(gpu, orc, name):
    import torch
    R = _ref(gpu, orc, name)
    c = R["c"]
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    ax = torch.from_numpy(c.Ax).to(dev)
    _poison(gpu)
    with _matched(gpu, c) as F:
        for k in (1, 16):
            B = np.ascontiguousarray(R["rhs"][:, :k])
            want = torch.from_numpy(B.copy()).to(dev)
            F.factor_dev(ax.data_ptr(), TOL, sh)
            F.solve_dev(want.data_ptr(), k, sh)
            F.factor_status(sh)
            want = want.cpu().numpy()
            x = torch.empty((c.n, k), dtype=torch.float64, device=dev)
            bsrc = torch.from_numpy(B).to(dev)
            for rep in range(4):                                       # the third call in a row with this X takes its own graph
                x.copy_(torch.from_numpy(B))
                F.factor_solve_dev(ax.data_ptr(), x.data_ptr(), k, TOL, sh)
                F.factor_status(sh)
                assert np.array_equal(x.cpu().numpy(), want), "%s k=%d in place, call %d" % (name, k, rep)
            x2 = torch.zeros_like(x)
            for rep in range(4):
                F.factor_solve_bx_dev(ax.data_ptr(), bsrc.data_ptr(), x2.data_ptr(), k, TOL, sh)
                F.factor_status(sh)
                assert np.array_equal(x2.cpu().numpy(), want), "%s k=%d out of place, call %d" % (name, k, rep)
            assert np.array_equal(bsrc.cpu().numpy(), B) and np.array_equal(ax.cpu().numpy(), c.Ax)


# 5. refactorisation keeps the matching
@pytest.mark.parametrize("name", mc.SINGLE)
def test_refactorisation_with_new_values_keeps_the_matching(gpu, orc, name):
    R = _ref(gpu, orc, name)
    c = R["c"]
    Ax2 = c.Ax * (1.0 + 0.05 * np.random.default_rng(19).uniform(-1.0, 1.0, len(c.Ax)))
    B2 = mc.scaled(c, Ax2, R["rowperm"], R["dr"], R["dc"])
    assert pc.first_off_diagonal(orc, c.n, *B2, R["q"], TOL) is None
    oL = orc.csc_lu_f(c.n, c.n, *B2, R["q"], TOL)
    b = R["rhs"][:, 0].copy()
    solve_b, _ = _oracle_solver(orc, c.n, *B2, R["q"], TOL)
    y = solve_b((R["dr"] * b)[R["rowperm"]])[:, 0]
    _poison(gpu)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        F.solve(b)
        F.factor(Ax2, TOL)
        for got, want in zip(F.matching(), (R["rowperm"], R["dr"], R["dc"])):
            assert np.array_equal(got, want)
        Lp, Li, Lx, Up, Ui, Ux = F.factors()
        x = F.solve(b)
    _assert_factors(c.n, B2, (Lp, Li, Lx, Up, Ui, Ux), oL, name)
    assert rel_err(x / R["dc"], y) <= RTOL


# 6. the other paths stay in terms of A
def _dense(c):
    return csc_to_scipy(c.n, c.n, c.Ap, c.Ai, c.Ax).toarray()


@pytest.mark.parametrize("name", ["kkt400", "jac200"])
def test_residual_and_refinement_are_in_terms_of_a(gpu, orc, name):
    import torch
    R = _ref_solutions(gpu, orc, name)
    c = R["c"]
    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream().cuda_stream
    k = 3
    B = np.ascontiguousarray(R["rhs"][:, :k])
    ax, b = torch.from_numpy(c.Ax).to(dev), torch.from_numpy(B).to(dev)
    _poison(gpu)
    with _matched(gpu, c) as F, gpu.Factorization(c.n, c.n, c.Ap, c.Ai) as P:
        F.factor_dev(ax.data_ptr(), TOL, sh)
        x = b.clone()
        F.solve_dev(x.data_ptr(), k, sh)
        F.factor_status(sh)
        r, rp = torch.empty_like(b), torch.empty_like(b)
        for trans in (False, True):
            F.residual_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), r.data_ptr(), k, sh, trans=trans)
            P.residual_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), rp.data_ptr(), k, sh, trans=trans)   # (needs no factors)
            torch.cuda.synchronize()
            assert np.array_equal(r.cpu().numpy(), rp.cpu().numpy())
        X = x.cpu().numpy()
        want = np.stack([B[:, j] - orc.csc_mat_vec_ff(c.n, c.n, c.Ap, c.Ai, c.Ax, np.ascontiguousarray(X[:, j])) for j in range(k)], axis=1)
        F.residual_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), r.data_ptr(), k, sh)
        torch.cuda.synchronize()
        assert np.array_equal(r.cpu().numpy(), want)
        for trans in (False, True):
            x0 = torch.from_numpy(F.solve(B, trans=trans).reshape(c.n, k) * (1.0 + 1e-6 * np.cos(np.arange(c.n)))[:, None]).to(dev)
            c1 = F.refine_dev(ax.data_ptr(), b.data_ptr(), x0.data_ptr(), k, 1, sh, trans=trans)
            c2 = F.refine_dev(ax.data_ptr(), b.data_ptr(), x0.data_ptr(), k, 1, sh, trans=trans)
            print("%s trans=%d: corrections %.3e -> %.3e" % (name, trans, c1, c2))
            assert 0.0 < c1 and c2 < 1e-3 * c1
            assert rel_err(x0.cpu().numpy(), R["xt" if trans else "x"][:, :k]) <= RTOL


@pytest.mark.parametrize("name", ["kkt400", "jac200"])
def test_condest_and_slogdet_are_of_a(gpu, orc, name):
    import torch
    R = _ref(gpu, orc, name)
    c = R["c"]
    A = _dense(c)
    exact = np.abs(A).sum(axis=0).max() * np.abs(np.linalg.inv(A)).sum(axis=0).max()
    sign_w, logabs_w = np.linalg.slogdet(A)
    _poison(gpu)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        cond, inv = F.condest(c.Ax)
        sign, logabs = F.slogdet()
        dev = torch.device("cuda", 0)
        out = torch.zeros(2, dtype=torch.float64, device=dev)
        F.slogdet_dev(out.data_ptr(), out.data_ptr() + 8, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), [sign[0], logabs[0]])
    print("%s: condest %.6e, dense %.6e; slogdet (%g, %.15g), dense (%g, %.15g)" % (name, cond[0], exact, sign[0], logabs[0], sign_w, logabs_w))
    assert cond[0] == gpu.csc_norm(c.n, c.Ap, c.Ax) * inv[0]
    assert exact / 3.0 <= cond[0] <= exact * (1.0 + 1e-10)
    assert sign[0] == sign_w and abs(logabs[0] - logabs_w) <= 1e-10 * max(1.0, abs(logabs_w))


@pytest.mark.parametrize("name", ["kkt400", "jac200"])
def test_low_rank_modified_solves_and_export(gpu, orc, name):
    import torch
    R = _ref(gpu, orc, name)
    c = R["c"]
    A = _dense(c)
    b = R["rhs"][:, 0].copy()
    col = np.repeat(np.arange(c.n), np.diff(c.Ap))
    pick = np.random.default_rng(23).choice(np.flatnonzero(c.Ax != 0.0), size=5, replace=False)
    # rank 1, rank 2, rank 2: existing entries changed by 30 %
    cases = [(c.Ai[pick[:1]], col[pick[:1]], 0.3 * c.Ax[pick[:1]]), (c.Ai[pick[1:3]], col[pick[1:3]], 0.3 * c.Ax[pick[1:3]]),
             (c.Ai[pick[3:5]], col[pick[3:5]], -0.3 * c.Ax[pick[3:5]])]
    _poison(gpu)
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        with F.updates_plan([(i, j) for i, j, _ in cases]) as plan:
            X, rpiv = F.solve_updates(plan, np.concatenate([v for _, _, v in cases]), b)
        buf = torch.empty(int(F.info.factor_bytes) // 8 + 1, dtype=torch.float64, device=torch.device("cuda", 0))
        for fn in (F.export_factor_dev, F.import_factor_dev):
            with pytest.raises(gpu.Cs3Error) as e:
                fn(buf.data_ptr())
            assert e.value.code == gpu.CS3_ERR_ARG
        x_after = F.solve(b)
    for k, (i, j, v) in enumerate(cases):
        M = A.copy()
        np.add.at(M, (i, j), v)
        err = rel_err(X[:, k], np.linalg.solve(M, b))
        print("%s case %d: %.2e (rpiv %.2e)" % (name, k, err, rpiv[k]))
        assert err <= 1e-9
    assert rel_err(x_after, np.linalg.solve(A, b)) <= 1e-9


# 7. a batch shares one matching
def test_batch_of_twenty_shares_the_matching(gpu, orc):
    R = _ref(gpu, orc, "db48x20")
    c = R["c"]
    AX = mc.batch_values(c)
    b = np.random.default_rng(29).standard_normal((c.batch, c.n))
    _poison(gpu)
    with _matched(gpu, c) as F:
        FR = pc.fronts(gpu, F)
        for cls in c.classes:
            assert cls in FR.cls
        F.factor(AX, TOL)
        X = F.solve(b)
        XT = F.solve(b, trans=True)
        factors = [F.factors(m) for m in (0, c.batch - 1)]
    for m in range(c.batch):
        Bm = mc.scaled(c, AX[m], R["rowperm"], R["dr"], R["dc"])
        solve_b, pinv = _oracle_solver(orc, c.n, *Bm, R["q"], TOL)
        assert np.array_equal(pinv[R["q"]], np.arange(c.n))
        y = solve_b((R["dr"] * b[m])[R["rowperm"]])[:, 0]
        assert rel_err(X[m] / R["dc"], y) <= RTOL, m
        zt = _oracle_solver(orc, c.n, *_transposed(c.n, *Bm), R["q"], TOL)[0](R["dc"] * b[m])[:, 0]
        assert rel_err((XT[m] / R["dr"])[R["rowperm"]], zt) <= RTOL, m
    for m, (Lp, Li, Lx, Up, Ui, Ux) in zip((0, c.batch - 1), factors):
        oL = orc.csc_lu_f(c.n, c.n, *mc.scaled(c, AX[m], R["rowperm"], R["dr"], R["dc"]), R["q"], TOL)
        _assert_factors(c.n, R["B"], (Lp, Li, Lx, Up, Ui, Ux), oL, "matrix %d" % m)


# 8. lifetime
def test_matched_handle_frees_every_device_block(gpu, orc):
    gc.collect()
    before = gpu.debug_live_device_buffers()
    c = mc.case("kkt400")
    b = np.random.default_rng(31).standard_normal((c.n, 64))
    _poison(gpu)
    F = _matched(gpu, c)
    F.factor(c.Ax, TOL)
    F.solve(b[:, 0].copy())
    F.solve(b, trans=True)
    F.condest(c.Ax)
    F.slogdet()
    F.factors()
    with F.updates_plan([([0], [0])]) as plan:
        F.solve_updates(plan, [0.1 * c.Ax[0]], b[:, 0].copy())
    assert gpu.debug_live_device_buffers() > before
    F.close()
    assert gpu.debug_live_device_buffers() == before


# 9. a plain handle does what it did, whatever matched handles the process has used
def test_plain_path_keeps_its_bits_beside_matched_handles(gpu, orc):
    m, n, Ap, Ai, Ax = synth.grid_jacobian(3000, seed=13)
    b = np.random.default_rng(37).standard_normal((n, 16))

    def plain():
        with gpu.Factorization(m, n, Ap, Ai) as P:
            P.factor(Ax, TOL)
            return P.solve(b[:, 0].copy()), P.solve(b), P.solve(b, trans=True), P.slogdet(), P.factors()

    _poison(gpu)
    first = plain()
    with gpu.Factorization(m, n, Ap, Ai, match_values=Ax) as F:             # the same matrix through a matched handle
        F.factor(Ax, TOL)
        xm = F.solve(b)
        assert np.array_equal(F.matching()[0], np.arange(n))
    c = mc.case("kkt400")
    with _matched(gpu, c) as F:
        F.factor(c.Ax, TOL)
        F.solve(np.ones(c.n))
    second = plain()
    for a, s in zip(first[:3], second[:3]):
        assert np.array_equal(a, s)
    assert np.array_equal(first[3], second[3])
    for a, s in zip(first[4], second[4]):
        assert np.array_equal(a, s)
    assert rel_err(xm, first[1]) <= RTOL


# 10. the matrix class
def test_cscmat_lu_and_lusol_with_match(gpu, orc):
    from csparse3_amd.csc import CscMat, lusol
    R = _ref_solutions(gpu, orc, "kkt400")
    c = R["c"]
    A = CscMat(c.n, c.n, indptr=c.Ap, indices=c.Ai, data=c.Ax.copy())
    b = R["rhs"][:, 0].copy()
    _poison(gpu)
    with pytest.raises(gpu.SingularMatrix):
        A.lu(tol=TOL)
    x = A.lu(tol=TOL, match=True).solve(b)
    assert rel_err(x, R["x"][:, 0]) <= RTOL
    assert np.array_equal(A.solve(b, tol=TOL, match=True), x)
    assert rel_err(A.solve(b, tol=TOL, trans=True, match=True), R["xt"][:, 0]) <= RTOL
    assert np.array_equal(lusol(A, b, tol=TOL, match=True), x)
    with pytest.raises(gpu.SingularMatrix):
        lusol(A, b, tol=TOL)
    A._factorization[1].close()
