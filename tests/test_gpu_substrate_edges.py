"""The conversion / assembly kernels (substrate.hip) and the Newton-chain glue of kernels.hip at their bucket, tile and
grid edges: the cases of tests/substrate_cases.py (whose claims and oracle tests/test_substrate_cases_cpu.py proves),
bit for bit against the reference's own recorded outputs (tests/golden/substrate_edges.npz) where the reference ran,
and against the CPU oracle / the NumPy restatements otherwise."""
import numpy as np
import pytest

import substrate_cases as sc

pytestmark = pytest.mark.gpu
G = sc.gold()


def gold_csc(tag, names=("p", "i", "x")):
    return tuple(G["%s__%s" % (tag, k)] for k in names)


def to_csr(gpu, m, n, Ap, Ai, Ax):
    Bp = np.zeros(m + 1, dtype=np.int32); Bi = np.empty(len(Ai), dtype=np.int32); Bx = np.empty(len(Ai))
    gpu.csc_to_csr(m, n, Ap, Ai, Ax, Bp, Bi, Bx)
    return Bp, Bi, Bx


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                    # noqa: E731
    return torch, dev, T


# ---- 1. bucket lengths ------------------------------------------------------------------------------------------------

def test_bucket_lengths_transpose_and_csr(gpu):
    """Rows of 0 ... 33 (insertion sort), 64, 65, 1000 and 3001 entries (heap sort), duplicates in storage order."""
    m, n, Ap, Ai, Ax, _ = sc.bucket_lengths()
    tn, tm, Tp, Ti, Tx = gpu.csc_transpose(m, n, Ap, Ai, Ax)
    assert (tn, tm) == (n, m) and sc.same_csc((Tp, Ti, Tx), gold_csc("bucket", ("t_p", "t_i", "t_x")))
    assert sc.same_csc(to_csr(gpu, m, n, Ap, Ai, Ax), gold_csc("bucket", ("csr_p", "csr_i", "csr_x")))


def test_bucket_lengths_coo_to_csc(gpu):
    m, n, Ti, Tj, Tx, _ = sc.bucket_triplets()
    assert sc.same_csc(gpu.coo_to_csc(m, n, Ti, Tj, Tx, len(Ti))[2:], gold_csc("bucket_coo"))


# ---- 2. scan tiles -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", sc.SCAN_BUCKETS)
def test_scan_tiles(gpu, nb):
    m, n, Ap, Ai, Ax, _ = sc.scan_tiles(nb)
    assert sc.same_csc(gpu.csc_transpose(m, n, Ap, Ai, Ax)[2:], gold_csc("scan%d" % nb, ("t_p", "t_i", "t_x")))
    assert sc.same_csc(to_csr(gpu, m, n, Ap, Ai, Ax), gold_csc("scan%d" % nb, ("csr_p", "csr_i", "csr_x")))
    assert sc.same_csc(gpu.coo_to_csc(n, m, sc.columns_of(Ap), Ai, Ax, len(Ai))[2:], gold_csc("scan%d_coo" % nb))


def test_scan_of_no_buckets_and_no_entries(gpu):
    z = np.zeros(0, dtype=np.int32)
    for tag, m, n in (("m0", 0, 4), ("n0", 4, 0)):
        assert sc.same_csc(gpu.csc_transpose(m, n, np.zeros(n + 1, dtype=np.int32), z, np.zeros(0))[2:], gold_csc(tag, ("t_p", "t_i", "t_x")))
        # (the reference's coo_to_csc cannot run on nothing: the restatement)
        assert sc.same_csc(gpu.coo_to_csc(m, n, z, z, np.zeros(0), 0)[2:], sc.coo_restated(n, z, z, np.zeros(0)))


# ---- 3. one grid pass plus one ----------------------------------------------------------------------------------------

def test_one_pass_plus_one_entries_transpose(gpu, orc):
    m, n, Ap, Ai, Ax, _ = sc.pass_plus_one_entries()
    got = gpu.csc_transpose(m, n, Ap, Ai, Ax)[2:]
    assert sc.same_csc(got, orc.csc_transpose(m, n, Ap, Ai, Ax)[2:])
    assert got[0][m] - got[0][m - 1] == 1 and got[2][-1] == Ax[-1]                     # the last work item's bucket


def test_one_pass_plus_one_entries_coo(gpu, orc):
    m, n, Ap, Ai, Ax, _ = sc.pass_plus_one_entries()
    cols = sc.columns_of(Ap)
    perm = np.random.default_rng(3).permutation(len(Ai))
    perm[np.argmax(perm)], perm[-1] = perm[-1], len(Ai) - 1                            # the only entry of the last column stays last
    Ti, Tj, Tx = cols[perm], Ai[perm], Ax[perm]
    got = gpu.coo_to_csc(n, m, Ti, Tj, Tx, len(Ti))[2:]
    assert sc.same_csc(got, orc.coo_to_csc(n, m, Ti, Tj, Tx, len(Ti))[2:]) and got[2][-1] == Ax[-1]


def test_one_pass_plus_one_columns_transpose_and_norm(gpu, orc):
    """The last bucket of the transpose (row n - 1) fills out of order and is sorted by the last work item of
    k_bucket_sort; the last column has the largest sum."""
    n, Ap, Ai, Ax, c = sc.pass_plus_one_columns()
    got = gpu.csc_transpose(n, n, Ap, Ai, Ax)[2:]
    assert sc.same_csc(got, orc.csc_transpose(n, n, Ap, Ai, Ax)[2:])
    assert np.array_equal(got[1][got[0][n - 1]:got[0][n]], c["hub"])                   # ascending columns in the last bucket
    assert sc.same_bits(gpu.csc_norm(n, Ap, Ax), orc.csc_norm(n, Ap, Ax)) and gpu.csc_norm(n, Ap, Ax) == c["largest_sum"]


def test_one_pass_plus_one_columns_islands(gpu):
    """The last node joins seven chains through interior nodes: k_label_jump's last work item compresses its label."""
    n, Ap, Ai, Ax, c = sc.pass_plus_one_columns()
    got = gpu.find_islands(n, Ap, Ai)
    want = sc.islands_from_labels(c["label"])                                          # (proved in test_substrate_cases_cpu.py)
    assert sc.same_islands(got, want) and len(got) == c["islands"] and got[0][-1] == n - 1


@pytest.mark.parametrize("kind", ["no way in", "one way in"])
def test_one_pass_plus_one_columns_directed_islands(gpu, kind):
    """Every entry without a mirror in the last column, the last work item of k_pattern_symmetric; "no way in": the
    last node an island of its own (a symmetric treatment merges eight); "one way in": six chains entered from node 0
    only through the last work item of k_reach_hook."""
    n, Ap, Ai, c = sc.pass_plus_one_directed(kind)
    got = gpu.find_islands(n, Ap, Ai)
    assert sc.same_islands(got, sc.islands_from_labels(c["label"])) and len(got) == c["islands"]
    assert (got[-1].tolist() == [n - 1]) if kind == "no way in" else (got[0][-1] == n - 1)


def test_one_pass_plus_one_add(gpu, orc):
    m, n, A, B, alpha, beta, c = sc.pass_plus_one_add()
    got = gpu.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)[2:]
    assert sc.same_csc(got, orc.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)[2:]) and got[0][n] == c["nnz_c"]


def test_one_pass_plus_one_sub_matrix(gpu, orc):
    Am, Ap, Ai, Ax, rows, cols, c = sc.pass_plus_one_sub()
    got = gpu.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
    want = orc.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
    assert got[0] == want[0] == 1 and sc.same_csc(got[1:], want[1:]) and list(got[2]) == [1]


# ---- 4. csc_add_ff ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["columns", "A empty", "B empty", "both empty"])
def test_add_cases(gpu, name):
    """Shared, disjoint and duplicated rows, 300 entries a side, +0.0 / -0.0 results, Inf and NaN, empty sides."""
    m, n, A, B, alpha, beta, _ = sc.add_cases()[name]
    cm, cn, Cp, Ci, Cx = gpu.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)
    assert (cm, cn) == (m, n) and sc.same_csc((Cp, Ci, Cx), gold_csc("add_" + name.replace(" ", "_")))


# ---- 5. csc_sub_matrix ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", sc.SUB_ROW_COUNTS)
def test_sub_matrix_selections(gpu, nrows):
    Am, Ap, Ai, Ax, _ = sc.sub_matrix_source()
    rows, cols = sc.sub_selection(nrows, Ap, Ai)
    nz, Bp, Bi, Bx = gpu.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
    assert nz == int(G["sub%d__nz" % nrows]) and sc.same_csc((Bp, Bi, Bx), gold_csc("sub%d" % nrows))


def test_sub_matrix_of_no_columns(gpu):
    Am, Ap, Ai, Ax, _ = sc.sub_matrix_source()
    nz, Bp, Bi, Bx = gpu.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, np.array([sc.SUB_R0, 5], dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert nz == 0 and np.array_equal(Bp, G["sub_ncols0__p"]) and len(Bi) == len(Bx) == 0


# ---- 6. csc_norm ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.norm_cases()))
def test_norm_cases(gpu, name):
    n, Ap, Ax, _ = sc.norm_cases()[name]
    assert sc.same_bits(gpu.csc_norm(n, Ap, Ax), float(G["norm_" + name.replace(" ", "_")]))


# ---- 7. find_islands -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.island_cases()))
def test_island_cases(gpu, name):
    n, Ap, Ai, _ = sc.island_cases()[name]
    tag = "isl_" + name.replace(" ", "_")
    want = np.split(G[tag + "__flat"], np.cumsum(G[tag + "__sizes"])[:-1])
    assert sc.same_islands(gpu.find_islands(n, Ap, Ai), want)


# ---- 8. stacking ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.stack_cases()))
def test_stack_cases(gpu, torch_dev, name):
    """Host-pointer and device-pointer stacking against the reference's output; the restack map against its restatement,
    at the four seams in particular; restacking new values through the map."""
    torch, dev, T = torch_dev
    blocks, _ = sc.stack_cases()[name]
    tag = "stack_" + name.replace(" ", "_")
    want = gold_csc(tag)
    m, n, Pi, Pp, Px = gpu.csc_stack_4_by_4_ff(*[v for b in blocks for v in b])
    assert (m, n) == (int(G[tag + "__m"]), int(G[tag + "__n"])) and sc.same_csc((Pp, Pi, Px), want)
    sh = torch.cuda.current_stream().cuda_stream
    dblk = [(m_, n_, len(x_), T(i_), T(p_), T(x_)) for (m_, n_, i_, p_, x_) in blocks]
    nnz = sum(b[2] for b in dblk)
    dPi = torch.full((nnz,), -7, dtype=torch.int32, device=dev); dPp = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    dPx = torch.full((nnz,), -7.0, dtype=torch.float64, device=dev); dmap = torch.full((nnz,), -7, dtype=torch.int32, device=dev)
    gpu.csc_stack_4_by_4_dev([(m_, n_, z_, i_.data_ptr(), p_.data_ptr(), x_.data_ptr()) for (m_, n_, z_, i_, p_, x_) in dblk],
                             dPi.data_ptr(), dPp.data_ptr(), dPx.data_ptr(), dmap.data_ptr(), sh)
    torch.cuda.synchronize()
    assert sc.same_csc((dPp.cpu().numpy(), dPi.cpu().numpy(), dPx.cpu().numpy()), want)
    mp = dmap.cpu().numpy()
    want_map = sc.stack_restated(blocks)[5]
    assert np.array_equal(mp, want_map)
    sizes = [b[2] for b in dblk]
    # the seams of A | B | C | D stated on their own, from the reference's column pointers: where the first and the last
    # entry of every block land in the output (upper blocks open a column, lower blocks close it), the map holds the
    # block's offset and the offset of its last entry
    an = blocks[0][1]
    offs = np.cumsum([0] + sizes)
    for b, (shift, lower) in enumerate(((0, False), (an, False), (0, True), (an, True))):
        if sizes[b]:
            bp = blocks[b][3]
            upper_len = np.diff(blocks[b - 2][3]) if lower else None
            filled = np.flatnonzero(np.diff(bp))
            j0, j1 = filled[0], filled[-1]
            first = want[0][shift + j0] + (upper_len[j0] if lower else 0)
            last = want[0][shift + j1 + 1] - 1 if lower else want[0][shift + j1] + (bp[j1 + 1] - bp[j1]) - 1
            assert mp[first] == offs[b] and mp[last] == offs[b + 1] - 1, (name, "ABCD"[b])
    new = [np.random.default_rng(9).standard_normal(s) for s in sizes]
    dnew = [T(v) for v in new]
    gpu.restack_values_dev(nnz, dmap.data_ptr(), sizes[0], sizes[1], sizes[2], *[v.data_ptr() for v in dnew], dPx.data_ptr(), sh)
    torch.cuda.synchronize()
    assert sc.same_bits(dPx.cpu().numpy(), np.concatenate(new)[want_map])


def test_restack_values_past_one_grid_pass(gpu, torch_dev):
    torch, dev, T = torch_dev
    mp, parts, c = sc.restack_pass_plus_one()
    sh = torch.cuda.current_stream().cuda_stream
    dmap, dparts = T(mp), [T(p) for p in parts]
    dPx = torch.full((c["nnz"],), -7.0, dtype=torch.float64, device=dev)
    gpu.restack_values_dev(c["nnz"], dmap.data_ptr(), len(parts[0]), len(parts[1]), len(parts[2]), *[p.data_ptr() for p in dparts],
                           dPx.data_ptr(), sh)
    torch.cuda.synchronize()
    got = dPx.cpu().numpy()
    assert sc.same_bits(got, np.concatenate(parts)[mp]) and got[-1] == parts[3][-1]


# ---- 9. general triangular solves -------------------------------------------------------------------------------------------

def _tri_check(gpu, orc, n, L, U):
    """Every solve with k = 1 and 3: within 4 x the oracle's own error of the longdouble solution (the butterfly sum is
    another valid order of the same additions), and the same bits when run again."""
    refs = sc.tri_references(orc, n, L, U)
    for name, lower, trans in sc.TRI_SOLVES:
        Gp, Gi, Gx = L if lower else U
        for k in (1, 3):
            B, X, oracle_err = refs[(name, k)]
            x1 = np.ascontiguousarray(B).copy(); x2 = x1.copy()
            getattr(gpu, "csc_%s_f" % name)(n, Gp, Gi, Gx, x1)
            getattr(gpu, "csc_%s_f" % name)(n, Gp, Gi, Gx, x2)
            err = float(np.abs(x1 - X).max() / np.abs(X).max())
            print("%s k=%d n=%d: device error %.3e, oracle error %.3e" % (name, k, n, err, oracle_err))
            assert err <= 4.0 * oracle_err, (name, k, err, oracle_err)
            assert sc.same_bits(x1, x2), (name, k)


def test_tri_rows_of_0_1_63_64_65_200(gpu, orc):
    n, L, U, _ = sc.tri_edges()
    _tri_check(gpu, orc, n, L, U)


@pytest.mark.parametrize("name", ["n=1", "diagonal", "chain"])
def test_tri_small_cases(gpu, orc, name):
    n, L, U, _ = sc.tri_small_cases()[name]
    _tri_check(gpu, orc, n, L, U)


# ---- 10. resident matvec / residual / refine ------------------------------------------------------------------------------

@pytest.mark.parametrize("trans", [False, True])
def test_resident_matvec_and_residual_past_the_grid_caps(gpu, torch_dev, trans):
    """n = 65 537 with 17 right-hand sides: n k exceeds one pass of both kernels; rows of 0 and of 200 entries."""
    torch, dev, T = torch_dev
    n, Ap, Ai, Ax, c = sc.resident_matrix()
    k = sc.RESIDENT_K
    rng = np.random.default_rng(8)
    X, B = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    want = sc.matvec_restated(n, Ap, Ai, Ax, X, trans)
    sh = torch.cuda.current_stream().cuda_stream
    with gpu.Factorization(n, n, Ap, Ai) as F:
        d_ax, d_x, d_b = T(Ax), T(X), T(B)
        d_y = torch.full((n, k), -7.0, dtype=torch.float64, device=dev); d_r = d_y.clone()
        F.matvec_dev(d_ax.data_ptr(), d_x.data_ptr(), d_y.data_ptr(), k, sh, trans=trans)
        F.residual_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), k, sh, trans=trans)
        torch.cuda.synchronize()
        Y, R = d_y.cpu().numpy(), d_r.cpu().numpy()
    assert sc.same_bits(Y, want) and sc.same_bits(R, B - want)
    assert np.all(Y[c["empty_row"]] == 0.0) and np.all(Y[c["long_row"]] != 0.0)


@pytest.mark.parametrize("trans", [False, True])
def test_refine_correction_norm_and_nan(gpu, torch_dev, trans):
    """refine_dev returns max |d| of the correction d = A \\ (b - A x), bit for bit what residual_dev and a solve on the
    same handle give, with the largest |d| in the last element of the last right-hand side; a NaN in one right-hand side
    makes the norm NaN and leaves every other right-hand side as it is without the NaN."""
    torch, dev, T = torch_dev
    n, Ap, Ai, Ax, _ = sc.resident_matrix(empty_row=False)
    k = sc.RESIDENT_K
    rng = np.random.default_rng(10)
    B = rng.standard_normal((n, k))
    sh = torch.cuda.current_stream().cuda_stream
    with gpu.Factorization(n, n, Ap, Ai) as F:
        F.factor(Ax)
        X0 = F.solve(B, trans=trans)
        X0[-1, -1] += 0.125                                                            # the only large correction: -0.125 there
        d_ax, d_b, d_x, d_r = T(Ax), T(B), T(X0), T(np.zeros((n, k)))
        F.residual_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), k, sh, trans=trans)
        F.solve_dev(d_r.data_ptr(), k, sh, trans=trans)
        torch.cuda.synchronize()
        D = d_r.cpu().numpy()
        assert np.unravel_index(np.argmax(np.abs(D)), D.shape) == (n - 1, k - 1) and abs(D[-1, -1] + 0.125) < 1e-12
        corr = F.refine_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), k, 1, sh, trans=trans)
        X1 = d_x.cpu().numpy()
        assert sc.same_bits(corr, np.abs(D).max()) and sc.same_bits(X1, X0 + D)
        # one NaN, in the right-hand side of column 5
        Bn = B.copy(); Bn[n // 2, 5] = np.nan
        d_bn, d_xn = T(Bn), T(X0)
        corr = F.refine_dev(d_ax.data_ptr(), d_bn.data_ptr(), d_xn.data_ptr(), k, 1, sh, trans=trans)
        Xn = d_xn.cpu().numpy()
    assert np.isnan(corr)
    others = [t for t in range(k) if t != 5]
    assert sc.same_bits(Xn[:, others], X1[:, others]) and np.isnan(Xn[:, 5]).any() and np.isnan(Xn[n // 2, 5])


# ---- error paths ----------------------------------------------------------------------------------------------------------

def test_out_of_range_index_in_the_last_work_item(gpu):
    m, n, Ap, Ai, Ax, _ = sc.pass_plus_one_entries()
    bad = Ai.copy(); bad[-1] = m
    with pytest.raises(gpu.Cs3Error) as e:
        gpu.csc_transpose(m, n, Ap, bad, Ax)
    assert "out of range" in str(e.value)
    cols = sc.columns_of(Ap).copy(); cols[-1] = n
    with pytest.raises(gpu.Cs3Error) as e:
        gpu.coo_to_csc(m, n, Ai, cols, Ax, len(Ai))
    assert "out of range" in str(e.value)


def test_sub_matrix_over_capacity_past_one_grid_pass(gpu):
    Am, Ap, Ai, Ax, rows, cols, c = sc.sub_over_capacity()
    with pytest.raises(gpu.Cs3Error) as e:
        gpu.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
    assert "result has %d entries, room for %d" % (c["result"], c["room"]) in str(e.value)
