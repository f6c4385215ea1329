"""The engineered inputs of tests/substrate_cases.py deliver what they claim (proved from NumPy alone), and the CPU oracle
is pinned at these edges: against the outputs of the reference's own kernels recorded in tests/golden/substrate_edges.npz
and, for the sizes the reference was not run at, against oracle-independent restatements.  No GPU."""
import os
import zlib

import numpy as np
import pytest

import substrate_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = sc.gold()


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def gold_csc(tag, names=("p", "i", "x")):
    return tuple(G["%s__%s" % (tag, k)] for k in names)


def test_constants_are_the_ones_in_the_kernels():
    cache = {}
    for name, value, fname, line, text in sc.SOURCE_LINES:
        lines = cache.setdefault(fname, open(os.path.join(ROOT, "csparse3_amd", "csrc", fname)).read().split("\n"))
        assert text in lines[line - 1], "%s = %d: %s:%d no longer reads %r" % (name, value, fname, line, text)
        assert str(value) in text or name == "SUB_COLS_PER_PASS"
    assert sc.SUB_COLS_PER_PASS == 16384 and sc.ONE_PASS == 1048576


def test_the_reference_ran_every_recorded_case():
    assert sorted(G["skipped"]) == ["m0_coo: IndexError", "n0_coo: IndexError"]       # coo_to_csc of nothing: Ti[0] of an empty array


# ---- 1. bucket lengths ------------------------------------------------------------------------------------------------

def test_bucket_lengths_claims_and_oracle(orc):
    m, n, Ap, Ai, Ax, c = sc.bucket_lengths()
    lens = np.bincount(Ai, minlength=m)
    assert list(lens) == c["row_lengths"] and lens.max() == c["max_bucket"] == n
    assert set(sc.BUCKET_ROW_LENGTHS) <= set(lens) and sc.SORT_INSERTION_MAX in lens and sc.SORT_INSERTION_MAX + 1 in lens
    cols = sc.columns_of(Ap)
    for row, key, times in ((c["twice_row"], "twice_cols", 2), (c["thrice_row"], "thrice_cols", 3)):
        per_col = np.bincount(cols[Ai == row], minlength=n)
        assert np.all(per_col[c[key]] >= times) and lens[row] > sc.SORT_INSERTION_MAX
    assert any(np.any(np.diff(Ai[Ap[j]:Ap[j + 1]]) < 0) for j in range(n))             # unsorted rows inside columns
    assert len(np.unique(Ax)) == len(Ax)                                               # every misplacement shows
    assert crc(Ap, Ai, Ax) == int(G["bucket__in"])
    got = orc.csc_transpose(m, n, Ap, Ai, Ax)[2:]
    assert sc.same_csc(got, gold_csc("bucket", ("t_p", "t_i", "t_x"))) and sc.same_csc(got, sc.transpose_restated(m, n, Ap, Ai, Ax))
    Bp = np.zeros(m + 1, dtype=np.int32); Bi = np.empty(len(Ai), dtype=np.int32); Bx = np.empty(len(Ai))
    orc.csc_to_csr(m, n, Ap, Ai, Ax, Bp, Bi, Bx)
    assert sc.same_csc((Bp, Bi, Bx), gold_csc("bucket", ("csr_p", "csr_i", "csr_x")))
    # duplicates of a row come out in storage order: their source positions ascend
    Tp, Ti, Tx = got
    pos = {v: k for k, v in enumerate(Ax)}
    for row in (c["twice_row"], c["thrice_row"]):
        src = [pos[v] for v in Tx[Tp[row]:Tp[row + 1]]]
        assert src == sorted(src)


def test_bucket_triplets_claims_and_oracle(orc):
    m, n, Ti, Tj, Tx, c = sc.bucket_triplets()
    lens = np.bincount(Tj, minlength=n)
    assert list(lens) == c["col_lengths"] and {0, 32, 33, 1000} <= set(lens)
    assert np.any(np.diff(Tj) < 0) and crc(Ti, Tj, Tx) == int(G["bucket_coo__in"])
    got = orc.coo_to_csc(m, n, Ti, Tj, Tx, len(Ti))[2:]
    assert sc.same_csc(got, gold_csc("bucket_coo")) and sc.same_csc(got, sc.coo_restated(n, Ti, Tj, Tx))


# ---- 2. scan tiles -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", sc.SCAN_BUCKETS)
def test_scan_tiles_claims_and_oracle(orc, nb):
    m, n, Ap, Ai, Ax, c = sc.scan_tiles(nb)
    cnt = np.bincount(Ai, minlength=m)
    assert m == nb and c["tiles"] == -(-nb // sc.SCAN_TILE) == len(c["tile_sums"])
    assert all(s > 0 for s in c["tile_sums"]) and c["tile_sums"] == [int(cnt[t:t + sc.SCAN_TILE].sum()) for t in range(0, nb, sc.SCAN_TILE)]
    assert len(c["carry_at_edges"]) == c["tiles"] - 1 and all(v > 0 for v in c["carry_at_edges"])
    assert list(np.diff([0] + c["carry_at_edges"])) == c["tile_sums"][:-1]            # the carry changes at every edge
    for e in range(sc.SCAN_TILE, nb, sc.SCAN_TILE):
        assert cnt[e - 1] > 0 and cnt[e] > 0                                           # both sides of an edge hold entries
    if nb >= 3 and nb % sc.SCAN_TILE != 1:
        assert c["empty_ends"] and cnt[0] == 0 and cnt[-1] == 0
    assert crc(Ap, Ai, Ax) == int(G["scan%d__in" % nb])
    got = orc.csc_transpose(m, n, Ap, Ai, Ax)[2:]
    assert sc.same_csc(got, gold_csc("scan%d" % nb, ("t_p", "t_i", "t_x"))) and sc.same_csc(got, sc.transpose_restated(m, n, Ap, Ai, Ax))
    cols = sc.columns_of(Ap)
    got = orc.coo_to_csc(n, m, cols, Ai, Ax, len(Ai))[2:]
    assert sc.same_csc(got, gold_csc("scan%d_coo" % nb)) and sc.same_csc(got, sc.coo_restated(m, cols, Ai, Ax))


def test_empty_shapes_against_the_reference(orc):
    z = np.zeros(0, dtype=np.int32)
    for tag, m, n in (("m0", 0, 4), ("n0", 4, 0)):
        got = orc.csc_transpose(m, n, np.zeros(n + 1, dtype=np.int32), z, np.zeros(0))[2:]
        assert sc.same_csc(got, gold_csc(tag, ("t_p", "t_i", "t_x"))) and np.array_equal(got[0], np.zeros(m + 1))


# ---- 3. one grid pass plus one ----------------------------------------------------------------------------------------

def test_pass_plus_one_entries(orc):
    m, n, Ap, Ai, Ax, c = sc.pass_plus_one_entries()
    assert c["nnz"] == len(Ai) == Ap[n] == sc.GRID_CAP * sc.BLOCK + 1 and np.all(np.diff(Ap) >= 0)
    assert list(np.flatnonzero(Ai == m - 1)) == c["last_row_entries"] == [len(Ai) - 1]       # the last work item makes the last bucket
    assert Ai.min() >= 0 and Ai.max() == m - 1
    want = sc.transpose_restated(m, n, Ap, Ai, Ax)
    assert sc.same_csc(orc.csc_transpose(m, n, Ap, Ai, Ax)[2:], want)
    cols = sc.columns_of(Ap)
    perm = np.random.default_rng(3).permutation(len(Ai)); perm[-1], perm[np.argmax(perm)] = len(Ai) - 1, perm[-1]
    assert sc.same_csc(orc.coo_to_csc(n, m, cols[perm], Ai[perm], Ax[perm], len(perm))[2:], sc.coo_restated(m, cols[perm], Ai[perm], Ax[perm]))


def test_pass_plus_one_columns(orc):
    n, Ap, Ai, Ax, c = sc.pass_plus_one_columns()
    assert n == sc.GRID_CAP * sc.BLOCK + 1 == c["n"]
    lens = np.diff(Ap)
    hub = c["hub"]
    assert set(lens[:n - 1]) <= {1, 2, 3} and lens[n - 1] == len(hub) == 7 and sc.pattern_is_symmetric(n, Ap, Ai)
    assert list(Ai[Ap[n - 1]:Ap[n]]) == list(hub) and np.all(hub % 4096 != 0) and len(set(hub // 4096)) == 7
    assert hub.min() // 4096 == 0 and hub.max() // 4096 == (n - 2) // 4096             # the first and the last chain
    # the last bucket of the transpose: its entries' positions lie in both grid passes, and a lower position belongs to a
    # later block than a higher one (blocks start in order, and a block takes its second pass before later blocks start):
    # the bucket fills out of order
    pos = np.flatnonzero(Ai == n - 1)
    assert len(pos) == 7 and np.all(sc.columns_of(Ap)[pos] == hub)
    grid_pass, block = pos // sc.ONE_PASS, pos % sc.ONE_PASS // sc.BLOCK
    assert set(grid_pass) == {0, 1}
    assert any(grid_pass[s] < grid_pass[t] and block[s] > block[t] + 2048 for s in range(7) for t in range(s + 1, 7))
    sums = np.add.reduceat(np.abs(Ax), Ap[:-1])
    assert int(np.argmax(sums)) == c["largest_column"] == n - 1 and sums[n - 1] > 2 * np.delete(sums, n - 1).max()
    assert orc.csc_norm(n, Ap, Ax) == sc.norm_restated(n, Ap, Ax) == c["largest_sum"] == 52.5
    assert sc.same_csc(orc.csc_transpose(n, n, Ap, Ai, Ax)[2:], sc.transpose_restated(n, n, Ap, Ai, Ax))
    label = sc.island_labels_restated(n, Ap, Ai, True)
    assert np.array_equal(label, c["label"]) and label[n - 1] == c["last_node_island"] == 0 and len(np.unique(label)) == c["islands"] == 250
    # after the first hook round the last node points at its smallest neighbour, and that one at its own: not a root
    assert Ai[Ap[n - 1]:Ap[n]].min() == 1500 and Ai[Ap[1500]:Ap[1501]].min() == 1499 != label[1500]
    of = np.zeros(n, dtype=np.int32)
    cnt = orc.lib().orc_find_islands(orc.I64(n), orc._pi(Ap), orc._pi(Ai), orc._pi(of))
    assert cnt == 250 and np.array_equal(np.unique(label)[of], label)                  # island k of the oracle = the k-th smallest label


@pytest.mark.parametrize("kind", ["no way in", "one way in"])
def test_pass_plus_one_directed(orc, kind):
    n, Ap, Ai, c = sc.pass_plus_one_directed(kind)
    n0, Ap0, Ai0, _, c0 = sc.pass_plus_one_columns()
    cols = sc.columns_of(Ap).astype(np.int64)
    back = np.unique(cols * n + Ai)
    lonely = ~np.isin(Ai.astype(np.int64) * n + cols, back)
    # every entry without a mirror is in the last column, the last work item of k_pattern_symmetric
    assert sorted(set(cols[lonely])) == c["unsymmetric_columns"] == [n - 1] and np.array_equal(Ai[Ap[n - 1]:Ap[n]], c0["hub"])
    assert lonely.sum() == (7 if kind == "no way in" else 6) and Ap0[n] - Ap[n] == lonely.sum()
    label = c["label"]
    assert np.array_equal(sc.island_labels_restated(n, Ap, Ai, False), label) and len(np.unique(label)) == c["islands"]
    if kind == "no way in":
        assert label[n - 1] == n - 1 and c["islands"] == 257 and not np.array_equal(label, c0["label"])      # the symmetric treatment differs
    else:
        # only the last column leads into the six other chains: without its work item they keep their own labels
        assert label[n - 1] == 0 and c["islands"] == 250 and list(cols[Ai == n - 1]) == [1500]
        assert all(label[v] == 0 and n - 1 in set(Ai0[Ap0[v]:Ap0[v + 1]]) and n - 1 not in set(Ai[Ap[v]:Ap[v + 1]]) for v in c0["hub"][1:])
    of = np.zeros(n, dtype=np.int32)
    cnt = orc.lib().orc_find_islands(orc.I64(n), orc._pi(Ap), orc._pi(Ai), orc._pi(of))
    assert cnt == c["islands"] and np.array_equal(np.unique(label)[of], label)


def test_pass_plus_one_add_and_sub(orc):
    m, n, A, B, alpha, beta, c = sc.pass_plus_one_add()
    assert n == sc.GRID_CAP * sc.ADD_BLOCK + 1 and np.all(np.diff(A[0]) == 1)
    assert np.flatnonzero(np.diff(B[0])).tolist() == [c["overlap_column"]] == [n - 1] and A[1][-1] in B[1] and len(set(B[1])) == 2
    Cp, Ci, Cx = orc.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)[2:]
    assert Cp[n] == c["nnz_c"] and np.array_equal(Ci[:n], A[1]) and sc.same_bits(Cx[:n - 1], alpha * A[2][:n - 1])
    assert Ci[n] == B[1][0] and Cx[n] == beta * B[2][0] and Cx[n - 1] == alpha * A[2][-1] + beta * B[2][1]
    Am, Ap, Ai, Ax, rows, cols, c = sc.pass_plus_one_sub()
    assert len(cols) == sc.SUB_COLS_PER_PASS + 1 and len(rows) <= 3 and np.diff(Ap).max() <= 4
    hit = np.isin(Ai, rows)
    assert hit.sum() == c["matches"] == 1 and sc.columns_of(Ap)[hit][0] == c["match_column"] == len(cols) - 1
    nz, Bp, Bi, Bx = orc.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
    assert nz == 1 and np.all(Bp[:-1] == 0) and Bp[-1] == 1 and list(Bi) == [1] and Bx[0] == Ax[hit][0]     # row 2 unmatched first: numbering from 1
    Am, Ap, Ai, Ax, rows, cols, c = sc.sub_over_capacity()
    assert c["result"] == sum(np.isin(Ai[Ap[j]:Ap[j + 1]], rows).sum() for j in cols) > c["room"] == len(Ai)


# ---- 4. csc_add_ff ------------------------------------------------------------------------------------------------------

def test_add_cases_claims_and_oracle(orc):
    cases = sc.add_cases()
    m, n, A, B, alpha, beta, c = cases["columns"]
    col = lambda M, j: (M[1][M[0][j]:M[0][j + 1]], M[2][M[0][j]:M[0][j + 1]])            # noqa: E731
    k = {name: j for j, name in enumerate(c["names"])}
    ra, rb = col(A, k["same rows"])[0], col(B, k["same rows"])[0]
    assert np.array_equal(ra, rb) and len(ra) > 1
    assert not set(col(A, k["none shared"])[0]) & set(col(B, k["none shared"])[0])
    ra, rb = col(A, k["last shared"])[0], col(B, k["last shared"])[0]
    assert set(ra) & set(rb) == {ra[-1]} == {rb[-1]}
    ra, rb = col(A, k["duplicates"])[0], col(B, k["duplicates"])[0]
    assert len(set(ra)) < len(ra) and len(set(rb)) < len(rb)
    ra, rb = col(A, k["300 each"])[0], col(B, k["300 each"])[0]
    assert len(ra) == len(rb) == c["longest_column"] == 300 and len(set(ra) & set(rb)) == 150
    assert len(col(A, k["A empty"])[0]) == 0 < len(col(B, k["A empty"])[0]) and len(col(B, k["B empty"])[0]) == 0 < len(col(A, k["B empty"])[0])
    assert len(col(A, k["both empty"])[0]) == len(col(B, k["both empty"])[0]) == 0
    for name, (m, n, A, B, alpha, beta, _) in cases.items():
        tag = "add_" + name.replace(" ", "_")
        assert crc(*A, *B) == int(G[tag + "__in"])
        got = orc.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)[2:]
        assert sc.same_csc(got, gold_csc(tag)), name
    # what the reference made of the signed zeros, infinities and NaNs
    Cp, Ci, Cx = gold_csc("add_columns")
    j = k["signed zeros"]
    rows, vals = Ci[Cp[j]:Cp[j + 1]], Cx[Cp[j]:Cp[j + 1]]
    assert list(rows) == [5, 9, 2] and np.all(vals == 0.0) and list(np.signbit(vals)) == [False, True, True]
    j = k["inf nan"]
    rows, vals = Ci[Cp[j]:Cp[j + 1]], Cx[Cp[j]:Cp[j + 1]]
    assert list(rows) == [4, 1, 8, 3, 6] and vals[0] == np.inf and np.isnan(vals[1]) and vals[2] == 3.0 and vals[3] == -np.inf and np.isnan(vals[4])
    assert int(G["add_both_empty__p"][-1]) == 0


# ---- 5. csc_sub_matrix ---------------------------------------------------------------------------------------------------

def test_sub_matrix_claims_and_oracle(orc):
    Am, Ap, Ai, Ax, c = sc.sub_matrix_source()
    lens = list(np.diff(Ap))
    assert lens == c["col_lengths"] and set(sc.EDGE_LENGTHS) <= set(lens)
    where = [list(np.flatnonzero(Ai[Ap[j]:Ap[j + 1]] == sc.SUB_R0)) for j in range(len(lens))]
    assert [w[0] if w else None for w in where] == c["r0_at"]
    assert {0, 63, 64, 199} <= {w[0] for j, w in enumerate(where) if w and lens[j] == 200} and any(not w and lens[j] == 200 for j, w in enumerate(where))
    t = c["twice_col"]
    assert len(where[t]) == 2 and list(Ai[Ap[t]:Ap[t + 1]]).count(c["twice_rows"][1]) == 2
    for nrows in sc.SUB_ROW_COUNTS:
        rows, cols = sc.sub_selection(nrows, Ap, Ai)
        assert len(rows) == nrows and len(set(rows)) == nrows and (nrows < 3 or np.any(np.diff(rows) < 0))
        assert (nrows == 0 or rows[0] == sc.SUB_R0) and (nrows < 3 or c["twice_rows"][1] in rows)
        assert sorted(cols) == sorted(list(range(len(lens))) + [1])                   # one column twice
        tag = "sub%d" % nrows
        assert crc(Ap, Ai, Ax, rows, cols) == int(G[tag + "__in"])
        nz, Bp, Bi, Bx = orc.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, rows, cols)
        assert nz == int(G[tag + "__nz"]) <= len(Ai) and sc.same_csc((Bp, Bi, Bx), gold_csc(tag)), nrows
        if nrows:                                            # the numbering starts at 1 exactly where SUB_R0 matches nothing
            for k, j in enumerate(cols):
                if Bp[k + 1] > Bp[k]:
                    assert Bi[Bp[k]] == (0 if where[j] else 1)
    nz, Bp, Bi, Bx = orc.csc_sub_matrix(Am, len(Ai), Ap, Ai, Ax, np.array([sc.SUB_R0, 5], dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert nz == int(G["sub_ncols0__nz"]) == 0 and np.array_equal(Bp, G["sub_ncols0__p"])


# ---- 6. csc_norm ---------------------------------------------------------------------------------------------------------

def test_norm_cases_claims_and_oracle(orc):
    cases = sc.norm_cases()
    assert [cases["n%d" % n][0] for n in sc.NORM_COLUMNS] == [0, 1, 1023, 1024, 1025, 2049]
    for name, (n, Ap, Ax, c) in cases.items():
        tag = "norm_" + name.replace(" ", "_")
        assert crc(Ap, Ax) == int(G[tag + "__in"])
        want = float(G[tag])
        if name.startswith("n") and name[1:].isdigit() and n:
            sums = np.zeros(n); nzc = np.flatnonzero(np.diff(Ap)); sums[nzc] = np.add.reduceat(np.abs(Ax), Ap[nzc])
            assert int(np.argmax(sums)) == c["largest_column"] == n - 1 and sums[n - 1] == want == 3.75 > np.delete(sums, n - 1).max(initial=0.0)
        if "norm" in c:
            assert want == c["norm"]
        if "nan_entry" in c:
            assert np.isnan(Ax[c["nan_entry"]]) and np.isnan(Ax).sum() == 1 and np.isfinite(want) and want > 0.0      # the reference passes a NaN sum over
        assert sc.same_bits(sc.norm_restated(n, Ap, Ax), want), name
        assert sc.same_bits(orc.csc_norm(n, Ap, Ax), want), name
    assert float(G["norm_nan"]) == 3.75 and float(G["norm_nan_last"]) < 3.0


# ---- 7. find_islands -----------------------------------------------------------------------------------------------------

def test_island_cases_claims_and_oracle(orc):
    cases = sc.island_cases()
    for name, (n, Ap, Ai, c) in cases.items():
        tag = "isl_" + name.replace(" ", "_")
        assert crc(Ap, Ai) == int(G[tag + "__in"])
        assert sc.pattern_is_symmetric(n, Ap, Ai) == c["symmetric"], name
        want = np.split(G[tag + "__flat"], np.cumsum(G[tag + "__sizes"])[:-1])
        assert sc.same_islands(sc.islands_from_labels(sc.island_labels_restated(n, Ap, Ai, c["symmetric"])), want), name
        assert sc.same_islands(orc.find_islands(n, Ap, Ai), want), name
        if "islands" in c:
            assert len(want) == c["islands"], name
    n, Ap, Ai, c = cases["star hub last"]
    assert np.diff(Ap)[c["hub"]] == n - 1 and np.all(np.diff(Ap)[:-1] == 1) and c["hub"] == n - 1
    n, Ap, Ai, c = cases["star hub first"]
    assert np.diff(Ap)[0] == n - 1 and np.all(np.diff(Ap)[1:] == 1)
    n, Ap, Ai, c = cases["zigzag path"]
    seq = c["sequence"]
    assert list(seq[:4]) == [n - 1, 0, n - 2, 1] and sorted(seq) == list(range(n)) and np.diff(Ap).max() == 2
    # every node but the two ends has one neighbour above and one below it... except that the smaller one is far away:
    # a node's smallest neighbour is at most one step closer to node 0 along the path
    pos = np.empty(n, dtype=np.int64); pos[seq] = np.arange(n)
    assert all(abs(pos[Ai[p]] - pos[j]) == 1 for j in range(n) for p in range(Ap[j], Ap[j + 1]))
    n, Ap, Ai, c = cases["binary tree"]
    deg = np.diff(Ap)
    assert n == 4095 and deg[c["root"]] == 2 and np.all(deg[:2048] == 1) and np.all(deg[2048:n - 1] == 3)    # leaves first
    n1, Ap1, Ai1, _ = cases["two rings joined"]; n2, Ap2, Ai2, _ = cases["two rings apart"]
    assert Ap1[-1] - Ap2[-1] == 2                                                         # one edge, stored both ways
    n, Ap, Ai, c = cases["last entry dropped"]
    i, j = c["dropped"]
    assert j == n - 1 and i not in Ai[Ap[n - 1]:Ap[n]] and (n - 1) in Ai[Ap[i]:Ap[i + 1]]
    full_p = Ap.copy(); full_p[n] += 1
    assert sc.pattern_is_symmetric(n, full_p, np.concatenate([Ai, [i]]).astype(np.int32))
    # ... and the missing entry is the only unsymmetric one, met after every other entry in column order
    cols = sc.columns_of(Ap).astype(np.int64)
    back = set((cols * n + Ai).tolist())
    lonely = [(int(r), int(cc)) for r, cc in zip(Ai, cols) if r != cc and int(r) * n + int(cc) not in back]
    assert lonely == [(n - 1, i)]
    # the mirror case: the only entry without a mirror is the only entry of the last column, the last stored entry of all
    n, Ap, Ai, c = cases["mirror of last entry dropped"]
    cols = sc.columns_of(Ap).astype(np.int64)
    back = set((cols * n + Ai).tolist())
    lonely = [(int(r), int(cc)) for r, cc in zip(Ai, cols) if r != cc and int(r) * n + int(cc) not in back]
    assert lonely == [c["lonely"]] == [(n - 2, n - 1)] == [(int(Ai[-1]), int(cols[-1]))] and Ap[n] - Ap[n - 1] == 1
    full = sc.island_labels_restated(n, Ap, Ai, False)
    assert full[n - 1] == n - 1 and full[n - 2] == n - 300 and c["islands"] == 3          # a symmetric treatment leaves it with the last ring
    n, Ap, Ai, c = cases["loops duplicates"]
    cols = sc.columns_of(Ap)
    assert (Ai == cols).sum() == 500 and len(np.unique(cols.astype(np.int64) * n + Ai)) < len(Ai)


# ---- 8. stacking ----------------------------------------------------------------------------------------------------------

def test_stack_cases_claims_and_oracle(orc):
    cases = sc.stack_cases()
    blocks, c = cases["edges"]
    for b in blocks:
        assert set(sc.EDGE_LENGTHS) <= set(np.diff(b[3]))
    A, B, C, D = blocks
    assert any(a > 64 and cc > 64 for a, cc in zip(np.diff(A[3]), np.diff(C[3])))
    assert cases["an=0"][0][0][1] == 0 and cases["bn=0"][0][1][1] == 0 and cases["am=0"][0][0][0] == 0 and cases["cm=0"][0][2][0] == 0
    assert len(cases["C empty"][0][2][2]) == 0 and cases["C empty"][0][2][1] > 0
    recorded = 0
    for name, (blocks, _) in cases.items():
        tag = "stack_" + name.replace(" ", "_")
        m, n, Pi, Pp, Px, mp = sc.stack_restated(blocks)
        flat = [v for b in blocks for v in b]
        om, on, oPi, oPp, oPx = orc.csc_stack_4_by_4_ff(*flat)
        assert (om, on) == (m, n) and sc.same_csc((oPp, oPi, oPx), (Pp, Pi, Px)), name
        if tag + "__p" in G:
            recorded += 1
            assert crc(*[v for b in blocks for v in b[2:]]) == int(G[tag + "__in"])
            assert (m, n) == (int(G[tag + "__m"]), int(G[tag + "__n"])) and sc.same_csc((Pp, Pi, Px), gold_csc(tag)), name
        # the map: Px = (A | B | C | D)[map], a bijection, and the seams land where the blocks meet
        cat = np.concatenate([b[4] for b in blocks])
        assert sc.same_bits(cat[mp], Px) and sorted(mp) == list(range(len(cat)))
    assert recorded == len(cases)


def test_restack_pass_plus_one():
    mp, parts, c = sc.restack_pass_plus_one()
    assert len(mp) == c["nnz"] == sc.GRID_CAP * sc.BLOCK + 1 == sum(len(p) for p in parts)
    assert mp[-1] == c["nnz"] - 1 and np.flatnonzero(mp == c["nnz"] - 1).tolist() == [c["nnz"] - 1]
    assert sorted(set(c["seams"])) == c["seams"] and np.all(np.isin(c["seams"], mp))


# ---- 9. general triangular solves -------------------------------------------------------------------------------------------

def test_tri_edges_claims_and_oracle_error(orc):
    n, L, U, c = sc.tri_edges()
    for counts in (c["row_counts"], c["col_counts"]):
        assert set(sc.EDGE_LENGTHS) <= set(counts) and counts.max() == 200
    (Lp, Li, Lx), (Up, Ui, Ux) = L, U
    assert np.array_equal(np.diff(Lp) - 1, c["col_counts"]) and np.array_equal(np.diff(Up) - 1, c["row_counts"])
    assert all(Li[Lp[j]] == j and Ui[Up[j + 1] - 1] == j for j in range(n))                # diagonal first / last
    assert any(np.any(np.diff(Li[Lp[j] + 1:Lp[j + 1]]) < 0) for j in range(n)) and any(np.any(np.diff(Ui[Up[j]:Up[j + 1] - 1]) < 0) for j in range(n))
    GL, GU = sc.tri_dense(n, *L), sc.tri_dense(n, *U)
    assert np.array_equal(GL, GU.T) and np.array_equal(GL, np.tril(GL))
    assert np.linalg.cond(GL.astype(np.float64)) < 1e6
    for (name, k), (B, X, err) in sc.tri_references(orc, n, L, U).items():
        lower = name in ("lsolve", "ltsolve")
        G_ = (GL if lower else GU)
        G_ = G_.T if name.endswith("tsolve") else G_
        assert np.abs(G_ @ X.reshape(n, -1) - B.reshape(n, -1)).max() < 1e-15 * 50          # the longdouble solution solves the system
        assert 0.0 < err < 1e-13, (name, k, err)                                            # measured, and of rounding size


def test_tri_small_cases_claims(orc):
    cases = sc.tri_small_cases()
    assert cases["n=1"][0] == 1 and cases["chain"][0] == 1500
    for name, (n, L, U, c) in cases.items():
        for solve, lower, trans in sc.TRI_SOLVES:
            Gp, Gi, _ = L if lower else U
            assert sc.tri_levels(n, Gp, Gi, lower, trans) == c["levels"], (name, solve)
        if name != "chain":
            assert L[0][-1] == n == U[0][-1]                                                # pure diagonal
        for (solve, k), (B, X, err) in sc.tri_references(orc, n, L, U).items():
            assert err < 1e-13
    n, L, U, c = sc.tri_edges()
    assert sc.tri_levels(n, L[0], L[1], True, False) > 1


# ---- 10. resident products ----------------------------------------------------------------------------------------------------

def test_resident_matrix_claims(orc):
    n, Ap, Ai, Ax, c = sc.resident_matrix()
    assert n * sc.RESIDENT_K > sc.RESIDUAL_GRID_CAP * 256 > sc.AXPY_GRID_CAP * 256
    rows = np.bincount(Ai, minlength=n)
    assert rows[c["long_row"]] == c["long_row_entries"] == 200 and rows[c["empty_row"]] == 0 and np.diff(Ap)[c["empty_row"]] == 0
    assert rows.max() == 200 and np.all(np.diff(Ai.astype(np.int64) + sc.columns_of(Ap).astype(np.int64) * n) > 0)    # sorted, no duplicates
    # the restatement of the summation order against the oracle's csc_mat_vec_ff loop, plain and transposed
    X = np.random.default_rng(1).standard_normal((n, 2))
    Y = sc.matvec_restated(n, Ap, Ai, Ax, X)
    assert sc.same_bits(Y, orc.csc_mat_vecs(n, n, Ap, Ai, Ax, X)) and np.all(Y[c["empty_row"]] == 0.0)
    _, _, Tp, Ti, Tx = orc.csc_transpose(n, n, Ap, Ai, Ax)
    # A' x summed in the storage order of A's column = the matvec of the transpose only when rows ascend in a column: they do
    assert sc.same_bits(sc.matvec_restated(n, Ap, Ai, Ax, X, trans=True), orc.csc_mat_vecs(n, n, Tp, Ti, Tx, X))
    n2, Ap2, Ai2, Ax2, c2 = sc.resident_matrix(empty_row=False)
    cols = sc.columns_of(Ap2)
    d = np.abs(Ax2[Ai2 == cols]); off = np.bincount(Ai2[Ai2 != cols], weights=np.abs(Ax2[Ai2 != cols]), minlength=n2)
    assert len(d) == n2 and np.all(d > off) and c2["empty_row"] is None                   # strictly diagonally dominant by rows
