"""Inputs of the edge tests of the conversion / assembly kernels (substrate.hip) and of the Newton-chain glue in
kernels.hip, shared by tests/test_substrate_cases_cpu.py (which proves every claim from NumPy alone) and
tests/test_gpu_substrate_edges.py.  Every builder returns its inputs plus a dict of the claims it makes.  No GPU here.

The constants below are read off the kernels; the code is their only source, and test_substrate_cases_cpu.py checks that
the cited line still holds the number.  Whoever changes one of them finds here which cases depend on it.

    SORT_INSERTION_MAX 32    substrate.hip:84    sort_ints: buckets up to this length are insertion-sorted, longer ones heap-sorted
    SCAN_TILE          4096  substrate.hip:48    k_scan: entries per tile, a carried total between tiles
    GRID_CAP           4096  substrate.hip:321   blocks_for: blocks per launch; beyond it the grid-stride loops take over
    BLOCK              256   substrate.hip:339   threads per block of the 256-thread kernels (work items per pass: 4096 * 256)
    ADD_BLOCK          128   substrate.hip:444   k_add_columns: one column per thread (4096 * 128 columns per pass)
    WAVE               64    substrate.hip:220   k_sub_matrix: lanes over a column (bump search) and over the row selection (:224)
    SUB_COLS_PER_PASS  16384 substrate.hip:482   k_sub_matrix: one wave per selected column, 4 per block, 4096 blocks
    REDUCE_THREADS     1024  substrate.hip:152   k_max_reduce: one block, column sums strided by 1024
    STACK_WAVE         64    kernels.hip:3870    k_stack_4_by_4: one wave copies a block column 64 entries at a time
    TRI_WAVE           64    kernels.hip:3758    k_tri_level: lanes split a row 64 entries at a time
    RESIDUAL_GRID_CAP  4096  kernels.hip:3832    k_residual_rows (k_matvec_rows: grid_for's default cap, kernels.hip:3923)
    AXPY_GRID_CAP      2048  kernels.hip:3840    k_axpy_max
"""
import os

import numpy as np

SORT_INSERTION_MAX = 32
SCAN_TILE = 4096
GRID_CAP = 4096
BLOCK = 256
ADD_BLOCK = 128
WAVE = 64
SUB_COLS_PER_PASS = GRID_CAP * BLOCK // WAVE
REDUCE_THREADS = 1024
STACK_WAVE = 64
TRI_WAVE = 64
RESIDUAL_GRID_CAP = 4096
AXPY_GRID_CAP = 2048

# (name, value, file under csparse3_amd/csrc, line, text that line must contain)
SOURCE_LINES = [
    ("SORT_INSERTION_MAX", SORT_INSERTION_MAX, "substrate.hip", 84, "if (len <= 32)"),
    ("SCAN_TILE", SCAN_TILE, "substrate.hip", 48, "base += 4096"),
    ("GRID_CAP", GRID_CAP, "substrate.hip", 321, "4096));"),
    ("BLOCK", BLOCK, "substrate.hip", 339, "blocks_for(count, 256)), dim3(256)"),
    ("ADD_BLOCK", ADD_BLOCK, "substrate.hip", 444, "blocks_for(n, 128)), dim3(128)"),
    ("WAVE", WAVE, "substrate.hip", 220, "k += 64"),
    ("WAVE", WAVE, "substrate.hip", 224, "rr0 += 64"),
    ("SUB_COLS_PER_PASS", SUB_COLS_PER_PASS, "substrate.hip", 482, "blocks_for((long long) ncols * 64, 256)"),
    ("REDUCE_THREADS", REDUCE_THREADS, "substrate.hip", 152, "i += 1024"),
    ("STACK_WAVE", STACK_WAVE, "kernels.hip", 3870, "k += 64"),
    ("STACK_WAVE", STACK_WAVE, "kernels.hip", 3874, "k += 64"),
    ("TRI_WAVE", TRI_WAVE, "kernels.hip", 3758, "p += 64"),
    ("RESIDUAL_GRID_CAP", RESIDUAL_GRID_CAP, "kernels.hip", 3832, "4096)"),
    ("AXPY_GRID_CAP", AXPY_GRID_CAP, "kernels.hip", 3840, "2048)"),
]

ONE_PASS = GRID_CAP * BLOCK                 # work items the 256-thread kernels cover without striding
EDGE_LENGTHS = (0, 1, 63, 64, 65, 200)      # either side of one wave of 64, and more than three waves
GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "substrate_edges.npz")
_gold = None


def gold():
    """The recorded outputs of the reference's own kernels (tests/golden/make_substrate_edges.py)."""
    global _gold
    if _gold is None:
        _gold = np.load(GOLD_PATH)
    return _gold


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def csc_from_columns(columns, values=None):
    """(Ap, Ai) from a list of row lists: stored order and duplicates kept."""
    Ap = np.zeros(len(columns) + 1, dtype=np.int32)
    if columns:
        Ap[1:] = np.cumsum([len(c) for c in columns])
    Ai = i32(np.concatenate([np.asarray(c, dtype=np.int64) for c in columns])) if columns and Ap[-1] else np.zeros(0, dtype=np.int32)
    return Ap, Ai


def csc_from_triplets(n, rows, cols, vals):
    """CSC with the entries of a column in triplet order (a stable sort by column: what coo_to_csc does)."""
    order = np.argsort(cols, kind="stable")
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.cumsum(np.bincount(cols, minlength=n)[:n]) if n else 0
    return Ap, i32(rows[order]), np.ascontiguousarray(vals[order], dtype=np.float64)


def columns_of(Ap):
    return np.repeat(np.arange(len(Ap) - 1, dtype=np.int32), np.diff(Ap))


def values(rng, count):
    """Distinct, non-zero, sign-mixed values: a misplaced entry is always visible.  (Quarters of small integers, so the
    recorded outputs compress; the kernels that round get rng.standard_normal instead.)"""
    v = rng.permutation(count).astype(np.float64) + 1.0
    return v * np.where(rng.random(count) < 0.5, -1.0, 1.0) * 0.25


def same_bits(a, b):
    """Bitwise equality of two float64 arrays (or scalars): distinguishes -0.0 from +0.0 and compares NaNs by pattern."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64))


def same_csc(got, want):
    """(p, i, x) triples equal: integers exactly, values bit for bit."""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])


# ---- oracle-independent restatements --------------------------------------------------------------------------------

def transpose_restated(m, n, Ap, Ai, Ax):
    """transpose = stable sort of the stored positions by row."""
    order = np.argsort(Ai, kind="stable")
    Cp = np.zeros(m + 1, dtype=np.int32)
    if m:
        Cp[1:] = np.cumsum(np.bincount(Ai, minlength=m))
    return Cp, columns_of(Ap)[order], Ax[order]


def coo_restated(n, Ti, Tj, Tx):
    """coo_to_csc = stable sort of the triplets by column."""
    return csc_from_triplets(n, Ti, Tj, Tx)


def norm_restated(n, Ap, Ax):
    """csc_norm: the largest column sum, with the reference's rule for NaN as the plain loop: `norm = max(norm, s)` keeps
    norm unless s > norm (csc_numba.py:738), so a NaN sum is passed over."""
    if n == 0:
        return 0.0
    nz = np.flatnonzero(np.diff(Ap))
    sums = np.zeros(n)
    if nz.size:
        sums[nz] = np.add.reduceat(np.abs(Ax), Ap[nz])      # (reduceat sums pairwise past 8 entries: use on short columns only)
    norm = 0.0
    for s in sums:
        if s > norm:
            norm = float(s)
    return norm


def island_labels_restated(n, Ap, Ai, symmetric):
    """label[i] = the smallest node that reaches i along column -> row edges (the island the reference's visiting rule
    puts i in).  Symmetric patterns: the smallest node of the connected component (scipy); otherwise a plain worklist."""
    if symmetric:
        import scipy.sparse as sp
        import scipy.sparse.csgraph as csg
        G = sp.csc_matrix((np.ones(len(Ai)), Ai, Ap), shape=(n, n))
        _, comp = csg.connected_components(G, directed=False)
        smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        return smallest[comp].astype(np.int32)
    label = np.full(n, -1, dtype=np.int32)
    for s in range(n):
        if label[s] >= 0:
            continue
        work = [s]
        label[s] = s
        while work:
            v = work.pop()
            for k in Ai[Ap[v]:Ap[v + 1]]:
                if label[k] < 0:
                    label[k] = s
                    work.append(int(k))
    return label


def islands_from_labels(label):
    """A list of islands ordered by their smallest node, each sorted: from label[i] = smallest node of i's island."""
    order = np.argsort(label, kind="stable")
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [g.astype(np.int32) for g in np.split(order, cuts)] if len(label) else []


def same_islands(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def pattern_is_symmetric(n, Ap, Ai):
    cols = columns_of(Ap).astype(np.int64)
    fwd = np.unique(cols * n + Ai)
    bwd = np.unique(Ai.astype(np.int64) * n + cols)
    return np.array_equal(fwd, bwd)


# ---- 1. bucket lengths ------------------------------------------------------------------------------------------------

BUCKET_ROW_LENGTHS = (0, 1, 2, 31, 32, 33, 64, 65, 1000)          # ... and n, the dense row


def bucket_lengths(seed=101, n=3001):
    """One m x n matrix whose rows (the buckets of the transpose) have 0, 1, 2, 31, 32, 33, 64, 65, 1000 and n entries,
    rows of every column in arbitrary order, plus two rows that sit twice and three times in some columns (43 and 70
    entries: both heap-sorted), so the order among duplicates shows in the values.
    -> (m, n, Ap, Ai, Ax, claims)."""
    rng = np.random.default_rng(seed)
    lengths = list(BUCKET_ROW_LENGTHS) + [n]
    rows, cols = [], []
    for r, L in enumerate(lengths):
        rows.append(np.full(L, r)); cols.append(np.sort(rng.choice(n, size=L, replace=False)))
    r2, r3 = len(lengths), len(lengths) + 1
    twice = np.sort(rng.choice(n, size=20, replace=False)); thrice = np.sort(rng.choice(n, size=20, replace=False))
    rows += [np.full(43, r2), np.full(70, r3)]
    cols += [np.concatenate([np.repeat(twice, 2), twice[:3]]), np.concatenate([np.repeat(thrice, 3), thrice[:10]])]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    perm = rng.permutation(len(rows))                       # unsorted rows inside a column, duplicates apart from each other
    m = r3 + 1
    Ap, Ai, Ax = csc_from_triplets(n, rows[perm], cols[perm], values(rng, len(rows)))
    claims = {"row_lengths": lengths + [43, 70], "max_bucket": n, "twice_row": r2, "thrice_row": r3,
              "twice_cols": twice, "thrice_cols": thrice}
    return m, n, Ap, Ai, Ax, claims


def bucket_triplets(seed=102):
    """The transpose of bucket_lengths() as triplets in a random permutation: for coo_to_csc the buckets are the columns,
    of 0, 1, 2, 31, 32, 33, 64, 65, 1000 and 3001 entries.  -> (m, n, Ti, Tj, Tx, claims)."""
    m, n, Ap, Ai, Ax, c = bucket_lengths()
    perm = np.random.default_rng(seed).permutation(len(Ai))
    return n, m, columns_of(Ap)[perm], Ai[perm].copy(), Ax[perm].copy(), {"col_lengths": c["row_lengths"]}


# ---- 2. scan tiles -----------------------------------------------------------------------------------------------------

SCAN_BUCKETS = (1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1)


def scan_tiles(nbucket, seed=7, ncols=5):
    """An nbucket x ncols matrix (the transpose scans nbucket counts) with 0 ... 3 entries per row, at least one entry in
    every tile of SCAN_TILE counts (so the carried total is non-zero and changes at every tile edge), two entries in the
    last row of every tile and in the first row of the next, and empty rows at both ends where there is room.
    -> (m, n, Ap, Ai, Ax, claims)."""
    rng = np.random.default_rng(seed + nbucket)
    cnt = rng.integers(0, 4, size=nbucket)
    for e in range(SCAN_TILE, nbucket, SCAN_TILE):          # counts e-1 and e (0-based) end one tile and start the next
        cnt[e - 1] = 2
        cnt[e] = 2
    if nbucket >= 3:
        cnt[0] = 0
        if nbucket % SCAN_TILE != 1:                         # (a last tile of one count keeps it, or its tile would add nothing)
            cnt[-1] = 0
        cnt[1] = max(cnt[1], 1)
    else:
        cnt[:] = np.arange(1, nbucket + 1)
    rows = rng.permutation(np.repeat(np.arange(nbucket), cnt))
    cols = np.sort(rng.integers(0, ncols, size=len(rows)))
    Ap, Ai, Ax = csc_from_triplets(ncols, rows, cols, values(rng, len(rows)))
    totals = np.cumsum(cnt)
    edges = list(range(SCAN_TILE, nbucket, SCAN_TILE))
    claims = {"tiles": -(-nbucket // SCAN_TILE), "carry_at_edges": [int(totals[e - 1]) for e in edges],
              "tile_sums": [int(cnt[t:t + SCAN_TILE].sum()) for t in range(0, nbucket, SCAN_TILE)],
              "empty_ends": bool(cnt[0] == 0 and cnt[-1] == 0)}
    return nbucket, ncols, Ap, Ai, Ax, claims


# ---- 3. one grid pass plus one ----------------------------------------------------------------------------------------

def pass_plus_one_entries(seed=11, m=4099, n=64):
    """nnz = 4096 * 256 + 1 entries (k_histogram / k_bucket_fill / k_gather_pairs stride once): the last stored entry is the
    only entry of the last row, so the last work item alone makes the last bucket.  -> (m, n, Ap, Ai, Ax, claims)."""
    rng = np.random.default_rng(seed)
    nnz = ONE_PASS + 1
    Ai = rng.integers(0, m - 1, size=nnz).astype(np.int32)
    Ai[-1] = m - 1
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.sort(rng.integers(0, nnz, size=n))
    Ap[n] = nnz
    Ap[n - 1] = min(Ap[n - 1], nnz - 1)                     # the last column is not empty
    Ax = values(rng, nnz)
    return m, n, Ap, Ai, Ax, {"nnz": nnz, "last_row_entries": [nnz - 1]}


PASS_HUB = (1500, 262921, 512100, 524328, 537088, 787431, ONE_PASS - 100)


def pass_plus_one_columns(seed=12):
    """m = n = 4096 * 256 + 1: chains j -- j + 1 of 4096 nodes (two entries per column, one at the chain ends), stored
    symmetrically, and the last node joined to the seven nodes of PASS_HUB: interior nodes (not the smallest) of seven
    chains, the first and the last chain among them.  Row n - 1 (the last bucket of the transpose) therefore holds seven
    entries whose stored positions lie in both grid passes of k_bucket_fill, lower positions in later blocks than higher
    ones, so the bucket fills out of order and k_bucket_sort's last work item has to sort it.  The last column has the
    largest sum (k_col_abs_sums, k_expand_columns).  The first hook round leaves label[n - 1] = 1500, which is no root:
    the last work item of k_label_jump has to compress it to 0.  -> (n, Ap, Ai, Ax, claims)."""
    n = ONE_PASS + 1
    j = np.arange(n - 2, dtype=np.int64)
    j = j[(j + 1) % 4096 != 0]                               # edge j -- j + 1 unless j + 1 starts a chain
    hub = np.array(PASS_HUB, dtype=np.int64)
    lo = np.concatenate([j, hub]); hi = np.concatenate([j + 1, np.full(len(hub), n - 1)])
    rows = np.concatenate([hi, lo]); cols = np.concatenate([lo, hi])
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    rng = np.random.default_rng(seed)
    Ax = rng.uniform(0.5, 1.0, size=len(rows))
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.cumsum(np.bincount(cols, minlength=n))
    Ax[Ap[n - 1]:Ap[n]] = 7.5                               # the largest column sum by far
    label = (np.arange(n) // 4096 * 4096).astype(np.int32)   # the smallest node of every chain ...
    label[np.isin(label, hub // 4096 * 4096)] = 0            # ... and of the seven that the last node joins
    label[n - 1] = 0
    return n, Ap, i32(rows), Ax, {"n": n, "largest_column": n - 1, "largest_sum": 7.5 * len(hub), "hub": hub, "label": label,
                                  "last_node_island": 0, "islands": (n - 1) // 4096 - (len(hub) - 1)}


def pass_plus_one_directed(kind):
    """pass_plus_one_columns() made unsymmetric so that every entry without a mirror sits in the last column, the last
    work item of k_pattern_symmetric:
    "no way in": row n - 1 is taken out of every other column.  Nothing reaches the last node, so it is an island of its
        own, and the chains it points at stay apart (each is entered from its own smallest node first).  A symmetric
        treatment would merge all eight.
    "one way in": row n - 1 stays in column 1500 only.  Node 0 reaches the last node through its chain, and the six other
        chains only through the last column, the last work item of k_reach_hook.
    -> (n, Ap, Ai, claims) with claims["label"][i] = the smallest node that reaches i."""
    n, Ap, Ai, _, c = pass_plus_one_columns()
    cols = columns_of(Ap)
    keep = ~((Ai == n - 1) & (cols != n - 1))
    label = c["label"].copy()
    if kind == "one way in":
        keep |= (Ai == n - 1) & (cols == PASS_HUB[0])
    else:
        assert kind == "no way in"
        label = (np.arange(n) // 4096 * 4096).astype(np.int32)
        label[n - 1] = n - 1
    Ap2 = np.zeros(n + 1, dtype=np.int32)
    Ap2[1:] = np.cumsum(np.bincount(cols[keep], minlength=n))
    return n, Ap2, Ai[keep].copy(), {"label": label, "islands": len(np.unique(label)), "unsymmetric_columns": [n - 1]}


def pass_plus_one_add(seed=13, m=8):
    """n = 4096 * 128 + 1 columns for csc_add_ff: one entry per column in A, B empty but for the last column, where it
    holds A's row (the only overlap) and one more.  -> (m, n, A, B, alpha, beta, claims)."""
    rng = np.random.default_rng(seed)
    n = GRID_CAP * ADD_BLOCK + 1
    Ap = np.arange(n + 1, dtype=np.int32)
    Ai = rng.integers(0, m, size=n).astype(np.int32)
    Ax = values(rng, n)
    Bp = np.zeros(n + 1, dtype=np.int32); Bp[n] = 2
    Bi = i32([(Ai[-1] + 1) % m, Ai[-1]])
    Bx = np.array([0.375, -2.5])
    return m, n, (Ap, Ai, Ax), (Bp, Bi, Bx), 1.5, -0.25, {"n": n, "overlap_column": n - 1, "nnz_c": n + 1}


def pass_plus_one_sub(seed=14):
    """ncols = 16 385 selected columns (one wave each, 16 384 per pass), 3 selected rows, columns of at most 4 entries; the
    only match is in the last selected column.  -> (Am, Ap, Ai, Ax, rows, cols, claims)."""
    rng = np.random.default_rng(seed)
    ncols = SUB_COLS_PER_PASS + 1
    Am = 16
    lens = rng.integers(0, 5, size=ncols); lens[-1] = 4
    Ap = np.zeros(ncols + 1, dtype=np.int32); Ap[1:] = np.cumsum(lens)
    Ai = rng.integers(3, Am, size=Ap[-1]).astype(np.int32)   # rows 0 ... 2 are the selection: no match anywhere ...
    Ai[Ap[ncols - 1] + 2] = 1                                # ... but here
    rows = i32([2, 1, 0])
    cols = np.arange(ncols, dtype=np.int32)
    return Am, Ap, Ai, values(rng, len(Ai)), rows, cols, {"ncols": ncols, "matches": 1, "match_column": ncols - 1}


def sub_over_capacity():
    """A 4-column matrix of 8 entries selected 16 385 times over: the result outgrows nnz(A) (all the reference allocates)."""
    Ap = i32([0, 2, 4, 6, 8]); Ai = i32([0, 1, 1, 2, 0, 3, 2, 3]); Ax = np.arange(1.0, 9.0)
    cols = (np.arange(SUB_COLS_PER_PASS + 1) % 4).astype(np.int32)
    return 4, Ap, Ai, Ax, i32([0, 1, 2, 3]), cols, {"result": 2 * (SUB_COLS_PER_PASS + 1), "room": 8}


# ---- 4. csc_add_ff ------------------------------------------------------------------------------------------------------

ADD_ALPHA, ADD_BETA = 1.5, -0.25


def add_cases(seed=21, m=700):
    """name -> (m, n, (Ap, Ai, Ax), (Bp, Bi, Bx), alpha, beta, claims).  "columns" has one column per situation (claims
    name them); the others are whole matrices that are empty."""
    rng = np.random.default_rng(seed)
    pick = lambda k: list(rng.choice(m, size=k, replace=False))
    ca, cb, va, vb, names = [], [], [], [], []

    def col(name, ra, rb, xa=None, xb=None):
        names.append(name); ca.append(ra); cb.append(rb)
        va.append(rng.standard_normal(len(ra)) if xa is None else np.asarray(xa, dtype=np.float64))
        vb.append(rng.standard_normal(len(rb)) if xb is None else np.asarray(xb, dtype=np.float64))

    r = pick(9)
    col("same rows", r, list(r))
    r = pick(12)
    col("none shared", r[:7], r[7:])
    r = pick(11)
    col("last shared", r[:6], r[6:] + [r[5]])
    r = pick(6)
    col("duplicates", [r[0], r[1], r[0], r[2], r[1], r[0]], [r[3], r[3], r[0], r[4], r[3], r[5], r[4]])
    r = pick(450)
    col("300 each", r[:300], list(rng.permutation(r[150:450])))
    # 1.5 * 1 - 0.25 * 6 = +0.0 (the entry stays); 1.5 * -0.0 + (-0.25 * 0.0) = -0.0 + -0.0 = -0.0; alone: 1.5 * -0.0
    col("signed zeros", [5, 9, 2], [9, 5], [1.0, -0.0, -0.0], [0.0, 6.0])
    col("inf nan", [4, 1, 8, 3], [1, 3, 6], [np.inf, np.nan, 2.0, -np.inf], [1.0, np.inf, np.nan])
    col("A empty", [], pick(5))
    col("B empty", pick(5), [])
    col("both empty", [], [])
    Ap, Ai = csc_from_columns(ca); Bp, Bi = csc_from_columns(cb)
    A = (Ap, Ai, np.concatenate(va)); B = (Bp, Bi, np.concatenate(vb))
    n = len(names)
    E = lambda: (np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))       # noqa: E731
    out = {"columns": (m, n, A, B, ADD_ALPHA, ADD_BETA, {"names": names, "longest_column": 300})}
    out["A empty"] = (m, n, E(), B, ADD_ALPHA, ADD_BETA, {})
    out["B empty"] = (m, n, A, E(), ADD_ALPHA, ADD_BETA, {})
    out["both empty"] = (m, n, E(), E(), ADD_ALPHA, ADD_BETA, {})
    return out


# ---- 5. csc_sub_matrix ---------------------------------------------------------------------------------------------------

SUB_ROW_COUNTS = (0, 1, 63, 64, 65, 129)
SUB_R0 = 300                                                # the first selected row of every selection


def sub_matrix_source(seed=31, Am=400):
    """The matrix the selections are taken from: columns of 0, 1, 63, 64, 65 entries, four of 200 entries with row SUB_R0
    at entry position 0, 63, 64 and 199, one of 200 without it, and one that holds SUB_R0 and another row twice.
    -> (Am, Ap, Ai, Ax, claims)."""
    rng = np.random.default_rng(seed)
    others = np.array([r for r in range(Am) if r != SUB_R0])
    cols, r0_at = [], []
    for L in (0, 1, 63, 64, 65):
        c = list(rng.choice(others, size=L, replace=False))
        cols.append(c); r0_at.append(None)
    cols[1] = [SUB_R0]; r0_at[1] = 0
    for pos in (0, 63, 64, 199, None):
        c = list(rng.choice(others, size=200, replace=False))
        if pos is not None:
            c[pos] = SUB_R0
        cols.append(c); r0_at.append(pos)
    c = list(rng.choice(others, size=40, replace=False))
    c[7] = SUB_R0; c[31] = SUB_R0; c[12] = c[3]
    cols.append(c); r0_at.append(7)
    Ap, Ai = csc_from_columns(cols)
    return Am, Ap, Ai, values(rng, len(Ai)), {"col_lengths": [len(c) for c in cols], "r0_at": r0_at, "twice_col": len(cols) - 1,
                                              "twice_rows": (SUB_R0, int(c[3]))}


def sub_selection(nrows, Ap, Ai, seed=32, Am=400):
    """A selection of nrows rows in non-monotone order, SUB_R0 first, the row stored twice among them (from 3 rows on);
    every column once in a shuffled order and the one-entry column a second time.  -> (rows, cols)."""
    rng = np.random.default_rng(seed + nrows)
    n = len(Ap) - 1
    twice_other = int(Ai[Ap[n - 1] + 3])
    rest = rng.permutation([r for r in range(Am) if r not in (SUB_R0, twice_other)])
    rows = ([SUB_R0] + ([twice_other] if nrows >= 3 else []) + list(rest))[:nrows]
    if nrows >= 3:
        rows = [rows[0]] + list(rng.permutation(rows[1:]))
    cols = list(rng.permutation(n)) + [1]
    return i32(rows), i32(cols)


# ---- 6. csc_norm ---------------------------------------------------------------------------------------------------------

NORM_COLUMNS = (0, 1, REDUCE_THREADS - 1, REDUCE_THREADS, REDUCE_THREADS + 1, 2 * REDUCE_THREADS + 1)


def norm_cases(seed=41):
    """name -> (n, Ap, Ax, claims): 0 ... 2049 columns of 0 ... 3 entries with the largest sum in the last column; all-zero
    values; a NaN column beside finite ones (before and after the largest finite one); an Inf column."""
    rng = np.random.default_rng(seed)
    out = {}

    def build(n):
        lens = rng.integers(0, 4, size=n)
        if n:
            lens[-1] = 3
        Ap = np.zeros(n + 1, dtype=np.int32); Ap[1:] = np.cumsum(lens)
        Ax = rng.uniform(-1.0, 1.0, size=Ap[-1])
        if n:
            Ax[Ap[n - 1]:] = [-1.25, 1.5, -1.0]              # 3.75 > 3 * 1.0
        return Ap, Ax

    for n in NORM_COLUMNS:
        Ap, Ax = build(n)
        out["n%d" % n] = (n, Ap, Ax, {"largest_column": n - 1 if n else None})
    Ap, Ax = build(37)
    out["zeros"] = (37, Ap, np.zeros_like(Ax), {"norm": 0.0})
    Ap, Ax = build(1500)
    Ax1 = Ax.copy(); Ax1[Ap[700]] = np.nan                  # (an empty column 700: then the next stored entry, still one column)
    out["nan"] = (1500, Ap, Ax1, {"nan_entry": int(Ap[700])})
    Ax2 = Ax.copy(); Ax2[-1] = np.nan                       # the NaN in the last column: the largest finite sum comes first
    out["nan last"] = (1500, Ap, Ax2, {"nan_entry": len(Ax2) - 1})
    Ax3 = Ax.copy(); Ax3[Ap[700]] = 1.0; Ax3[Ap[1200]] = -np.inf
    out["inf"] = (1500, Ap, Ax3, {"norm": np.inf})
    return out


# ---- 7. find_islands -----------------------------------------------------------------------------------------------------

def _symmetric_pattern(n, a, b, extra_rows=(), extra_cols=()):
    """The pattern with entries (a, b) and (b, a), rows of a column ascending, plus the given entries as they are."""
    rows = np.concatenate([a, b, np.asarray(extra_rows, dtype=np.int64)]).astype(np.int64)
    cols = np.concatenate([b, a, np.asarray(extra_cols, dtype=np.int64)]).astype(np.int64)
    order = np.lexsort((rows, cols))
    Ap = np.zeros(n + 1, dtype=np.int32); Ap[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return Ap, i32(rows[order])


def island_cases(n=3000):
    """name -> (n, Ap, Ai, claims)."""
    out = {}
    spokes = np.arange(n - 1)
    Ap, Ai = _symmetric_pattern(n, spokes, np.full(n - 1, n - 1))
    out["star hub last"] = (n, Ap, Ai, {"symmetric": True, "islands": 1, "hub": n - 1})
    Ap, Ai = _symmetric_pattern(n, spokes + 1, np.zeros(n - 1, dtype=np.int64))
    out["star hub first"] = (n, Ap, Ai, {"symmetric": True, "islands": 1, "hub": 0})
    # a path visiting n-1, 0, n-2, 1, ...: neighbours alternate between the two ends of the numbering
    seq = np.empty(n, dtype=np.int64); seq[0::2] = n - 1 - np.arange((n + 1) // 2); seq[1::2] = np.arange(n // 2)
    Ap, Ai = _symmetric_pattern(n, seq[:-1], seq[1:])
    out["zigzag path"] = (n, Ap, Ai, {"symmetric": True, "islands": 1, "sequence": seq})
    # a complete binary tree, heap position h numbered nt - 1 - h: leaves first, the root last
    nt = 4095
    h = np.arange(1, nt)
    Ap, Ai = _symmetric_pattern(nt, nt - 1 - h, nt - 1 - (h - 1) // 2)
    out["binary tree"] = (nt, Ap, Ai, {"symmetric": True, "islands": 1, "root": nt - 1})
    # two rings joined by one edge, and the same without it
    half = n // 2
    ring = lambda lo, k: (lo + np.arange(k), lo + (np.arange(k) + 1) % k)      # noqa: E731
    a1, b1 = ring(0, half); a2, b2 = ring(half, n - half)
    Ap, Ai = _symmetric_pattern(n, np.concatenate([a1, a2, [half - 1]]), np.concatenate([b1, b2, [n - 1]]))
    out["two rings joined"] = (n, Ap, Ai, {"symmetric": True, "islands": 1})
    Ap, Ai = _symmetric_pattern(n, np.concatenate([a1, a2]), np.concatenate([b1, b2]))
    out["two rings apart"] = (n, Ap, Ai, {"symmetric": True, "islands": 2})
    # ten rings of n / 10 nodes with chords, symmetric, then one entry of the last column dropped (the last one): the entry
    # left without a mirror is (n - 1, i), in column i ...
    k = n // 10
    parts = [ring(lo, k) for lo in range(0, n, k)]
    a = np.concatenate([p[0] for p in parts] + [np.arange(0, n - 2 * k, 3)])
    b = np.concatenate([p[1] for p in parts] + [np.arange(0, n - 2 * k, 3) + k])
    Ap0, Ai0 = _symmetric_pattern(n, a, b)
    Ap = Ap0.copy(); Ap[n] -= 1
    dropped = (int(Ai0[-1]), n - 1)
    out["last entry dropped"] = (n, Ap, Ai0[:-1].copy(), {"symmetric": False, "dropped": dropped})
    # ... and every pass of that ring still reaches every node, so the islands do not tell which kernels ran.  Here they
    # do: the last node hangs off node n - 2 alone, and the entry (n - 1, n - 2) is dropped from column n - 2.  The only
    # entry without a mirror is (n - 2, n - 1), the only one of the last column and the very last one that
    # k_pattern_symmetric looks at; nothing reaches the last node any more, so it is an island of its own, while a
    # symmetric treatment would leave it with the last ring (which no chord joins to the other nine).
    parts = [ring(lo, k) for lo in range(0, n - k, k)] + [ring(n - k, k - 1)]
    a = np.concatenate([p[0] for p in parts] + [np.arange(0, n - 2 * k, 3), [n - 2]])
    b = np.concatenate([p[1] for p in parts] + [np.arange(0, n - 2 * k, 3) + k, [n - 1]])
    Ap0, Ai0 = _symmetric_pattern(n, a, b)
    at = int(Ap0[n - 2] + np.flatnonzero(Ai0[Ap0[n - 2]:Ap0[n - 1]] == n - 1)[0])
    Ap = Ap0.copy(); Ap[n - 1:] -= 1
    out["mirror of last entry dropped"] = (n, Ap, np.delete(Ai0, at), {"symmetric": False, "islands": 3, "dropped": (n - 1, n - 2),
                                                                     "lonely": (n - 2, n - 1)})
    # self-loops on every third node and every ring edge stored twice
    a, b = ring(0, 500); a2, b2 = ring(500, 700)
    aa = np.concatenate([a, a, a2, a2]); bb = np.concatenate([b, b, b2, b2])
    loops = np.arange(0, 1500, 3)
    Ap, Ai = _symmetric_pattern(1500, aa, bb, loops, loops)
    out["loops duplicates"] = (1500, Ap, Ai, {"symmetric": True, "islands": 2 + 300})
    return out


# ---- 8. stacking ----------------------------------------------------------------------------------------------------------

def _block(rng, m, lengths):
    cols = [list(rng.choice(m, size=L, replace=False)) if L else [] for L in lengths]
    Ap, Ai = csc_from_columns(cols)
    return m, len(lengths), Ai, Ap, values(rng, len(Ai))


def stack_cases(seed=51):
    """name -> ([A, B, C, D] as (m, n, indices, indptr, data), claims).  In "edges" every block has columns of 0, 1, 63,
    64, 65 and 200 entries, paired so that every length of the upper block meets another length of the lower one, and two
    columns are long in both."""
    rng = np.random.default_rng(seed)
    L = list(EDGE_LENGTHS)
    rot = lambda k: L[k:] + L[:k]                                                      # noqa: E731
    out = {}
    out["edges"] = ([_block(rng, 256, L + rot(1) + [200, 65]), _block(rng, 256, rot(2) + L), _block(rng, 230, rot(3) + rot(5) + [200, 65]),
                     _block(rng, 230, rot(4) + rot(1))], {"lengths": L})
    small = [3, 0, 65, 1]
    out["an=0"] = ([_block(rng, 90, []), _block(rng, 90, small), _block(rng, 70, []), _block(rng, 70, small[::-1])], {})
    out["bn=0"] = ([_block(rng, 90, small), _block(rng, 90, []), _block(rng, 70, small[::-1]), _block(rng, 70, [])], {})
    out["am=0"] = ([_block(rng, 0, [0] * 4), _block(rng, 0, [0] * 3), _block(rng, 70, small), _block(rng, 70, small[:3])], {})
    out["cm=0"] = ([_block(rng, 90, small), _block(rng, 90, small[:3]), _block(rng, 0, [0] * 4), _block(rng, 0, [0] * 3)], {})
    out["C empty"] = ([_block(rng, 90, small), _block(rng, 90, small[:3]), _block(rng, 70, [0] * 4), _block(rng, 70, [64, 2, 0])], {})
    return out


def stack_restated(blocks):
    """-> (m, n, Pi, Pp, Px, map): column j < an is A(:, j) then C(:, j) shifted by am; column an + j is B(:, j) then
    D(:, j); map[p] = position of the entry in the concatenation A | B | C | D of the value arrays."""
    (am, an, Ai, Ap, Ax), (_, bn, Bi, Bp, Bx), (cm, _, Ci, Cp, Cx), (_, _, Di, Dp, Dx) = blocks
    offs = np.cumsum([0, len(Ax), len(Bx), len(Cx)])
    Pi, Px, mp, Pp = [], [], [], [0]
    for (Tp, Ti, Tx, o1), (Up, Ui, Ux, o2), ncol in (((Ap, Ai, Ax, offs[0]), (Cp, Ci, Cx, offs[2]), an),
                                                     ((Bp, Bi, Bx, offs[1]), (Dp, Di, Dx, offs[3]), bn)):
        for j in range(ncol):
            s, e = int(Tp[j]), int(Tp[j + 1]); s2, e2 = int(Up[j]), int(Up[j + 1])
            Pi += [Ti[s:e], Ui[s2:e2] + am]; Px += [Tx[s:e], Ux[s2:e2]]
            mp += [o1 + np.arange(s, e), o2 + np.arange(s2, e2)]
            Pp.append(Pp[-1] + (e - s) + (e2 - s2))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)   # noqa: E731
    return am + cm, an + bn, cat(Pi, np.int32), i32(Pp), cat(Px, np.float64), cat(mp, np.int32)


def restack_pass_plus_one(seed=52):
    """nnz = 4096 * 256 + 1 for restack_values_dev: a random map into four value arrays of unequal length whose last entry
    is the only one that reads the last value of D.  -> (map, (Ax, Bx, Cx, Dx), claims)."""
    rng = np.random.default_rng(seed)
    nnz = ONE_PASS + 1
    sizes = (300001, 1, 448575, 300000)
    assert sum(sizes) == nnz
    parts = tuple(rng.standard_normal(s) for s in sizes)
    mp = rng.permutation(nnz - 1).astype(np.int32)
    mp = np.concatenate([mp, [nnz - 1]]).astype(np.int32)
    return mp, parts, {"nnz": nnz, "sizes": sizes, "seams": [0, sizes[0], sizes[0] + sizes[1], sum(sizes[:3]), nnz - 1]}


# ---- 9. general triangular solves -------------------------------------------------------------------------------------------

def _tri_from_entries(n, rows, cols, vals, diag, lower):
    """CSC with the diagonal first (lower) or last (upper) in every column and the other rows in the order given."""
    Ap = np.zeros(n + 1, dtype=np.int32); Ai, Ax = [], []
    order = np.argsort(cols, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    cut = np.searchsorted(cols, np.arange(n + 1))
    for j in range(n):
        r, v = list(rows[cut[j]:cut[j + 1]]), list(vals[cut[j]:cut[j + 1]])
        Ai += ([j] + r) if lower else (r + [j]); Ax += ([diag[j]] + v) if lower else (v + [diag[j]])
        Ap[j + 1] = len(Ai)
    return Ap, i32(Ai), np.array(Ax, dtype=np.float64)


def tri_dense(n, Gp, Gi, Gx):
    G = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        for p in range(Gp[j], Gp[j + 1]):
            G[Gi[p], j] += Gx[p]
    return G


def tri_solve_longdouble(G, B, lower):
    """Dense substitution in np.longdouble (64-bit significand on x86): the reference solution of G x = b."""
    n = G.shape[0]
    X = np.array(B, dtype=np.longdouble).reshape(n, -1)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        sl = slice(0, i) if lower else slice(i + 1, n)
        X[i] = (X[i] - G[i, sl] @ X[sl]) / G[i, i]
    return X.reshape(np.shape(B))


def tri_edges(seed=61, n=300):
    """A lower triangular L of order 300 in which both rows and columns have 0, 1, 63, 64, 65 and 200 off-diagonal entries
    (rows feed lsolve / utsolve, columns ltsolve / usolve), rows of a column unsorted after the diagonal; U = L' with the
    diagonal last.  Off-diagonals of a row add up to at most 0.5 |diagonal|.  -> (n, L, U, claims) with L, U = (p, i, x)."""
    rng = np.random.default_rng(seed)
    big = (63, 64, 65, 200)
    ent = set()
    free = np.arange(6, n - 6)                               # rows / columns that take the long lines' entries
    for t, L in enumerate(big):
        r = n - 1 - t                                        # long rows at the bottom ...
        ent |= {(r, int(c)) for c in rng.choice(free[free < r], size=L, replace=False)}
        c = t                                                # ... long columns on the left
        ent |= {(int(rr), c) for rr in rng.choice(free[free > c], size=L, replace=False)}
    ent |= {(5, 4), (n - 5, n - 6)}                          # row 5 and column n - 6: exactly one (rows 4, 5 and columns n - 6, n - 5 take nothing else)
    rows = np.array([e[0] for e in ent]); cols = np.array([e[1] for e in ent])
    perm = rng.permutation(len(rows))
    rows, cols = rows[perm], cols[perm]
    diag = rng.uniform(1.0, 2.0, size=n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    rowcount = np.bincount(rows, minlength=n)
    vals = rng.uniform(-0.5, 0.5, size=len(rows)) / rowcount[rows]
    L = _tri_from_entries(n, rows, cols, vals, diag, True)
    U = _tri_from_entries(n, cols, rows, vals, diag, False)
    return n, L, U, {"row_counts": rowcount, "col_counts": np.bincount(cols, minlength=n), "lengths": EDGE_LENGTHS}


def tri_small_cases(seed=62):
    """name -> (n, L, U, claims): n = 1, a pure diagonal, a bidiagonal chain of 1500 (one row per level)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, n, chain in (("n=1", 1, False), ("diagonal", 77, False), ("chain", 1500, True)):
        diag = rng.uniform(1.0, 2.0, size=n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        rows = np.arange(1, n) if chain else np.zeros(0, dtype=np.int64)
        cols = rows - 1
        vals = rng.uniform(-0.5, 0.5, size=len(rows))
        out[name] = (n, _tri_from_entries(n, rows, cols, vals, diag, True), _tri_from_entries(n, cols, rows, vals, diag, False),
                     {"levels": n if chain else 1})
    return out


def tri_levels(n, Gp, Gi, lower, trans):
    """Number of levels of the solve's dependency graph (a row waits for every row it reads)."""
    dep = [[] for _ in range(n)]
    for j in range(n):
        for p in range(Gp[j], Gp[j + 1]):
            i = int(Gi[p])
            if i != j:
                (dep[j] if trans else dep[i]).append(i if trans else j)
    level = np.zeros(n, dtype=np.int64)
    forward = lower != trans
    for i in (range(n) if forward else range(n - 1, -1, -1)):
        level[i] = 1 + max((level[d] for d in dep[i]), default=-1)
    return int(level.max()) + 1 if n else 0


TRI_SOLVES = (("lsolve", True, False), ("usolve", False, False), ("ltsolve", True, True), ("utsolve", False, True))


def tri_references(orc, n, L, U, seed=63, ks=(1, 3)):
    """For every solve and k: the right-hand side, the np.longdouble solution and the error of the oracle's cs_lsolve-family
    result against it (max |x - x_ld| / max |x_ld|): the yardstick of the device bound, measured, not hard-coded.
    -> {(solve, k): (B, X_ld, oracle_err)}."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, lower, trans in TRI_SOLVES:
        Gp, Gi, Gx = L if lower else U
        G = tri_dense(n, Gp, Gi, Gx)
        for k in ks:
            B = rng.standard_normal((n, k)) if k > 1 else rng.standard_normal(n)
            X = tri_solve_longdouble(G.T if trans else G, B, lower != trans)
            Xo = np.empty_like(B)
            for t in range(k):
                x = np.ascontiguousarray(B[:, t] if k > 1 else B).copy()
                getattr(orc, "csc_%s_f" % name)(n, Gp, Gi, Gx, x)
                if k > 1:
                    Xo[:, t] = x
                else:
                    Xo = x
            err = float(np.abs(Xo - X).max() / np.abs(X).max())
            out[(name, k)] = (B, X, err)
    return out


# ---- 10. resident matvec / residual / refine ------------------------------------------------------------------------------

RESIDENT_N, RESIDENT_K = 65537, 17                           # n * k = 1 114 129 > 4096 * 256 > 2048 * 256


def resident_matrix(seed=71, n=RESIDENT_N, empty_row=True):
    """A banded n x n matrix (diagonal, +-1, +-3; strictly diagonally dominant) with one row of 200 entries and -- for the
    products only -- one row and one column without any entry.  -> (n, Ap, Ai, Ax, claims)."""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.int64)
    rows = [j]; cols = [j]
    for d in (1, 3):
        rows += [j[d:], j[:-d]]; cols += [j[:-d], j[d:]]
    long_row = n // 3
    lc = rng.choice(np.setdiff1d(np.arange(n), np.arange(long_row - 3, long_row + 4)), size=200 - 5, replace=False)
    rows.append(np.full(len(lc), long_row)); cols.append(lc)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    hole = 2 * n // 3
    if empty_row:
        keep = (rows != hole) & (cols != hole)
        rows, cols = rows[keep], cols[keep]
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    vals = rng.uniform(-1.0, 1.0, size=len(rows))
    vals[rows == long_row] *= 0.02
    vals[rows == cols] = rng.uniform(8.0, 9.0, size=int((rows == cols).sum()))
    Ap = np.zeros(n + 1, dtype=np.int32); Ap[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return n, Ap, i32(rows), vals, {"long_row": long_row, "long_row_entries": 200, "empty_row": hole if empty_row else None}


def matvec_restated(n, Ap, Ai, Ax, X, trans=False):
    """Y = A X (A' X) summed as csc_mat_vec_ff sums: ascending column inside a row (storage order inside a column for A'),
    the product rounded, then the sum."""
    cols = columns_of(Ap).astype(np.int64)
    out_idx, in_idx = (cols, Ai.astype(np.int64)) if trans else (Ai.astype(np.int64), cols)
    order = np.argsort(out_idx, kind="stable")
    out_idx, in_idx, v = out_idx[order], in_idx[order], Ax[order]
    start = np.searchsorted(out_idx, np.arange(n))
    rank = np.arange(len(out_idx)) - start[out_idx]
    Y = np.zeros((n,) + X.shape[1:])
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == r
        prod = v[sel].reshape((-1,) + (1,) * (X.ndim - 1)) * X[in_idx[sel]]
        Y[out_idx[sel]] = Y[out_idx[sel]] + prod
    return Y
