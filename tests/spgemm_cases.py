"""Inputs of the sparse-product tests: the recorded cases of tests/golden/spgemm.npz and matrices engineered to sit at the
edges of the device paths (built from cs3_spgemm_limits, so they stay at the edges when a constant moves).  No GPU here;
tests/test_spgemm_cpu.py checks the generators themselves."""
import os

import numpy as np

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spgemm.npz"))
GOLD_CASES = [str(t) for t in GOLD["cases"]]
KEYS = ("Am", "An", "Ap", "Ai", "Ax", "Bm", "Bn", "Bp", "Bi", "Bx")


def golden(tag):
    """-> (args of csc_multiply_ff, transpose_a, (Cp, Ci, Cx) of the reference)."""
    args = tuple(int(GOLD[tag + "_" + k]) if k in ("Am", "An", "Bm", "Bn") else GOLD[tag + "_" + k] for k in KEYS)
    return args, bool(GOLD[tag + "_ta"]), (GOLD[tag + "_Cp"], GOLD[tag + "_Ci"], GOLD[tag + "_Cx"])


def csc_from_columns(m, columns, values=None):
    """CSC arrays from a list of row lists (stored order kept, duplicates kept)."""
    Ap = np.zeros(len(columns) + 1, dtype=np.int32)
    Ap[1:] = np.cumsum([len(c) for c in columns])
    Ai = np.array([i for c in columns for i in c], dtype=np.int32)
    assert Ai.size == 0 or (Ai.min() >= 0 and Ai.max() < m)
    return Ap, Ai, values


def random_csc(rng, m, n, density):
    mask = rng.random((n, m)) < density
    cols = [list(np.flatnonzero(mask[j])) for j in range(n)]
    Ap, Ai, _ = csc_from_columns(m, cols)
    return Ap, Ai, rng.standard_normal(Ai.size)


def engineered_columns(rng, specs, per_col, Am):
    """One column of C per (T, D) in specs: exactly T products on exactly D distinct rows.  A is blocks of columns side by
    side, block i holding T products in columns of per_col entries (the last one shorter), product k of the block at row
    rowmap[perm(k) mod D]; column i of B selects the columns of block i in order.  per_col > 1 makes chunks of 64 products
    straddle columns of A and, when D < per_col, puts duplicate rows inside one column of A.
    -> (args of csc_multiply_ff, [(T, D)] as built)."""
    a_cols, b_cols = [], []
    for T, D in specs:
        assert 1 <= D <= T and D <= Am
        rowmap = rng.choice(Am, size=D, replace=False)
        perm = rng.permutation(T)
        rows = [int(rowmap[perm[k] % D]) for k in range(T)]
        assert len(set(rows)) == D
        first = len(a_cols)
        a_cols += [rows[k:k + per_col] for k in range(0, T, per_col)]
        b_cols.append(list(range(first, len(a_cols))))
    An = len(a_cols)
    Ap, Ai, _ = csc_from_columns(Am, a_cols)
    Bp, Bi, _ = csc_from_columns(An, b_cols)
    return (Am, An, Ap, Ai, rng.standard_normal(Ai.size), An, len(b_cols), Bp, Bi, rng.standard_normal(Bi.size)), list(specs)


def symbolic_edge_specs(lim):
    """(T, D): T at the capacity c of the LDS path (c - 1, c, c + 1), D = 1, T and the table's row capacity."""
    c, cap = int(lim.lds_products), int(lim.lds_table_rows)
    specs = []
    for T in (c - 1, c, c + 1):
        for D in sorted({1, T, min(T, cap)}):
            specs.append((T, D))
    return specs


def chunk_edge_specs():
    """T = 63, 64, 65 products on 5 rows: with 7 entries per column of A, one column holds a row twice, and two lanes of
    one chunk of 64 hit the same row."""
    return [(63, 5), (64, 5), (65, 5)]


def column_of_n(rng, n):
    """C = diag * (one dense column): one column of C with n entries, lists of length 1."""
    Ap, Ai, _ = csc_from_columns(n, [[i] for i in range(n)])
    Bp, Bi, _ = csc_from_columns(n, [list(rng.permutation(n))])
    return n, n, Ap, Ai, rng.standard_normal(n), n, 1, Bp, Bi, rng.standard_normal(n)


def one_long_list(rng, length, others=63):
    """One column of C with 1 + others entries: the list of row 0 has `length` products, every other list one."""
    a_cols = [[0] for _ in range(length)] + [[1 + i] for i in range(others)]
    order = list(rng.permutation(len(a_cols)))
    Ap, Ai, _ = csc_from_columns(1 + others, a_cols)
    Bp, Bi, _ = csc_from_columns(len(a_cols), [order])
    return 1 + others, len(a_cols), Ap, Ai, rng.standard_normal(Ai.size), len(a_cols), 1, Bp, Bi, rng.standard_normal(Bi.size)


def dot_product(rng, K):
    """1 x K times K x 1: one entry of C, a list of K products."""
    Ap, Ai, _ = csc_from_columns(1, [[0] for _ in range(K)])
    Bp, Bi, _ = csc_from_columns(K, [list(range(K))])
    return 1, K, Ap, Ai, rng.standard_normal(K), K, 1, Bp, Bi, rng.standard_normal(K)


def empty_csc(n):
    return np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)


def degenerate_cases(rng):
    """name -> args: Bn = 0, inner dimension 0, Am = 0, all-empty A, all-empty B."""
    A = random_csc(rng, 6, 5, 0.5)
    B = random_csc(rng, 5, 7, 0.5)
    return {
        "Bn=0": (6, 5, *A, 5, 0, *empty_csc(0)),
        "inner=0": (6, 0, *empty_csc(0), 0, 7, *empty_csc(7)),
        "Am=0": (0, 5, *empty_csc(5), 5, 7, *B),
        "A empty": (6, 5, *empty_csc(5), 5, 7, *B),
        "B empty": (6, 5, *A, 5, 7, *empty_csc(7)),
    }


def tall_cases(rng):
    """Shapes with Am > Bn, which the reference cannot do."""
    return {
        "57x31.31x25": (57, 31, *random_csc(rng, 57, 31, 0.15), 31, 25, *random_csc(rng, 31, 25, 0.15)),
        "200x3.3x2": (200, 3, *random_csc(rng, 200, 3, 0.4), 3, 2, *random_csc(rng, 3, 2, 0.9)),
    }
