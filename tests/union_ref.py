"""NumPy restatement of the union plan (include/csparse3_amd.h, "union plans"): the union pattern through np.unique over
(column, row) keys, the slot of every member entry by a search in those keys, and the embedding of the values as the loop
the header defines -- over a member's entries in storage order into a row that starts as +0.0, the first source of a slot
stored as it is, later ones added."""
import numpy as np


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


def _keys(n, Ap, Ai):
    Ap = np.asarray(Ap, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    return cols * max(n, 1) + np.asarray(Ai, dtype=np.int64)[:Ap[n]]


def union_pattern(n, patterns):
    """-> (Up int32[n + 1], Ui int32[nnz_u], key int64[nnz_u]): column j holds the rows of column j of any member, ascending."""
    key = np.unique(np.concatenate([_keys(n, Ap, Ai) for Ap, Ai in patterns] + [np.empty(0, dtype=np.int64)]))
    Up = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n)[:n], out=Up[1:])
    return Up.astype(np.int32), (key % max(n, 1)).astype(np.int32), key


def slots(n, key, Ap, Ai):
    """-> int32[nnz_b]: where every entry of the member sits in the union."""
    return np.searchsorted(key, _keys(n, Ap, Ai)).astype(np.int32)


def embed_loop(n, patterns, values):
    """The definition, entry by entry.  values: one array per member.  -> float64[nmat, nnz_u]."""
    Up, Ui, key = union_pattern(n, patterns)
    out = np.zeros((len(patterns), len(key)), dtype=np.float64)            # +0.0 where a member has no source
    for b, ((Ap, Ai), v) in enumerate(zip(patterns, values)):
        sl = slots(n, key, Ap, Ai)
        v = np.ascontiguousarray(v, dtype=np.float64)
        seen = np.zeros(len(key), dtype=bool)
        row, rowbits = out[b], out[b].view(np.uint64)
        for e in range(len(sl)):
            s = sl[e]
            if not seen[s]:
                rowbits[s] = v.view(np.uint64)[e]                          # the first source: its bit pattern
                seen[s] = True
            else:
                row[s] = row[s] + v[e]                                     # later ones: plain additions, left to right
    return out


def embed(n, patterns, values):
    """embed_loop for large cases: slots with one source are copied in one vector assignment, only the entries of slots
    with several sources walk the loop (tests/test_union_cpu.py holds the two against each other)."""
    Up, Ui, key = union_pattern(n, patterns)
    out = np.zeros((len(patterns), len(key)), dtype=np.float64)
    for b, ((Ap, Ai), v) in enumerate(zip(patterns, values)):
        sl = slots(n, key, Ap, Ai)
        v = np.ascontiguousarray(v, dtype=np.float64)
        single = np.bincount(sl, minlength=len(key))[sl] == 1
        row, rowbits = out[b], out[b].view(np.uint64)
        rowbits[sl[single]] = v.view(np.uint64)[:len(sl)][single]
        seen = np.zeros(len(key), dtype=bool)
        for e in np.flatnonzero(~single):
            s = sl[e]
            if not seen[s]:
                rowbits[s] = v.view(np.uint64)[e]
                seen[s] = True
            else:
                row[s] = row[s] + v[e]
    return out
