"""Cases for the complex plan: small structural patterns, a matrix whose diagonal runs through every branch of the
rotation, a Hermitian positive definite matrix, and values to go with a pattern."""
import numpy as np

from csparse3_amd import synth


def _csc(n, cols):
    """cols: a list over the columns of row lists, kept in that order.  -> (n, Ap int32, Ai int32)."""
    assert len(cols) == n
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.cumsum([len(c) for c in cols])
    Ai = np.array([r for c in cols for r in c], dtype=np.int32)
    return n, Ap, Ai


def structural_cases():
    """name -> (n, Ap, Ai)."""
    out = {
        "n0": _csc(0, []),
        "n1": _csc(1, [[0]]),
        "n2": _csc(2, [[0, 1], [1, 0]]),
        "unsorted": _csc(5, [[3, 0, 1], [1, 4, 0], [2, 4, 3], [4, 3, 0, 2], [1, 4, 2]]),
        "absent_diagonal": _csc(4, [[1, 0], [0, 2], [3, 2, 1], [2, 0]]),                  # rows 1 and 3 have no (i, i)
        "diag_twice": _csc(3, [[0, 1, 0], [1, 2], [2, 0, 2, 2]]),
        "empty_column": _csc(4, [[0, 1], [], [2, 0], [3, 2]]),
    }
    n, Ap, Ai, _ = synth.ybus(40, 60, seed=40)
    out["ybus40"] = (n, Ap, Ai)
    return out


def values_for(rng, nnz, batch=1):
    """complex128 [batch, nnz], entries of order 1."""
    return rng.standard_normal((batch, nnz)) + 1j * rng.standard_normal((batch, nnz))


DIAG_KINDS = ("re", "im", "tie", "tie_neg", "neg", "zero", "neg_zero", "nan", "nan_im", "inf", "absent", "twice", "twice_cancel")


def diag_zoo(rng, batch=1):
    """A matrix with one row per branch of the rotation, off-diagonals around it (rows unsorted), signed zeros among the
    values.  Matrix b of the batch has the kinds rolled by b, so every matrix rotates every row differently.
    -> (n, Ap, Ai, Az [batch, nnz], kinds)."""
    n = len(DIAG_KINDS)
    stored = {"absent": 0, "twice": 2, "twice_cancel": 2}
    cols = []
    for j, kind in enumerate(DIAG_KINDS):                                                    # (the two (j, j) of "twice" are not neighbours)
        count = stored.get(kind, 1)
        cols.append([(j + 3) % n] + [j] * min(count, 1) + [(j + 1) % n] + [j] * (count == 2))
    n, Ap, Ai = _csc(n, cols)
    Az = values_for(rng, int(Ap[n]), batch)
    diag_val = {"re": [3.0 - 1.25j], "im": [0.5 + 4.0j], "tie": [2.0 - 2.0j], "tie_neg": [-1.5 - 1.5j], "neg": [-5.0 + 0.25j],
                "zero": [0.0 + 0.0j], "neg_zero": [complex(-0.0, -0.0)], "nan": [complex(np.nan, 1.0)], "nan_im": [complex(2.0, np.nan)],
                "inf": [complex(1.0, -np.inf)], "twice": [1e16 + 1.0j, 1.0 - 3.0j], "twice_cancel": [2.5 - 1.0j, -2.5 + 1.0j]}
    for b in range(batch):
        for j in range(n):
            kind = DIAG_KINDS[(j + b) % n]
            pos = [p for p in range(Ap[j], Ap[j + 1]) if Ai[p] == j]
            vals = diag_val.get(kind, [])
            for t, p in enumerate(pos):                                                      # (a row without a stored diagonal stays so)
                Az[b, p] = vals[t % len(vals)] if vals else 1.0 + 1.0j
                if kind == "twice_cancel" and len(pos) == 1:
                    Az[b, p] = 0.0
    off = [p for j in range(n) for p in range(Ap[j], Ap[j + 1]) if Ai[p] != j]
    for b in range(batch):
        Az[b, off[0]] = complex(0.0, -0.0)
        Az[b, off[1]] = complex(-0.0, 0.0)
        Az[b, off[2]] = complex(-0.0, -0.0)
        Az[b, off[3]] = complex(0.0, 1.0)
    return n, Ap, Ai, Az, DIAG_KINDS


def diagonal_matrix(n, rng):
    """The cheapest matrix with n entries: for the grid-stride edge."""
    Ap = np.arange(n + 1, dtype=np.int32)
    Ai = np.arange(n, dtype=np.int32)
    return n, Ap, Ai, values_for(rng, n)


def hermitian_pd(nbus, nedges, seed):
    """A Hermitian positive definite matrix on the pattern of ybus(nbus, nedges): off-diagonals a_ij = conj(a_ji) of
    magnitude below 1, a real diagonal above the row sums.  -> (n, Ap, Ai, Az), full storage."""
    n, Ap, Ai, _ = synth.ybus(nbus, nedges, seed)
    rng = np.random.default_rng(seed + 1)
    col = np.repeat(np.arange(n), np.diff(Ap))
    lo, hi = np.minimum(Ai, col).astype(np.int64), np.maximum(Ai, col).astype(np.int64)
    key = lo * n + hi
    uniq, inv = np.unique(key, return_inverse=True)
    w = rng.uniform(0.1, 0.7, len(uniq)) * np.exp(1j * rng.uniform(0, 2 * np.pi, len(uniq)))
    Az = w[inv]
    Az = np.where(Ai > col, np.conj(Az), Az)                                                 # lower triangle = conj(upper)
    rowsum = np.zeros(n)
    offd = Ai != col
    np.add.at(rowsum, Ai[offd], np.abs(Az[offd]))
    Az[~offd] = rowsum[Ai[~offd]] + 1.0
    return n, Ap, Ai, Az.astype(np.complex128)


def norm1(n, Ap, Az):
    col = np.repeat(np.arange(n), np.diff(Ap[:n + 1]))
    s = np.zeros(n)
    np.add.at(s, col, np.abs(np.asarray(Az)[:Ap[n]]))
    return float(s.max()) if n else 0.0
