"""Plain Python restatement of the sparse product's definition (include/csparse3_amd.h, "sparse products"): the loops of
the reference's csc_multiply_ff with the workspaces sized by the ROWS of C, so that every shape works (the reference sizes
them by the columns and only runs when Am <= Bn).  tests/test_spgemm_cpu.py pins it to the reference's recorded outputs
bit for bit; the GPU tests then use it where no recorded output can exist."""
import numpy as np


def multiply(Am, An, Ap, Ai, Ax, Bm, Bn, Bp, Bi, Bx):
    """-> (Cm, Cn, Cp, Ci, Cx, nnz): rows of a column in order of first occurrence, sums left to right, the first product
    stored as it is, every product rounded on its own (Python floats: no fused multiply-add)."""
    assert An == Bm
    w = np.zeros(Am, dtype=np.int64)
    x = np.zeros(Am, dtype=np.float64)
    Cp = np.zeros(Bn + 1, dtype=np.int32)
    Ci, Cx = [], []
    for j in range(Bn):
        start = len(Ci)
        for pb in range(Bp[j], Bp[j + 1]):
            k = Bi[pb]
            b = float(Bx[pb])
            for pa in range(Ap[k], Ap[k + 1]):
                i = Ai[pa]
                v = b * float(Ax[pa])
                if w[i] < j + 1:
                    w[i] = j + 1
                    Ci.append(i)
                    x[i] = v
                else:
                    x[i] = x[i] + v
        Cx.extend(x[i] for i in Ci[start:])
        Cp[j + 1] = len(Ci)
    return Am, Bn, Cp, np.array(Ci, dtype=np.int32), np.array(Cx, dtype=np.float64), len(Ci)


def transpose(m, n, Ap, Ai, Ax):
    """-> (n, m, Tp, Ti, Tx): rows of A as columns, entries in ascending column of A, duplicates in stored order."""
    Tp = np.zeros(m + 1, dtype=np.int32)
    for p in range(Ap[n]):
        Tp[Ai[p] + 1] += 1
    Tp = np.cumsum(Tp).astype(np.int32)
    w = Tp[:-1].copy()
    Ti = np.empty(Ap[n], dtype=np.int32)
    Tx = np.empty(Ap[n], dtype=np.float64)
    for j in range(n):
        for p in range(Ap[j], Ap[j + 1]):
            q = w[Ai[p]]
            w[Ai[p]] += 1
            Ti[q] = j
            Tx[q] = Ax[p]
    return n, m, Tp, Ti, Tx


def multiply_t(Am, An, Ap, Ai, Ax, Bm, Bn, Bp, Bi, Bx):
    """C = A' B: transpose, then multiply."""
    Tm, Tn, Tp, Ti, Tx = transpose(Am, An, Ap, Ai, Ax)
    return multiply(Tm, Tn, Tp, Ti, Tx, Bm, Bn, Bp, Bi, Bx)


def bits(x):
    """The raw 64-bit patterns of a float64 array: -0.0 and 0.0 differ, NaNs compare by payload."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
