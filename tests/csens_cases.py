"""Operands and matrices for the tests of the complex sparse right-hand-side path and of complex Schur handles
(tests/test_csens_cpu.py, tests/test_gpu_csens.py, tests/test_gpu_cplx_schur.py): the operands of sens_cases with complex
values, and the small matrices the tests of the complex plan already use."""
import numpy as np

import cplx_cases
import sens_cases
from csparse3_amd import synth
from sens_ref import Op

BORDER = [37, 3, 11, 20, 5]


def cplx(op, seed):
    """The operand with every value turned by a phase of its own and, every fifth one, made purely real or imaginary
    (signed zeros in the other component)."""
    r = np.random.default_rng(seed)
    v = np.asarray(op.values, dtype=np.float64) * np.exp(1j * r.uniform(0, 2 * np.pi, len(op.values)))
    v[0::5] = np.asarray(op.values)[0::5] * (1.0 + 0.0j)
    v[2::5] = np.asarray(op.values)[2::5] * complex(-0.0, 1.0)
    return Op(op.ncols, op.indptr, op.indices, v.astype(np.complex128))


def incidence(n, ncols, seed):
    return cplx(sens_cases.incidence(n, ncols, seed), seed + 1)


def selection(idx):
    op = sens_cases.selection(idx)
    return Op(op.ncols, op.indptr, op.indices, op.values.astype(np.complex128))


def awkward(n, seed):
    """Six columns: empty, a duplicated index (twice, not neighbours), unsorted rows, a long column, empty, one entry."""
    r = np.random.default_rng(seed)
    a, b, c = (int(v) for v in r.choice(n, size=3, replace=False))
    long_rows, long_vals = sens_cases.long_column(n, min(n, 23), seed + 1)
    hi, mid, lo = sorted([a, b, c], reverse=True)
    cols = [([], []), ([a, b, a, a], [0.5, -1.25, 0.75, 1e-3]), ([hi, lo, mid], [1.0, 2.0, -3.0]),
            (long_rows, long_vals), ([], []), ([c], [1.5])]
    return cplx(sens_cases.from_columns(cols), seed + 2)


def ybus40():
    return synth.ybus(40, 60, seed=40)


def matrices():
    """name -> (n, Ap, Ai, Az [nnz], kind, rotate)."""
    out = {"ybus40": ybus40() + ("lu", True)}
    for name in ("unsorted", "absent_diagonal", "empty_column"):
        n, Ap, Ai = cplx_cases.structural_cases()[name]
        Az = cplx_cases.values_for(np.random.default_rng(len(name)), int(Ap[n]))[0]
        col = np.repeat(np.arange(n), np.diff(Ap))
        Az[Ai == col] += 6.0j                                            # an imaginary diagonal that dominates: the rotation matters
        out[name] = (n, Ap, Ai, Az, "lu", True)
    n, Ap, Ai, Az, _ = cplx_cases.diag_zoo(np.random.default_rng(11))
    out["diag_zoo"] = (n, Ap, Ai, Az[0], "lu", True)                     # (NaN and infinite diagonals: bits only, nothing to factorise)
    out["hermitian_pd"] = cplx_cases.hermitian_pd(40, 60, seed=3) + ("chol", False)
    return out


def banded(n, seed):
    """A complex tridiagonal matrix of order n with a mostly imaginary, dominant diagonal: any order for the edge tests."""
    r = np.random.default_rng(seed)
    cols, vals = [], []
    for j in range(n):
        rows = [i for i in (j - 1, j, j + 1) if 0 <= i < n]
        cols.append(rows)
        vals += [complex(0.3 * r.standard_normal(), 4.0 + r.uniform()) if i == j else complex(r.standard_normal(), r.standard_normal()) for i in rows]
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ap[1:] = np.cumsum([len(c) for c in cols])
    return n, Ap, np.array([i for c in cols for i in c], dtype=np.int32), np.array(vals, dtype=np.complex128)
