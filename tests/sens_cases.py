"""Operands and matrices for the tests of the sparse right-hand-side path (tests/test_sens_cpu.py, tests/test_gpu_sens.py).

The operands are what the feature is for: incidence-like columns with one or two entries +-v (an injection at a bus, a
flow between two buses), selections (unit columns), and the structural edge cases -- empty columns, duplicates, unsorted
rows, long columns.  Each matrix is the smallest of its kind that the parity tests of the library already use."""
import numpy as np

from csparse3_amd import synth
from helpers import csc_to_scipy
import match_cases as mc
from sens_ref import Op


def incidence(n, ncols, seed, single_every=3):
    """ncols columns of two entries (+v, -v) at distinct rows, every `single_every`-th one a single entry +v; v in
    [0.5, 1.5)."""
    r = np.random.default_rng(seed)
    counts = np.where(np.arange(ncols) % single_every == single_every - 1, 1, 2) if n > 1 else np.ones(ncols, dtype=int)
    indptr = np.zeros(ncols + 1, dtype=np.int32)
    np.cumsum(counts, out=indptr[1:])
    first = r.integers(0, n, ncols)
    second = (first + 1 + r.integers(0, max(n - 1, 1), ncols)) % n            # distinct from first
    v = r.uniform(0.5, 1.5, ncols)
    indices = np.empty(indptr[-1], dtype=np.int32)
    values = np.empty(indptr[-1])
    indices[indptr[:-1]] = first
    values[indptr[:-1]] = v
    two = counts == 2
    indices[indptr[:-1][two] + 1] = second[two]
    values[indptr[:-1][two] + 1] = -v[two]
    return Op(ncols, indptr, indices, values)


def selection(idx):
    """Unit columns e_idx[c]."""
    idx = np.asarray(idx, dtype=np.int32)
    return Op(len(idx), np.arange(len(idx) + 1, dtype=np.int32), idx, np.ones(len(idx)))


def from_columns(cols):
    """An operand from a list of (rows, values) per column, kept in the order given."""
    indptr = np.zeros(len(cols) + 1, dtype=np.int32)
    np.cumsum([len(c[0]) for c in cols], out=indptr[1:])
    rows = [np.asarray(c[0], dtype=np.int32) for c in cols]
    vals = [np.asarray(c[1], dtype=np.float64) for c in cols]
    return Op(len(cols), indptr, np.concatenate(rows) if cols else np.zeros(0, np.int32),
              np.concatenate(vals) if cols else np.zeros(0))


def long_column(n, count, seed):
    """(rows, values): `count` distinct rows in random (unsorted) order."""
    r = np.random.default_rng(seed)
    return r.choice(n, size=count, replace=False), r.uniform(-1.0, 1.0, count)


def _spd(n):
    ei, ej = synth.spd_grid_pattern(n, seed=n)
    return synth.spd_grid_matrix(n, ei, ej, seed=n + 1)


def _matched():
    c = mc.case("kkt400")
    return c.n, c.n, c.Ap, c.Ai, c.Ax


# name -> (builder of (m, n, Ap, Ai, Ax), how the handle is made: "lu", "chol" or "match")
MATRICES = {
    "toy10": (lambda: synth.toy10()[:5], "lu"),
    "jacobian_like": (synth.jacobian_like, "lu"),
    "grid5000": (lambda: synth.grid_jacobian(5000), "lu"),
    "spd900": (lambda: _spd(900), "chol"),
    "kkt400": (_matched, "match"),
}
_BUILT = {}


def matrix(name):
    """(m, n, Ap, Ai, Ax, kind, scipy matrix), built once per process."""
    if name not in _BUILT:
        build, kind = MATRICES[name]
        m, n, Ap, Ai, Ax = build()
        _BUILT[name] = (m, n, Ap, Ai, Ax, kind, csc_to_scipy(m, n, Ap, Ai[:Ap[n]], Ax[:Ap[n]]).tocsc())
    return _BUILT[name]


def handle(hip, name):
    """An unfactorised handle of the case and the call that factorises it."""
    m, n, Ap, Ai, Ax, kind, _ = matrix(name)
    if kind == "chol":
        return hip.Factorization(m, n, Ap, Ai, kind=hip.CS3_CHOLESKY), lambda F: F.factor(Ax)
    if kind == "match":
        return hip.Factorization(m, n, Ap, Ai, match_values=Ax), lambda F: F.factor(Ax, 1e-3)
    return hip.Factorization(m, n, Ap, Ai), lambda F: F.factor(Ax, 1e-3)


def default_operands(name, k=40, p=24):
    """(B, Ct): k incidence columns and p incidence rows for the case."""
    n = matrix(name)[1]
    return incidence(n, k, seed=11), incidence(n, p, seed=13)
