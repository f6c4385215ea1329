"""References for the bilinear forms on the selected inverse (cs3_quad_*): the dense inverse, a NumPy restatement of the
term map on the position function of tests/selinv_ref.py, and NumPy restatements of the three summation orders and of
omega, rn, the arg-max and J -- the arithmetic quadform.hip does, operation for operation, so that results can be compared
bit for bit.  Used by tests/test_quad_cpu.py and tests/test_gpu_quad.py.

Operands are rows: (m, indptr, indices) is the CSC pattern of the transposed operand, values in that entry order.
"""
import numpy as np

import selinv_ref

BOUND = selinv_ref.BOUND      # |t - t_ref| <= BOUND * sum |c_a| |Z_ref(a, b)| |b_b| per row
COND_MAX = selinv_ref.COND_MAX


# -- the term map

def position_function(hip, F):
    """position(k, l): the offset of Z(k, l), k and l in pivot order, in the handle's block of Z, restated as
    selinv_ref.restated_positions lays it out (the fronts' r x r blocks back to back in the order they are computed; the
    block of the front of min(k, l), at the positions of the two labels in its structure); None outside the pattern."""
    sn_ptr, _, _, st = selinv_ref.fronts(hip, F)
    front = F.selinv_plan()[0]
    z_off, total = {}, 0
    for s in front:
        z_off[int(s)] = total
        total += len(st[int(s)]) ** 2
    col2sn = np.repeat(np.arange(len(st)), np.diff(sn_ptr))
    at = [{int(v): i for i, v in enumerate(rows)} for rows in st]

    def position(k, l):
        s = int(col2sn[min(k, l)])
        if k not in at[s] or l not in at[s]:
            return None
        return z_off[s] + at[s][k] + at[s][l] * len(st[s])

    return position


def classes(limits, counts):
    """0 lane, 1 wave, 2 workgroup, by the term count."""
    counts = np.asarray(counts)
    return np.where(counts <= limits.lane_max_terms, 0, np.where(counts <= limits.wave_max_terms, 1, 2)).astype(np.int32)


def term_counts(Ct, Bt):
    Bt = Ct if Bt is None else Bt
    return np.diff(np.asarray(Ct[1], dtype=np.int64)) * np.diff(np.asarray(Bt[1], dtype=np.int64))


def term_pairs(Ct, Bt):
    """(row, a, b) of every term in the plan's order: rows in order, a-major; a and b index the entry arrays."""
    Bt = Ct if Bt is None else Bt
    m = int(Ct[0])
    rows, ea, eb = [], [], []
    for i in range(m):
        a = np.arange(Ct[1][i], Ct[1][i + 1])
        b = np.arange(Bt[1][i], Bt[1][i + 1])
        ea.append(np.repeat(a, len(b)))
        eb.append(np.tile(b, len(a)))
        rows.append(np.full(len(a) * len(b), i))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    return cat(rows), cat(ea), cat(eb)


def restated_plan(hip, F, Ct, Bt, limits):
    """(row_class, term_ptr, term_pos) as cs3_debug_quad_plan hands them out; an off-pattern pair: (row, col_c, col_b)."""
    position = position_function(hip, F)
    pinv = F.ordering()["pinv"]
    _, ea, eb = term_pairs(Ct, Bt)
    ci, bi = np.asarray(Ct[2]), np.asarray((Ct if Bt is None else Bt)[2])
    counts = term_counts(Ct, Bt)
    term_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos = np.empty(len(ea), dtype=np.int64)
    for u in range(len(ea)):
        p = position(int(pinv[ci[ea[u]]]), int(pinv[bi[eb[u]]]))
        if p is None:
            return int(np.searchsorted(term_ptr, u, side="right") - 1), int(ci[ea[u]]), int(bi[eb[u]])
        pos[u] = p
    return classes(limits, counts), term_ptr, pos


# -- the sums

def _sequential(x):
    """s = 0; s += x[0]; s += x[1]; ..."""
    return np.cumsum(np.concatenate([[0.0], x]))[-1]


def _tree(v):
    """64 lanes: lane l += lane l + off for l < off, off = 32, 16, ..., 1; lane 0."""
    v = np.asarray(v, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:off] + v[off:2 * off]
    return v[0]


def _waves(s):
    """256 threads: the tree inside each wave, then the four waves in order."""
    S = [_tree(s[64 * v:64 * v + 64]) for v in range(4)]
    return ((S[0] + S[1]) + S[2]) + S[3]


def _strided(terms, nthreads):
    """thread j: the sequential sum of terms j, j + nthreads, ..."""
    return np.array([_sequential(terms[j::nthreads]) for j in range(nthreads)])


def row_sum(terms, cls):
    """One row's rounded terms, summed as its class does."""
    if cls == 0:
        return _sequential(terms)
    if cls == 1:
        return _tree(_strided(terms, 64))
    return _waves(_strided(terms, 256))


def restated_forms(Ct, Bt, Cx, Bx, zterm, row_class):
    """t [m]: every term (c * z) * b with both products rounded, the rows summed in the order of their class.  zterm: Z at
    every term, in the plan's order."""
    m = int(Ct[0])
    Bx = Cx if Bt is None else Bx
    _, ea, eb = term_pairs(Ct, Bt)
    terms = (np.asarray(Cx)[ea] * zterm) * np.asarray(Bx)[eb]
    ptr = np.concatenate([[0], np.cumsum(term_counts(Ct, Bt))])
    return np.array([row_sum(terms[ptr[i]:ptr[i + 1]], int(row_class[i])) for i in range(m)])


def z_at_terms(Zdense, Ct, Bt):
    """Z(Cti[a], Bti[b]) at every term from a dense [n, n] array in the caller's labels."""
    _, ea, eb = term_pairs(Ct, Bt)
    return Zdense[np.asarray(Ct[2])[ea], np.asarray((Ct if Bt is None else Bt)[2])[eb]]


def scatter_entries(n, Ap, Ai, Zx):
    """inverse_entries() as a dense [n, n] array, NaN off the pattern of A."""
    Z = np.full((n, n), np.nan)
    nz = int(Ap[n])
    Z[np.asarray(Ai[:nz]), np.repeat(np.arange(n), np.diff(Ap))] = Zx
    return Z


def dense_forms(Zref, Ct, Bt, Cx, Bx):
    """(t_ref, scale): t_ref [m] from the dense inverse, scale [m] = sum |c_a| |Z_ref(a, b)| |b_b|."""
    m = int(Ct[0])
    Bx = Cx if Bt is None else Bx
    rows, ea, eb = term_pairs(Ct, Bt)
    terms = np.asarray(Cx)[ea] * z_at_terms(Zref, Ct, Bt) * np.asarray(Bx)[eb]
    t, scale = np.zeros(m), np.zeros(m)
    np.add.at(t, rows, terms)
    np.add.at(scale, rows, np.abs(terms))
    return t, scale


# -- the normalised residuals

def _best(cands):
    """The largest of (value, row) pairs: a NaN above every number, then the larger value, then the lower row."""
    return min(cands, key=lambda c: (0 if np.isnan(c[0]) else 1, 0.0 if np.isnan(c[0]) else -c[0], c[1]))


def _group_sums(x, rows):
    """The partition of the reduction: groups of `rows` consecutive entries (zeros behind the last), each summed by the
    tree and the waves; then thread j takes the groups j, j + 256, ... in order, and again the tree and the waves."""
    ngroups = -(-len(x) // rows)
    padded = np.zeros(ngroups * rows)
    padded[:len(x)] = x
    parts = np.array([_waves(padded[g * rows:(g + 1) * rows]) for g in range(ngroups)])
    return _waves(_strided(parts, 256))


def restated_normres(t, w, r, crit_tol, limits):
    """(omega, rn, summary) of one matrix: summary = [worst, worst_row, J, critical]."""
    assert limits.reduce_rows == 256 and limits.block == 256
    t, w, r = (np.asarray(a, dtype=np.float64) for a in (t, w, r))
    with np.errstate(all="ignore"):
        omega = 1.0 / w - t
        critical = 1.0 - w * t <= crit_tol
        rn = np.where(critical, 0.0, np.abs(r) / np.sqrt(omega))
        J = _group_sums(w * (r * r), int(limits.reduce_rows))
    worst, row = _best(list(zip(rn.tolist(), range(len(rn)))))
    return omega, rn, np.array([worst, float(row), J, float(critical.sum())])
