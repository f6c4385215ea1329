"""Case builders of the union-plan tests, shared by tests/test_union_cpu.py and tests/test_gpu_union.py.  A pattern is
(Ap int32[n + 1], Ai int32[nnz]); a family is (n, [patterns]) or, with values, (n, [patterns], [values])."""
import numpy as np

from csparse3_amd import synth


def _csc(n, cols_rows):
    """[(col, [rows in storage order]), ...] -> (Ap, Ai); columns not named are empty."""
    per = {j: list(r) for j, r in cols_rows}
    Ap = np.zeros(n + 1, dtype=np.int32)
    Ai = []
    for j in range(n):
        Ai += per.get(j, [])
        Ap[j + 1] = len(Ai)
    return Ap, np.array(Ai, dtype=np.int32)


def random_pattern(rng, n, per_col, sort=False):
    """About per_col distinct rows in every column, in random storage order unless sort."""
    cols = []
    for j in range(n):
        k = int(rng.integers(0, min(n, 2 * per_col) + 1))
        r = rng.choice(n, size=k, replace=False)
        cols.append((j, np.sort(r) if sort else r))
    return _csc(n, cols)


def structural_cases():
    """name -> (n, patterns): the shapes the union has to get right (tests/test_union_cpu.py lists what each is for)."""
    rng = np.random.default_rng(11)
    c = {}
    c["single_unsorted"] = (4, [_csc(4, [(0, [3, 0, 2]), (1, [1]), (3, [2, 3, 0, 1])])])
    c["disjoint"] = (5, [_csc(5, [(0, [0, 2]), (2, [4]), (4, [1])]), _csc(5, [(0, [1, 3]), (1, [0]), (4, [4, 0])])])
    c["unsorted"] = (17, [random_pattern(rng, 17, 4) for _ in range(4)])
    c["empty_column_filled_by_others"] = (4, [_csc(4, [(0, [0]), (1, [1, 3]), (3, [3])]),
                                              _csc(4, [(0, [0]), (2, [2, 0]), (3, [3])]),
                                              _csc(4, [(2, [1]), (3, [0])])])
    c["empty_member"] = (4, [_csc(4, [(0, [0, 1]), (2, [2])]), _csc(4, []), _csc(4, [(1, [3]), (2, [2, 0])])])
    c["column_empty_everywhere"] = (5, [_csc(5, [(0, [0]), (1, [4, 1]), (4, [2])]), _csc(5, [(1, [2]), (3, [3]), (4, [2, 0])])])
    c["n1"] = (1, [_csc(1, [(0, [0])]), _csc(1, [])])
    c["n1_empty"] = (1, [_csc(1, [])])
    c["dup2"] = (3, [_csc(3, [(0, [2, 0, 2]), (1, [1])]), _csc(3, [(0, [0]), (2, [1])])])
    c["dup5"] = (3, [_csc(3, [(0, [1]), (1, [2, 0, 2, 2, 1, 2, 2]), (2, [0, 0])]), _csc(3, [(1, [2, 2])])])
    shared = [random_pattern(rng, 9, 3) for _ in range(4)]
    twin = (shared[0][0].copy(), shared[0][1].copy())             # equal element for element, other arrays
    c["six_members_three_identical"] = (9, [shared[0], shared[1], twin, shared[2], shared[0], shared[3]])
    c["many_over_three_patterns"] = (13, [random_patterns_3(13)[k % 3] for k in range(130)])
    return c


_P3 = {}


def random_patterns_3(n):
    if n not in _P3:
        rng = np.random.default_rng(300 + n)
        _P3[n] = [random_pattern(rng, n, 3) for _ in range(3)]
    return _P3[n]


def values_for(rng, patterns):
    return [rng.standard_normal(int(Ap[-1])) for Ap, Ai in patterns]


def diagonal_family(total, rng):
    """nmat * nnz_union == total exactly: member 0 is the full diagonal of order n = total / nmat (nmat the largest of
    4, 3, 2, 1 that divides total), the others lack a random third of it, each another third."""
    nmat = next(k for k in (4, 3, 2, 1) if total % k == 0)
    n = total // nmat
    full = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32))
    pats = [full]
    for _ in range(nmat - 1):
        keep = rng.random(n) >= 1.0 / 3.0
        Ap = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(keep, out=Ap[1:])
        pats.append((Ap, np.flatnonzero(keep).astype(np.int32)))
    return n, pats, values_for(rng, pats)


def banded_odd_family(rng):
    """Three members with an odd union (nnz_union = 3 * 33 - 2 = 97): the tridiagonal matrix of order 33, the same without
    its superdiagonal, the same without every other diagonal entry.  Member boundaries fall at odd flat indices."""
    n = 33
    tri = _csc(n, [(j, [i for i in (j - 1, j, j + 1) if 0 <= i < n]) for j in range(n)])
    low = _csc(n, [(j, [i for i in (j, j + 1) if i < n]) for j in range(n)])
    gap = _csc(n, [(j, [i for i in (j - 1, j, j + 1) if 0 <= i < n and not (i == j and j % 2)]) for j in range(n)])
    pats = [tri, low, gap]
    assert int(tri[0][-1]) == 97
    return n, pats, values_for(rng, pats)


def contingency_family(nbus=150, nedges=230, members=9, symmetric_values=False):
    """The end-to-end family: a connected network and `members` cases of it; case c lacks c mod 9 chord edges (c = 0 is the base
    case, so the union is the base pattern) and has values of its own, strictly diagonally dominant.
    -> (n, patterns, values), rows sorted."""
    ei, ej = synth._connected_graph(nbus, nedges, np.random.default_rng(7))
    chords = synth.chord_edges(nbus, ei, ej)
    pats, vals = [], []
    for c in range(members):
        drop = np.random.default_rng(50 + c).choice(chords, size=c % 9, replace=False)
        keep = np.ones(len(ei), dtype=bool)
        keep[drop] = False
        m, n, Ap, Ai, Ax = synth._graph_to_matrix(nbus, ei[keep], ej[keep], np.random.default_rng(100 + c),
                                                  symmetric_values=symmetric_values)
        pats.append((Ap, Ai))
        vals.append(Ax)
    return nbus, pats, vals
