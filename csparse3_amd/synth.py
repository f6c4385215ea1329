"""Seeded synthetic inputs for the five BASELINE.json configurations.

No power-grid data ships with the reference beyond a 5-bus line list
(/root/reference/src/test/test3_lil_matrix.py:18-24), so every input is
synthesised from numpy.random.default_rng(seed) as SURVEY.md section 8d lays out.
All matrices come back in the reference's flat CSC convention:
(m, n, indptr int32, indices int32, data float64), rows sorted, no duplicates.
"""
import numpy as np


def _coo_to_sorted_csc(n, rows, cols, vals):
    """Assemble unique (row, col, val) triplets into row-sorted CSC."""
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, cols + 1, 1)
    indptr = np.cumsum(indptr)
    return (n, n, indptr.astype(np.int32), rows.astype(np.int32),
            vals.astype(np.float64))


def _graph_to_matrix(n, ei, ej, rng, asym=0.05, shift=1.0, symmetric_values=False):
    """Edges (ei < ej, unique) -> diagonally dominant matrix with that pattern.

    off-diagonal ~ -U(0.1, 1); the two triangles differ by a +-asym relative
    perturbation unless symmetric_values; diag = sum |row| + shift.
    """
    w = rng.uniform(0.1, 1.0, size=len(ei))
    if symmetric_values:
        lo = up = -w
    else:
        lo = -w * (1.0 + asym * rng.uniform(-1.0, 1.0, size=len(ei)))
        up = -w * (1.0 + asym * rng.uniform(-1.0, 1.0, size=len(ei)))
    rowsum = np.zeros(n)
    np.add.at(rowsum, ej, np.abs(lo))    # entry (ej, ei) lies in row ej
    np.add.at(rowsum, ei, np.abs(up))    # entry (ei, ej) lies in row ei
    if symmetric_values:
        diag = rowsum + shift
    else:
        diag = rowsum + shift
    rows = np.concatenate([ej, ei, np.arange(n)])
    cols = np.concatenate([ei, ej, np.arange(n)])
    vals = np.concatenate([lo, up, diag])
    return _coo_to_sorted_csc(n, rows, cols, vals)


def _unique_edges(n, ei, ej):
    lo = np.minimum(ei, ej)
    hi = np.maximum(ei, ej)
    keep = lo != hi
    key = np.unique(lo[keep].astype(np.int64) * n + hi[keep])
    return (key // n).astype(np.int64), (key % n).astype(np.int64)


def toy10(seed=1):
    """Config 1: 10x10, tridiagonal + 3 symmetric off-band pairs, strictly
    diagonally dominant.  -> (m, n, Ap, Ai, Ax, b, x_true), b = A (1..10)."""
    rng = np.random.default_rng(seed)
    n = 10
    ei = np.concatenate([np.arange(n - 1), np.array([0, 2, 4])])
    ej = np.concatenate([np.arange(1, n), np.array([5, 8, 9])])
    ei, ej = _unique_edges(n, ei, ej)
    m, n, Ap, Ai, Ax = _graph_to_matrix(n, ei, ej, rng)
    x_true = np.arange(1.0, n + 1.0)
    b = np.zeros(n)
    for j in range(n):
        for p in range(Ap[j], Ap[j + 1]):
            b[Ai[p]] += Ax[p] * x_true[j]
    return m, n, Ap, Ai, Ax, b, x_true


def _connected_graph(nbus, nedges, rng):
    """Random spanning tree (each node attaches to an earlier one, preferring
    recent nodes, which gives the long radial feeders of a grid) + chords."""
    parent = np.zeros(nbus, dtype=np.int64)
    for v in range(1, nbus):
        lo = max(0, v - 8)
        parent[v] = rng.integers(lo, v) if rng.random() < 0.8 else rng.integers(0, v)
    ei = parent[1:]
    ej = np.arange(1, nbus)
    ei, ej = _unique_edges(nbus, ei, ej)
    while len(ei) < nedges:
        need = nedges - len(ei)
        a = rng.integers(0, nbus, size=2 * need)
        b = rng.integers(0, nbus, size=2 * need)
        ei, ej = _unique_edges(nbus, np.concatenate([ei, a]), np.concatenate([ej, b]))
        if len(ei) > nedges:
            # drop surplus chords, never tree edges (tree edges have ej-parent relation)
            is_tree = parent[ej] == ei
            chord_idx = np.flatnonzero(~is_tree)
            drop = rng.choice(chord_idx, size=len(ei) - nedges, replace=False)
            keep = np.ones(len(ei), dtype=bool)
            keep[drop] = False
            ei, ej = ei[keep], ej[keep]
    return ei, ej


def jacobian_like(nbus=118, nedges=186, n_pv=34, seed=118):
    """Config 2: "118-bus-like" power-flow Jacobian.

    Y-bus of a random connected graph (branch r, x ~ U(0.01, 0.1)); the
    Jacobian J = [[H, N], [M, L]] is laid out exactly as the reference's
    pack_4_by_4 stacks it (/root/reference/src/CSparse3/csc.py:588-606):
    H is (pvpq x pvpq), N (pvpq x pq), M (pq x pvpq), L (pq x pq), bus 0 the
    slack.  Structurally symmetric, values unsymmetric; flat-start
    sensitivities with a small diagonal shift so it is diagonally dominant
    enough for diagonal pivots.  True IEEE-118 data is not available offline.
    -> (m, n, Ap, Ai, Ax)
    """
    rng = np.random.default_rng(seed)
    ei, ej = _connected_graph(nbus, nedges, rng)
    r = rng.uniform(0.01, 0.1, size=len(ei))
    x = rng.uniform(0.01, 0.1, size=len(ei))
    y = 1.0 / (r + 1j * x)
    g, bsus = y.real, y.imag                       # series admittance g + jb, b < 0
    G = np.zeros((nbus, nbus))
    B = np.zeros((nbus, nbus))
    for k in range(len(ei)):
        i, j = ei[k], ej[k]
        G[i, j] -= g[k]; G[j, i] -= g[k]; G[i, i] += g[k]; G[j, j] += g[k]
        B[i, j] -= bsus[k]; B[j, i] -= bsus[k]; B[i, i] += bsus[k]; B[j, j] += bsus[k]
    th = rng.uniform(-0.05, 0.05, size=nbus)       # small angle spread
    v = rng.uniform(0.98, 1.04, size=nbus)
    pv = np.sort(rng.choice(np.arange(1, nbus), size=n_pv, replace=False))
    pq = np.setdiff1d(np.arange(1, nbus), pv)
    pvpq = np.concatenate([pv, pq])
    dth = th[:, None] - th[None, :]
    vv = v[:, None] * v[None, :]
    mask = (G != 0) | (B != 0)
    Hf = vv * (G * np.sin(dth) - B * np.cos(dth)) * mask
    Nf = vv * (G * np.cos(dth) + B * np.sin(dth)) * mask / v[None, :]
    Mf = -vv * (G * np.cos(dth) + B * np.sin(dth)) * mask
    Lf = vv * (G * np.sin(dth) - B * np.cos(dth)) * mask / v[None, :]
    P = (vv * (G * np.cos(dth) + B * np.sin(dth))).sum(axis=1)
    Q = (vv * (G * np.sin(dth) - B * np.cos(dth))).sum(axis=1)
    idx = np.arange(nbus)
    Hf[idx, idx] = -Q - B[idx, idx] * v * v
    Nf[idx, idx] = P / v + G[idx, idx] * v
    Mf[idx, idx] = P - G[idx, idx] * v * v
    Lf[idx, idx] = Q / v - B[idx, idx] * v
    H = Hf[np.ix_(pvpq, pvpq)]
    N = Nf[np.ix_(pvpq, pq)]
    M = Mf[np.ix_(pq, pvpq)]
    L = Lf[np.ix_(pq, pq)]
    J = np.block([[H, N], [M, L]])
    pat = np.block([[mask[np.ix_(pvpq, pvpq)], mask[np.ix_(pvpq, pq)]],
                    [mask[np.ix_(pq, pvpq)], mask[np.ix_(pq, pq)]]])
    n = J.shape[0]
    rows, cols = np.nonzero(pat.T)                 # iterate column-major
    cols, rows = rows, cols
    vals = J[rows, cols]
    return _coo_to_sorted_csc(n, rows.astype(np.int64), cols.astype(np.int64), vals)


def jacobian_config2(seed=118):
    """BASELINE.json configs[1] at the size it states (~400 x 400, ~3k nnz): the same Jacobian builder on a
    220-bus / 340-branch network with 38 PV buses (2 * 219 - 38 = 400 unknowns, 2 986 entries).  The true
    IEEE-118 case is not available offline and would give a 181 x 181 Jacobian (117 + 64 unknowns), so the
    config's own size figures are used; `jacobian_like()` stays as the 118-bus-sized case.
    -> (m, n, Ap, Ai, Ax)"""
    return jacobian_like(nbus=220, nedges=340, n_pv=38, seed=seed)


def ybus_branches(nbus, nedges, seed):
    """The branches (ei, ej) with their series admittances y and the bus shunts behind ybus(nbus, nedges, seed)."""
    rng = np.random.default_rng(seed)
    ei, ej = _connected_graph(nbus, nedges, rng)
    r = rng.uniform(0.001, 0.01, size=len(ei))
    x = rng.uniform(0.02, 0.1, size=len(ei))
    y = 1.0 / (r + 1j * x)
    shunt = rng.uniform(0.0, 0.1, size=nbus) - 1j * rng.uniform(0.05, 0.5, size=nbus)
    return ei, ej, y, shunt


def ybus(nbus, nedges, seed, lossless=False):
    """Complex bus admittance matrix of a random connected network (the graph of jacobian_like): branches with
    r ~ U(0.001, 0.01), x ~ U(0.02, 0.1), y = 1 / (r + jx), and on every bus a shunt g - jb with g ~ U(0, 0.1),
    b ~ U(0.05, 0.5) on the diagonal (inductive, so the matrix is far from singular: condition number near 1e3).  The
    chords beyond the spanning tree are random, so fill grows quickly with nedges - nbus.  Symmetric, not Hermitian; the diagonal is mostly
    imaginary.  lossless: every real part is +0 -- the diagonal is purely imaginary, as for a network without
    resistance.  -> (n, Ap, Ai, Az) with Az complex128, rows sorted, no duplicates."""
    ei, ej, y, shunt = ybus_branches(nbus, nedges, seed)
    diag = shunt.copy()
    np.add.at(diag, ei, y)
    np.add.at(diag, ej, y)
    rows = np.concatenate([ej, ei, np.arange(nbus)])
    cols = np.concatenate([ei, ej, np.arange(nbus)])
    vals = np.concatenate([-y, -y, diag])
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    if lossless:
        vals = vals.copy()
        vals.real = 0.0                              # (+0, never -0)
    Ap = np.zeros(nbus + 1, dtype=np.int64)
    np.add.at(Ap, cols + 1, 1)
    return nbus, np.cumsum(Ap).astype(np.int32), rows.astype(np.int32), vals.astype(np.complex128)


def grid_graph_edges(n, offsets, chord_frac, rng):
    """1-D chain with extra local ties i <-> i+k for k in offsets, plus
    chord_frac * n random long chords."""
    ei, ej = [], []
    for k in offsets:
        ei.append(np.arange(0, n - k))
        ej.append(np.arange(k, n))
    nch = int(round(chord_frac * n))
    if nch > 0:
        ei.append(rng.integers(0, n, size=nch))
        ej.append(rng.integers(0, n, size=nch))
    return _unique_edges(n, np.concatenate(ei), np.concatenate(ej))


def grid_jacobian(n=50000, seed=50000, offsets=(1, 2, 3, 4), thin=(0.5,),
                  thin_offsets=(9,), chord_frac=0.01):
    """Config 3 / 4: synthetic banded power-grid Jacobian, ~10 nnz per row.

    Radial-plus-meshed graph: chain ties at +-offsets on every node, ties at
    +-thin_offsets on a random fraction `thin` of the nodes, and chord_frac * n
    random long chords; off-diagonal ~ -U(0.1, 1) with a +-5 % asymmetric
    perturbation, diag = sum |row| + 1.  -> (m, n, Ap, Ai, Ax)
    """
    rng = np.random.default_rng(seed)
    ei, ej = grid_graph_edges(n, offsets, chord_frac, rng)
    extra_i, extra_j = [ei], [ej]
    for frac, k in zip(thin, thin_offsets):
        start = np.flatnonzero(rng.random(n - k) < frac)
        extra_i.append(start)
        extra_j.append(start + k)
    ei, ej = _unique_edges(n, np.concatenate(extra_i), np.concatenate(extra_j))
    return _graph_to_matrix(n, ei, ej, rng)


def grid_rhs(n, k=1, seed=1024):
    """Right-hand sides: (n,) for k == 1 else row-major (n, k), the
    reference's multi-vector layout (/root/reference/src/CSparse3/csc.py:409-414)."""
    rng = np.random.default_rng(seed)
    if k == 1:
        return rng.standard_normal(n)
    return rng.standard_normal((n, k))


def spd_grid_pattern(n=5000, seed=5000, width=None, chord_frac=0.01):
    """Config 5 pattern: 2-D-ish grid (row length `width`) + chords.
    -> (ei, ej) with ei < ej."""
    rng = np.random.default_rng(seed)
    if width is None:
        width = int(round(np.sqrt(n)))
    idx = np.arange(n)
    right = idx[(idx % width) != width - 1]
    right = right[right + 1 < n]
    down = idx[idx + width < n]
    nch = int(round(chord_frac * n))
    ei = np.concatenate([right, down, rng.integers(0, n, size=nch)])
    ej = np.concatenate([right + 1, down + width, rng.integers(0, n, size=nch)])
    return _unique_edges(n, ei, ej)


def chord_edges(n, ei, ej):
    """Indices of the edges outside a spanning forest of the graph (walking the edges in order, the first one that joins
    two components is a tree edge): removing any set of them disconnects nothing -- the branches a contingency case
    may lack."""
    root = np.arange(n)

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    chords = []
    for k in range(len(ei)):
        a, b = find(int(ei[k])), find(int(ej[k]))
        if a == b:
            chords.append(k)
        else:
            root[a] = b
    return np.array(chords, dtype=np.int64)


def spd_grid_matrix(n, ei, ej, seed, shift=1e-2, lower_only=False):
    """Config 5 values: weighted graph Laplacian + shift * I on a given pattern
    (same pattern, different values per matrix: contingency-style).
    -> (m, n, Ap, Ai, Ax); full symmetric storage unless lower_only."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 1.0, size=len(ei))
    diag = np.full(n, shift)
    np.add.at(diag, ei, w)
    np.add.at(diag, ej, w)
    if lower_only:
        rows = np.concatenate([ej, np.arange(n)])
        cols = np.concatenate([ei, np.arange(n)])
        vals = np.concatenate([-w, diag])
    else:
        rows = np.concatenate([ej, ei, np.arange(n)])
        cols = np.concatenate([ei, ej, np.arange(n)])
        vals = np.concatenate([-w, -w, diag])
    return _coo_to_sorted_csc(n, rows, cols, vals)


def dense_block_matrix(n=700, nd=300, seed=1):
    """Sparse matrix with an embedded nd x nd dense block: its factorisation ends in
    fronts too large for the LDS, which exercises the blocked big-front kernels.
    Structurally symmetric, diagonally dominant.  -> (m, n, Ap, Ai, Ax)"""
    rng = np.random.default_rng(seed)
    nz = 3 * n
    ei = rng.integers(0, n, size=nz)
    ej = rng.integers(0, n, size=nz)
    idx = rng.choice(n, size=nd, replace=False)
    bi, bj = np.meshgrid(idx, idx, indexing="ij")
    ei, ej = _unique_edges(n, np.concatenate([ei, bi.ravel()]), np.concatenate([ej, bj.ravel()]))
    return _graph_to_matrix(n, ei, ej, rng)


def se_case(nbus, nedges, seed, inj_share=0.5, ncrit=2):
    """Measurement Jacobian of a DC-type state estimate (states: the nbus bus angles) on _connected_graph.

    The last `ncrit` buses are pendant: each hangs on one branch off a bus of the meshed part (nbus - ncrit buses,
    nedges - ncrit branches).  Rows, in this order: one flow row per branch, (b, -b) at its two buses, b = 1/x,
    x ~ U(0.5, 2) (scaled so that cond_1 of H' W H stays below 1e4 at a few hundred buses); then one row per bus of the meshed part -- an injection row (the sum of its branches' b at the bus,
    -b at each neighbour: degree + 1 entries) on a share `inj_share` of them, a magnitude row (a single 1) on the rest.
    The buses that carry a pendant branch have magnitude rows and a pendant bus has no row of its own, so the flow row of
    a pendant branch is the only row that sees its pendant bus: a designed critical measurement.  Weights w = 10^U(0, 2).
    -> (m, n, Hp, Hi, Hx, w, critical_rows): H is m x n in CSC, rows sorted, no duplicates."""
    rng = np.random.default_rng(seed)
    nb = nbus - ncrit
    assert ncrit >= 1 and nb >= 2 and nedges - ncrit >= nb - 1
    ei, ej = _connected_graph(nb, nedges - ncrit, rng)
    is_inj = rng.random(nb) < inj_share
    hosts = rng.choice(np.flatnonzero(~is_inj) if (~is_inj).sum() >= ncrit else np.arange(nb), size=ncrit, replace=False)
    is_inj[hosts] = False
    ei = np.concatenate([ei, hosts]).astype(np.int64)
    ej = np.concatenate([ej, nb + np.arange(ncrit)]).astype(np.int64)
    nbr = len(ei)
    b = 1.0 / rng.uniform(0.5, 2.0, size=nbr)
    flow = np.arange(nbr)
    rows = [flow, flow]
    cols = [ei, ej]
    vals = [b, -b]
    bus_row = nbr + np.arange(nb)
    diag = np.zeros(nbus)
    np.add.at(diag, ei, b)
    np.add.at(diag, ej, b)
    inj = np.flatnonzero(is_inj)
    rows.append(bus_row[inj]); cols.append(inj); vals.append(diag[inj])
    for me, other in ((ei, ej), (ej, ei)):
        k = np.flatnonzero((me < nb) & is_inj[np.minimum(me, nb - 1)])
        rows.append(bus_row[me[k]]); cols.append(other[k]); vals.append(-b[k])
    mag = np.flatnonzero(~is_inj)
    rows.append(bus_row[mag]); cols.append(mag); vals.append(np.ones(len(mag)))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    m = nbr + nb
    order = np.lexsort((rows, cols))
    Hp = np.zeros(nbus + 1, dtype=np.int64)
    np.add.at(Hp, cols + 1, 1)
    w = 10.0 ** rng.uniform(0.0, 2.0, size=m)
    return (m, nbus, np.cumsum(Hp).astype(np.int32), rows[order].astype(np.int32), vals[order].astype(np.float64), w,
            np.arange(nbr - ncrit, nbr))


def pf_planted(n, Ap, Ai, Az, vm, va):
    """S = V conj(Y V) for V = vm exp(j va): the injections that make (vm, va) a solution of the power flow."""
    V = vm * np.exp(1j * va)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    I = np.zeros(n, dtype=np.complex128)
    np.add.at(I, Ai, Az * V[cols])
    return V * np.conj(I)


def pf_case(nbus, nedges, seed, npv, spread=0.15):
    """A power-flow case with a planted solution on ybus(nbus, nedges, seed): voltages vm ~ U(0.97, 1.03) and
    va ~ U(-spread, spread) with va[0] = 0 from default_rng(seed + 7); injections S = V conj(Y V); pv = sorted
    choice(1 .. n - 1, npv), pq = the remaining buses, bus 0 the reference.  The flat start is vm = 1 at pq buses, the
    planted magnitude at pv and reference buses, va = 0.
    -> dict(n, Yp, Yi, Yz, pv, pq, vm, va, S, vm0, va0)."""
    n, Ap, Ai, Az = ybus(nbus, nedges, seed)
    rng = np.random.default_rng(seed + 7)
    vm = rng.uniform(0.97, 1.03, size=n)
    va = rng.uniform(-spread, spread, size=n)
    va[0] = 0.0
    pv = np.sort(rng.choice(np.arange(1, n), size=npv, replace=False)).astype(np.int32)
    is_pq = np.ones(n, dtype=bool)
    is_pq[0] = False
    is_pq[pv] = False
    pq = np.flatnonzero(is_pq).astype(np.int32)
    vm0 = vm.copy()
    vm0[pq] = 1.0
    return dict(n=n, Yp=Ap, Yi=Ai, Yz=Az, pv=pv, pq=pq, vm=vm, va=va, S=pf_planted(n, Ap, Ai, Az, vm, va), vm0=vm0,
                va0=np.zeros(n))


def se_flows(end_from, end_to, Ye, vm, va):
    """Sf_k = V_f conj(yff V_f + yft V_t) at every branch end, Ye complex [ne, 2] = (yff, yft)."""
    V = vm * np.exp(1j * va)
    Ye = np.asarray(Ye, dtype=np.complex128).reshape(-1, 2)
    return V[end_from] * np.conj(Ye[:, 0] * V[end_from] + Ye[:, 1] * V[end_to])


def se_measurements(n, Ap, Ai, Az, end_from, end_to, Ye, kind, where, vm, va):
    """h(x) of the measurement rows (kind, where) of an AC state estimate: 0 |V|, 1 / 2 Re / Im of the injection
    V conj(Y V) at a bus, 3 / 4 Re / Im of the flow at a branch end."""
    S = pf_planted(n, Ap, Ai, Az, vm, va)
    Sf = se_flows(end_from, end_to, Ye, vm, va) if len(end_from) else np.zeros(0, dtype=np.complex128)
    kind, where = np.asarray(kind), np.asarray(where)
    h = np.empty(len(kind))
    for k, src in ((0, vm), (1, S.real), (2, S.imag), (3, Sf.real), (4, Sf.imag)):
        h[kind == k] = src[where[kind == k]]
    return h


def se_ac_case(nbus, nedges, seed, noise=0.0, inj_share=0.5, spread=0.15):
    """An AC state-estimation case with a planted state on ybus(nbus, nedges, seed) and its branch list
    (ybus_branches).  Branch ends: both ends of every branch, the from-ends first,
    yff = y, yft = -y (the shunts sit on the diagonal of Y only).  State as in pf_case: vm ~ U(0.97, 1.03),
    va ~ U(-spread, spread) with va[0] = 0 from default_rng(seed + 7); bus 0 is the reference.  Rows, in this order: the P and
    Q flow at the from-end of every branch (P, Q interleaved); then per bus in ascending order P and Q of its injection on
    a share `inj_share` of the buses, a magnitude row on the rest and on bus 0.  w = 10^U(2, 4), z = h(x*) + noise N(0, 1) /
    sqrt(w).  The flat start is vm = 1, va = 0.
    -> dict(n, Yp, Yi, Yz, ref, end_from, end_to, Ye, kind, where, z, w, vm, va, vm0, va0)."""
    n, Ap, Ai, Az = ybus(nbus, nedges, seed)
    ei, ej, y, _ = ybus_branches(nbus, nedges, seed)
    nbr = len(ei)
    end_from = np.concatenate([ei, ej]).astype(np.int32)
    end_to = np.concatenate([ej, ei]).astype(np.int32)
    Ye = np.stack([np.concatenate([y, y]), -np.concatenate([y, y])], axis=1).astype(np.complex128)
    rng = np.random.default_rng(seed + 7)
    vm = rng.uniform(0.97, 1.03, size=n)
    va = rng.uniform(-spread, spread, size=n)
    va[0] = 0.0
    is_inj = rng.random(n) < inj_share
    kind, where = [], []
    for k in range(nbr):
        kind += [3, 4]; where += [k, k]
    for b in range(n):
        if is_inj[b]:
            kind += [1, 2]; where += [b, b]
        if not is_inj[b] or b == 0:
            kind.append(0); where.append(b)
    kind, where = np.asarray(kind, dtype=np.int32), np.asarray(where, dtype=np.int32)
    m = len(kind)
    w = 10.0 ** rng.uniform(2.0, 4.0, size=m)
    z = se_measurements(n, Ap, Ai, Az, end_from, end_to, Ye, kind, where, vm, va) + noise * rng.standard_normal(m) / np.sqrt(w)
    return dict(n=n, Yp=Ap, Yi=Ai, Yz=Az, ref=np.zeros(1, dtype=np.int32), end_from=end_from, end_to=end_to, Ye=Ye, kind=kind,
                where=where, z=z, w=w, vm=vm, va=va, vm0=np.ones(n), va0=np.zeros(n))
