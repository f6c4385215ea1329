"""The power-flow cases shared by test_pf_cpu.py and test_gpu_pf.py: planted solutions on synth.ybus networks, stars
whose hub row sits at the wave-row limit, chains with a chosen number of stored entries, and the small edge shapes.  A
case is a dict(n, Yp, Yi, Yz, pv, pq, vm, va (planted), S, vm0, va0 (the start)); reference results (the plan, the
Newton run of the NumPy restatement, the tolerance that separates its last two norms) are computed once per case and
shared."""
import functools

import numpy as np

import pf_ref as R
from csparse3_amd import synth

NOMINAL_TOL = 1e-8

# (nbus, nedges, seed, npv): the planted cases; the last is all PV, the one before all PQ
PLANTED = [(12, 16, 3, 3), (40, 60, 40, 8), (300, 480, 300, 60), (300, 480, 301, 0), (65, 90, 5, 64)]
PLANTED_ITERS = [4, 5, 5, 7, 4]                    # Newton steps of the restatement from the flat start (test_pf_cpu asserts them)


def network(n, edges, seed, ref=(0,), npv_every=5, shift_branch=None, drop=None, unsorted=False, descending=False,
            spread=0.15, flat=True, pv=None):
    """A network from an edge list: y = 1 / (r + jx) per branch as in synth.ybus, a shunt on every bus; voltages planted.
    ref: the reference buses; every npv_every-th of the other buses is PV (0: none; pv: an explicit list instead).
    shift_branch k: branch k carries a phase shift e^{+-0.05j} (unsymmetric values).  drop: (i, j), the stored entry that is
    removed (a one-sided pattern).  unsorted: the rows of every column in a shuffled order.  descending: the bus lists in
    descending order."""
    rng = np.random.default_rng(seed)
    ei, ej = np.asarray([e[0] for e in edges], dtype=np.int64), np.asarray([e[1] for e in edges], dtype=np.int64)
    y = 1.0 / (rng.uniform(0.001, 0.01, size=len(ei)) + 1j * rng.uniform(0.02, 0.1, size=len(ei)))
    diag = rng.uniform(0.0, 0.1, size=n) - 1j * rng.uniform(0.05, 0.5, size=n)
    np.add.at(diag, ei, y)
    np.add.at(diag, ej, y)
    lo, up = -y.copy(), -y.copy()
    if shift_branch is not None:
        lo[shift_branch] *= np.exp(0.05j)
        up[shift_branch] *= np.exp(-0.05j)
    rows = np.concatenate([ej, ei, np.arange(n)])
    cols = np.concatenate([ei, ej, np.arange(n)])
    vals = np.concatenate([lo, up, diag])
    if drop is not None:
        keep = ~((rows == drop[0]) & (cols == drop[1]))
        assert keep.sum() == len(rows) - 1
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    key = rng.permutation(len(rows)) if unsorted else rows
    order = np.lexsort((key, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    Yp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(Yp, cols + 1, 1)
    Yp = np.cumsum(Yp).astype(np.int32)
    Yi, Yz = rows.astype(np.int32), vals.astype(np.complex128)
    vm, va = rng.uniform(0.97, 1.03, size=n), rng.uniform(-spread, spread, size=n)
    va[ref[0]] = 0.0
    others = np.array([b for b in range(n) if b not in ref], dtype=np.int32)
    if pv is None:
        pv = others[npv_every - 1::npv_every] if npv_every else others[:0]
    pv = np.asarray(pv, dtype=np.int32)
    pq = np.array([b for b in others if b not in set(pv.tolist())], dtype=np.int32)
    if descending:
        pv, pq = pv[::-1].copy(), pq[::-1].copy()
    vm0, va0 = vm.copy(), va.copy()
    if flat:
        vm0[pq] = 1.0
        va0 = np.zeros(n)
        va0[list(ref)] = va[list(ref)]                  # (a reference bus keeps its angle)
    return dict(n=n, Yp=Yp, Yi=Yi, Yz=Yz, pv=pv, pq=pq, vm=vm, va=va, S=synth.pf_planted(n, Yp, Yi, Yz, vm, va), vm0=vm0, va0=va0)


@functools.lru_cache(maxsize=None)
def planted(k):
    nb, ne, seed, npv = PLANTED[k]
    return synth.pf_case(nb, ne, seed, npv)


@functools.lru_cache(maxsize=None)
def star(leaves):
    """Hub 0 (a PQ bus) with `leaves` leaves: the hub's row of Y holds leaves + 1 entries.  The last leaf is the
    reference, every fifth remaining bus is PV, branch 0 has a phase shift."""
    n = leaves + 1
    return network(n, [(0, k) for k in range(1, n)], 1000 + leaves, ref=(n - 1,), pv=np.arange(5, n - 1, 5), shift_branch=0, spread=0.05)


@functools.lru_cache(maxsize=None)
def one_sided():
    """40 buses, one lower-triangle entry removed, bus 20 a second reference."""
    rng = np.random.default_rng(41)
    ei, ej = synth._connected_graph(40, 60, rng)
    e = [(int(a), int(b)) for a, b in zip(ei, ej)]
    return network(40, e, 41, ref=(0, 20), drop=(max(e[7]), min(e[7])))


def chain(n, chords, **kw):
    """A path 0 - 1 - ... - n - 1 plus `chords` chords (k, k + 2): 3 n - 2 + 2 chords stored entries."""
    return network(n, [(k, k + 1) for k in range(n - 1)] + [(3 * k, 3 * k + 2) for k in range(chords)], 7 * n + chords, spread=0.1, **kw)


@functools.lru_cache(maxsize=None)
def shape(name):
    """The small edge shapes, by name."""
    if name == "nnz255":
        return chain(85, 1)
    if name == "nnz256":
        return chain(86, 0)
    if name == "nnz257":
        return chain(85, 2)
    if name == "n2":
        return network(2, [(0, 1)], 2, ref=(0,), npv_every=0)
    if name == "n3":
        return network(3, [(0, 1), (1, 2)], 3, ref=(1,), pv=[2])
    if name == "ref_middle":
        return chain(30, 3, ref=(14,))
    if name == "ref_last":
        return chain(30, 3, ref=(29,))
    if name == "two_refs":
        return chain(30, 3, ref=(4, 22))
    if name == "unsorted":
        return chain(30, 5, unsorted=True)
    if name == "descending":
        return chain(30, 3, descending=True)
    raise KeyError(name)


SHAPES = ["nnz255", "nnz256", "nnz257", "n2", "n3", "ref_middle", "ref_last", "two_refs", "unsorted", "descending"]


def star_sizes(limit):
    """Leaves for hub rows of limit - 1, limit, limit + 1, limit + 2, 2 limit + 2 and 2 limit + 3 entries."""
    return [limit - 2, limit - 1, limit, limit + 1, 2 * limit + 1, 2 * limit + 2]


def grid_edge(limits):
    """A diagonal Y plus one branch with one stored entry more than grid_cap * block: every bus but the reference (bus 0)
    and the two ends of the branch is isolated (a shunt alone), all PQ.  Started at the planted voltages."""
    n = int(limits.grid_cap * limits.block) - 1
    return network(n, [(n // 2, n // 2 + 1)], 9, ref=(0,), npv_every=0, flat=False)


_REF = {}


def reference(key, case):
    """The plan of the restatement, its Newton run from the case's start to the floor, the step count at the nominal
    tolerance and the tolerance that separates the two norms around it (their geometric mean).  Computed once per key."""
    if key not in _REF:
        P = R.plan_ref(case["n"], case["Yp"], case["Yi"], case["pv"], case["pq"])
        run = R.newton_ref(P, case["Yz"], case["S"], case["vm0"], case["va0"], NOMINAL_TOL, 15)
        k = run["iters"]
        tol = float(np.sqrt(run["norms"][k - 1] * run["norms"][k])) if k > 0 else NOMINAL_TOL
        _REF[key] = dict(P=P, run=run, iters=k, tol=tol)
    return _REF[key]


def newton_cases(limit):
    """(key, case) of every case the Newton tests run."""
    out = [("planted%d" % k, planted(k)) for k in range(len(PLANTED))]
    out += [("star%d" % s, star(s)) for s in star_sizes(limit)]
    out += [("one_sided", one_sided())]
    out += [(name, shape(name)) for name in SHAPES]
    return out


def smallest_pivot_ratio(J):
    """The smallest |diagonal| / max |column at and below| met by elimination without pivoting, in the natural order."""
    J, ratio = J.copy(), np.inf
    for k in range(len(J)):
        ratio = min(ratio, abs(J[k, k]) / np.abs(J[k:, k]).max())
        J[k + 1:, k] /= J[k, k]
        J[k + 1:, k + 1:] -= np.outer(J[k + 1:, k], J[k, k + 1:])
    return ratio


def newton_with_ratios(P, case, S=None, tol=NOMINAL_TOL, max_iters=15):
    """The restatement's Newton run, and the smallest pivot ratio of the Jacobian at EVERY iterate it factorises."""
    ratios = []

    def solver(P, Jx, rhs):
        J = R.dense_jacobian(P, Jx)
        ratios.append(smallest_pivot_ratio(J))
        return np.linalg.solve(J, rhs)

    run = R.newton_ref(P, case["Yz"], case["S"] if S is None else S, case["vm0"], case["va0"], tol, max_iters, solver=solver)
    return run, ratios


def scaled(case, scales):
    """A batch from one case: S[1:] scaled per member (bus 0 is the reference of the planted cases), the flat start.
    -> (S, vm0, va0), [len(scales), n] each."""
    S = np.stack([np.concatenate([case["S"][:1], case["S"][1:] * f]) for f in scales])
    k = len(scales)
    return S, np.tile(case["vm0"], (k, 1)), np.tile(case["va0"], (k, 1))


TRIO_SCALES = [1.0, 0.5, 0.1]


@functools.lru_cache(maxsize=None)
def trio():
    """Three scenarios of planted2 that need different numbers of steps, for the batch tests.  One tolerance has to serve
    all three: the geometric mean of the LARGEST last norm and the SMALLEST norm before the last over the members (the two
    norms the tolerance must separate for the batch); test_pf_cpu asserts that they are at least 1e3 apart.
    -> dict(case, P, S, vm0, va0, runs, tol)."""
    case = planted(2)
    P = reference("planted2", case)["P"]
    S, vm0, va0 = scaled(case, TRIO_SCALES)
    runs = [R.newton_ref(P, case["Yz"], S[b], vm0[b], va0[b], NOMINAL_TOL, 20) for b in range(3)]
    below, above = max(r["norms"][-1] for r in runs), min(r["norms"][-2] for r in runs)
    return dict(case=case, P=P, S=S, vm0=vm0, va0=va0, runs=runs, below=below, above=above, tol=float(np.sqrt(below * above)))


# The pivot threshold of the late-rejection test on planted3 (all PQ) in the NATURAL order: the Jacobian at the flat start
# passes it, the one at the first iterate does not (test_pf_cpu asserts a factor 1.8 of room on both sides).
LATE_PIVOT_TOL = 0.5
