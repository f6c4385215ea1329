"""The cases of the state-estimation tests (test_se_cpu.py asserts their properties, test_gpu_se.py runs them on the device).
Every case is a dict(n, Yp, Yi, Yz, ref, end_from, end_to, Ye, kind, where, z, w, vm, va (the planted state), vm0, va0 (the
flat start)); the sizes that bracket a path of the kernels come from cs3_se_limits.

Networks made here (stars, chains) use branches y = 1 / (r + jx) with x ~ U(0.8, 1.25), shunts of the size of a branch,
weights w = 10^U(2, 2.5) and a magnitude row on (nearly) every bus; the solved chains are short and reach their row and
entry counts by repeated rows.  That keeps cond_1 of the gain matrix below quad_ref.COND_MAX, which an estimate on a long
radial network cannot do (the angle block is a weighted path Laplacian: its condition grows with the square of the
length); test_se_cpu.py asserts it for every solved case.  The generator synth.se_ac_case (admittances of 10 to 50 per
unit against magnitude rows of 1, weights over two decades) stays below COND_MAX only on networks of about a dozen buses:
the solved cases ac* are that small and their seeds are chosen for it, while one case of 120 buses goes through the
kernel tests only."""
import functools

import numpy as np

import se_ref as R
from csparse3_amd import csc_hip, synth

TOL = 1e-8
MAX_ITERS = 20
CRIT_TOL = 1e-8


@functools.lru_cache(maxsize=None)
def limits():
    L = csc_hip.se_limits()
    return dict(block=int(L.block), grid_cap=int(L.grid_cap), wave_row=int(L.wave_row), wave_col=int(L.wave_col))


def network(n, ei, ej, seed, one_sided=False, unsorted=False):
    """Y of n buses with the branches (ei[k], ej[k]); both ends of every branch, the from-ends first; yff = y, yft = -y."""
    rng = np.random.default_rng(seed)
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    y = 1.0 / (rng.uniform(0.02, 0.1, size=len(ei)) + 1j * rng.uniform(0.8, 1.25, size=len(ei)))
    diag = rng.uniform(0.0, 0.2, size=n) - 1j * rng.uniform(0.5, 1.5, size=n)
    np.add.at(diag, ei, y)
    np.add.at(diag, ej, y)
    rows = np.concatenate([ej, ei, np.arange(n)])
    cols = np.concatenate([ei, ej, np.arange(n)])
    vals = np.concatenate([-y, -y, diag])
    if one_sided:                                   # Y_ij stored, Y_ji not, for the first branch: the values are simply absent
        keep = np.ones(len(rows), dtype=bool)
        keep[len(ei)] = False
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((rows, cols))
    if unsorted:                                    # every column's rows in descending order
        order = np.lexsort((-rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    Yp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    return dict(n=n, Yp=Yp, Yi=rows.astype(np.int32), Yz=vals.astype(np.complex128), end_from=np.concatenate([ei, ej]).astype(np.int32),
                end_to=np.concatenate([ej, ei]).astype(np.int32), Ye=np.stack([np.concatenate([y, y]), -np.concatenate([y, y])], axis=1),
                nbr=len(ei))


def finish(net, ref, kind, where, seed, noise=0.0, spread=0.1):
    """The planted state, the weights and the measured values of a network and its measurement rows."""
    n = net["n"]
    rng = np.random.default_rng(seed + 7)
    vm = rng.uniform(0.97, 1.03, size=n)
    va = rng.uniform(-spread, spread, size=n)
    ref = np.asarray(ref, dtype=np.int32).reshape(-1)
    va[ref] = 0.0
    kind, where = np.asarray(kind, dtype=np.int32), np.asarray(where, dtype=np.int32)
    w = 10.0 ** rng.uniform(2.0, 2.5, size=len(kind))
    h = synth.se_measurements(n, net["Yp"], net["Yi"], net["Yz"], net["end_from"], net["end_to"], net["Ye"], kind, where, vm, va)
    case = {k: net[k] for k in ("n", "Yp", "Yi", "Yz", "end_from", "end_to", "Ye")}
    case.update(ref=ref, kind=kind, where=where, w=w, z=h + noise * rng.standard_normal(len(kind)) / np.sqrt(w), vm=vm, va=va,
                vm0=np.ones(n), va0=np.zeros(n))
    return case


def rows_of(flows=(), inj=(), mag=()):
    """P and Q of the flows at the given branch ends, P and Q of the injections at the given buses, |V| at the given buses."""
    kind, where = [], []
    for k in flows:
        kind += [3, 4]; where += [k, k]
    for b in inj:
        kind += [1, 2]; where += [b, b]
    for b in mag:
        kind.append(0); where.append(b)
    return kind, where


def star(nleaves, seed, hub_mag=1, ref=1):
    """A hub (bus 0) with nleaves leaves: the hub's row of Y holds nleaves + 1 entries.  P and Q injections on the hub and on
    every leaf, a magnitude row on every leaf and hub_mag of them on the hub.  The hub's magnitude column of H then holds
    2 (nleaves + 1) + hub_mag entries, its angle column (where the hub is not the reference) 2 (nleaves + 1); a leaf's
    columns hold 5 and 4.  The hub's two injection rows sum over every leaf: their weights are divided by n^2, as a meter
    on a large bus is read in larger units.  With a leaf as the reference every other angle is seen through the hub, and
    cond_1 of the gain matrix grows with the number of leaves (3e4 at 64); with the hub as the reference it stays near 1e3."""
    n = nleaves + 1
    net = network(n, np.zeros(nleaves, dtype=np.int64), np.arange(1, n), seed)
    kind, where = rows_of(inj=range(n), mag=list(range(1, n)) + [0] * hub_mag)
    case = finish(net, [ref], kind, where, seed)
    case["w"][:2] /= float(n * n)
    case["hub_row"], case["hub_mag_col"], case["hub_angle_col"] = n, 2 * n + hub_mag, 2 * n if ref != 0 else None
    return case


def chain(n, seed, rows=None, entries=None, ref=(0,), flows=True, inj=(), mag=None, **kw):
    """A path of n buses, bus k - 1 to bus k: flows at the from-end of every branch, injections at the buses `inj`, a
    magnitude row on every bus (or on `mag`).  rows / entries: repeat these rows in order, again and again, up to exactly
    that many measurements / entries of H (a row that no longer fits gives way to magnitude rows, one entry each)."""
    net = network(n, np.arange(n - 1), np.arange(1, n), seed, **{k: kw.pop(k) for k in ("one_sided", "unsorted") if k in kw})
    kind, where = rows_of(flows=range(n - 1) if flows else (), inj=inj, mag=(range(n) if mag is None else mag))
    is_ref = np.zeros(n, dtype=bool)
    is_ref[list(ref)] = True
    size = lambda k, at: 1 if k == 0 else 4 - int(is_ref[net["end_from"][at]]) - int(is_ref[net["end_to"][at]])
    assert not inj or (rows is None and entries is None)
    base = list(zip(kind, where))
    have, k = sum(size(*r) for r in base), 0
    while (rows is not None and len(kind) < rows) or (entries is not None and have < entries):
        row = base[k % len(base)]
        k += 1
        if entries is not None and have + size(*row) > entries:
            row = (0, k % n)
        kind.append(row[0]); where.append(row[1])
        have += size(*row)
    return finish(net, list(ref), kind, where, seed, **kw)


CHAIN_BUSES = 12


def chain_rows(m, seed):
    """A chain of 12 buses with exactly m measurements."""
    return chain(CHAIN_BUSES, seed, rows=m)


def chain_entries(nnz, seed, n=CHAIN_BUSES):
    """A chain with exactly nnz entries of H: a flow row has 4 (3 on the branch at the reference), a magnitude row 1."""
    return chain(n, seed, entries=nnz)


def unobservable(seed=5):
    """A chain of 12 buses whose last bus no row touches: no flow on its branch, no injection at it or at its neighbour, no
    magnitude: both of its columns of H are empty."""
    n = 12
    net = network(n, np.arange(n - 1), np.arange(1, n), seed)
    kind, where = rows_of(flows=range(n - 2), mag=range(n - 1))
    return finish(net, [0], kind, where, seed)


def both_ends(seed=6):
    """A chain whose first three branches are measured at both ends."""
    n = 10
    net = network(n, np.arange(n - 1), np.arange(1, n), seed)
    kind, where = rows_of(flows=list(range(n - 1)) + [net["nbr"] + k for k in range(3)], mag=range(n))
    return finish(net, [0], kind, where, seed)


def repeated(seed=169):
    """Every row of a small meshed case twice."""
    case = dict(synth.se_ac_case(14, 16, seed))
    for key in ("kind", "where", "z", "w"):
        case[key] = np.repeat(case[key], 2)
    return case


def no_ends(seed=10):
    """ne = 0: injections and magnitudes only."""
    n = 6
    net = network(n, np.arange(n - 1), np.arange(1, n), seed)
    for key in ("end_from", "end_to"):
        net[key] = np.zeros(0, dtype=np.int32)
    net["Ye"] = np.zeros((0, 2), dtype=np.complex128)
    kind, where = rows_of(inj=range(n), mag=range(n))
    return finish(net, [0], kind, where, seed)


AC_SIZE = (14, 16)            # the largest size at which seeds with cond_1 <= COND_MAX are not rare (about 1 in 300)
AC_SEEDS = (169, 416, 442)
# noise 1 with both deciding steps a factor 100 away from TOL needs a linear rate below 1e-4 at a step of 1e-6: that is
# rare (test_se_cpu.py asserts it for this seed), and rarer the larger the network
NOISY_SIZE, NOISY_SEED, NOISY_INJ_SHARE = (4, 5), 16629, 0.7
AC_LARGE = (120, 138, 11)     # nbus, nedges, seed: kernel tests only

SOLVED = ["ac169", "ac416", "ac442", "noisy", "star_col63", "star_col64", "star_col65", "chain_m255", "chain_m256", "chain_m257",
          "chain_nnz255", "chain_nnz256", "chain_nnz257", "two_buses", "ref_first", "ref_middle", "ref_last", "two_refs",
          "flows_and_magnitudes", "injections_one_magnitude", "repeated", "unsorted", "one_sided", "both_ends", "no_ends"]
STARS = ["star_row63", "star_row64", "star_row65", "star_row129"]        # the hub's row of Y around wave_row; the hub is the reference
SOLVED += STARS
KERNEL_ONLY = ["ac_large", "grid_edge"]
EVERY = SOLVED + KERNEL_ONLY + ["unobservable"]
NOISE_FREE = [k for k in SOLVED if k != "noisy"]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, all but grid_edge (built on demand: it is large)."""
    L = limits()
    W, C = L["wave_row"], L["wave_col"]
    assert (W, C) == (64, 64), "the names above spell sizes around wave_row = wave_col = 64"
    out = {}
    for s in AC_SEEDS:
        out["ac%d" % s] = synth.se_ac_case(AC_SIZE[0], AC_SIZE[1], s)
    out["noisy"] = synth.se_ac_case(NOISY_SIZE[0], NOISY_SIZE[1], NOISY_SEED, noise=1.0, inj_share=NOISY_INJ_SHARE)
    for row in (W - 1, W, W + 1, 2 * W + 1):                   # the hub's row of Y: row - 1 leaves
        out["star_row%d" % row] = star(row - 1, 20 + row, ref=0)
    # the hub's magnitude column of H at wave_col - 1, wave_col, wave_col + 1 entries (its angle column: 62, 62, 64)
    out["star_col%d" % (C - 1)] = star(C // 2 - 2, 31, hub_mag=1)
    out["star_col%d" % C] = star(C // 2 - 2, 32, hub_mag=2)
    out["star_col%d" % (C + 1)] = star(C // 2 - 1, 33, hub_mag=1)
    for m in (255, 256, 257):
        out["chain_m%d" % m] = chain_rows(m, 40 + m)
    for nnz in (255, 256, 257):
        out["chain_nnz%d" % nnz] = chain_entries(nnz, 50 + nnz)
    net = network(2, [0], [1], 60)
    out["two_buses"] = finish(net, [0], *rows_of(flows=[0], mag=[0, 1]), 60)
    out["ref_first"] = chain(15, 61, ref=(0,), inj=range(15))
    out["ref_middle"] = chain(15, 62, ref=(7,), inj=range(15))
    out["ref_last"] = chain(15, 63, ref=(14,), inj=range(15))
    out["two_refs"] = chain(15, 64, ref=(3, 11))
    out["flows_and_magnitudes"] = chain(15, 65)
    out["injections_one_magnitude"] = chain(8, 66, flows=False, inj=range(8), mag=[0])
    out["repeated"] = repeated()
    out["unsorted"] = chain(15, 67, unsorted=True, inj=range(0, 15, 3))
    out["one_sided"] = chain(15, 68, one_sided=True, inj=range(0, 15, 3))
    out["both_ends"] = both_ends()
    out["no_ends"] = no_ends()
    out["unobservable"] = unobservable()
    out["ac_large"] = synth.se_ac_case(*AC_LARGE)
    assert sorted(out) == sorted(k for k in EVERY if k != "grid_edge")
    return out


@functools.lru_cache(maxsize=None)
def grid_edge():
    """grid_cap * block + 1 entries of H: the entry kernel's lanes loop.  For the kernel tests only."""
    L = limits()
    nnz = L["grid_cap"] * L["block"] + 1
    return chain_entries(nnz, 70, n=(nnz + 10) // 9)


def case_of(name):
    return grid_edge() if name == "grid_edge" else cases()[name]


@functools.lru_cache(maxsize=None)
def plan_of(name):
    case = case_of(name)
    return R.plan_ref(case["n"], case["Yp"], case["Yi"], case["ref"], case["end_from"], case["end_to"], case["kind"], case["where"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """gauss_newton_ref from the flat start, computed once and shared."""
    case = case_of(name)
    return R.gauss_newton_ref(plan_of(name), case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], TOL, MAX_ITERS)


def moved_voltages(case):
    """Voltages off the flat start, for the kernel tests: every derivative is exercised away from its symmetric values."""
    n = case["n"]
    vm = case["vm0"] + 0.01 * np.cos(np.arange(n))
    va = case["va0"] + 0.1 * np.sin(np.arange(n))
    va[case["ref"]] = 0.0
    return vm, va


@functools.lru_cache(maxsize=None)
def bad_data_case():
    """The noisy case with one injection row moved by 40 / sqrt(w): the P injection that the other rows check best
    (the largest 1 - w_i t_i at the reference's solution).  -> (case, planted row)."""
    case = dict(cases()["noisy"])
    P, ref = plan_of("noisy"), reference("noisy")
    Hr = R.jacobian_ref(P, case["Yz"], case["Ye"], ref["vm"], ref["va"])[0]
    bd = R.baddata_ref(P, Hr, case["w"], ref["r"])
    rows = np.flatnonzero(np.isin(case["kind"], (1, 2)))
    bad = int(rows[np.argmax((1.0 - case["w"] * bd["t"])[rows])])
    z = case["z"].copy()
    z[bad] += 40.0 / np.sqrt(case["w"][bad])
    case["z"] = z
    return case, bad
