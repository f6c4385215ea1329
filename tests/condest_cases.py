"""Matrices that take the condition estimator (estimate.hip, condest_run in api.cpp: LAPACK's dlacn2 per matrix, in slots)
and k_slogdet through the paths and over the partition edges that the parity cases never reach, for
tests/test_condest_cases_cpu.py (no device) and tests/test_gpu_condest_edges.py.

Two families.

GENERIC: A = blkdiag(D, c I) of order GEN_N on ONE pattern (a dense leading block of order GEN_K, then a diagonal), D a
seeded random matrix of order <= GEN_K (the rest of the block is c I with stored zeros) and c one of GEN_PADS by the
seed, so that any set of them is a batch.  `search_generic` walks the seeds and keeps, per path class, the first whose every decision has a
relative margin >= MARGIN and whose no-pivot LU in the handle's own order keeps max |L| <= 1 / TOL; the seeds it found
are the table GENERIC.  The CPU module rebuilds every case from its seed and proves the class again.

EXACT: block-diagonal, small unit-triangular integer blocks times powers of two on a diagonal of powers of two.  A^-1
has the same form, so x = A^-1 e_j, A^-T s and every sum of their |x_i| are exact in any order, whatever the pivot order
(every principal minor of a unit-triangular matrix is 1, so static diagonal pivoting in any order meets integers only).
Only J1's sum (over multiples of fl(1 / n)) and J5 round; J1's sum enters one comparison, whose margin the trace bounds.
Ties of |x_i| are legitimate here and planned: the trace lists them, and `last_argmax=True` shows what each decides.
"""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from lacn2_ref import lacn2_traced

MARGIN = 1e-9            # generic cases: every decision of the port is at least this far from its other branch
TOL = 1e-3               # F.factor(Ax, TOL) accepts a pivot while every |multiplier| <= 1 / TOL
U = 2.0 ** -53

EST_CHUNK = 2048         # estimate.hip / cs3_device.hpp: entries per part of k_est_partial
EST_NORM_COLS = 256      # columns per part of k_est_colsums
PART_NT = 256            # threads of k_est_partial: a thread's second entry is 256 past its first
SLOGDET_NT = 1024        # threads of k_slogdet

GEN_N, GEN_K = 300, 32
GEN_PADS = (64.0, 4.0, 1.0, 0.25)


def bound(n, want):
    """|inv_gpu - inv_port| <= 2 (n + 2) u inv_port: both sides sum n non-negative terms in different orders, each sum
    with a relative error of at most (n - 1) u; J5 adds one division and one product."""
    return 2.0 * (n + 2) * U * want


# ----------------------------------------------------------------------------------------------------------- generic --

def generic_pattern(n=GEN_N, k=GEN_K):
    """(Ap, Ai) of a dense leading k x k block followed by a diagonal."""
    Ap = np.concatenate([np.arange(k + 1) * k, k * k + 1 + np.arange(n - k)]).astype(np.int32)
    Ai = np.concatenate([np.tile(np.arange(k), k), np.arange(k, n)]).astype(np.int32)
    return Ap, Ai


def generic_block(seed, spd=False):
    """-> (D, c): the seeded block D (order 3 .. GEN_K; dense normal, triangular plus a weak other half, small integers,
    or sparse) and the value c of the rest of the diagonal."""
    if isinstance(seed, tuple):                                  # (seed, w, delta): seed's block and a blind block after it
        D, pad = generic_block(seed[0], spd)
        k = len(D)
        assert k + 2 <= GEN_K
        B = np.zeros((k + 2, k + 2))
        B[:k, :k] = D
        B[k:, k:] = blind_block(*seed[1:])
        return B, pad
    rng = np.random.default_rng(seed)
    k = int(rng.integers(3, GEN_K + 1))
    kind = seed % 4
    if kind == 0:
        D = rng.standard_normal((k, k))
    elif kind == 1:
        D = np.tril(rng.standard_normal((k, k))) + 0.05 * np.triu(rng.standard_normal((k, k)), 1)
        D[np.diag_indices(k)] = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    elif kind == 2:
        D = rng.integers(-3, 4, (k, k)).astype(np.float64)
        D[np.diag_indices(k)] += rng.choice([-4.0, 4.0], k)
    else:
        D = rng.standard_normal((k, k)) * (rng.uniform(size=(k, k)) < 0.3)
        D[np.diag_indices(k)] = rng.uniform(1.0, 3.0, k) * rng.choice([-1.0, 1.0], k)
    if spd:
        D = D @ D.T + 1e-3 * np.trace(D @ D.T) / k * np.eye(k)
    return D, GEN_PADS[(seed // 4) % 4]


def blind_block(w, delta):
    """P with P^-1 = w [[1 + delta, -1], [-1, 1 + delta]] (symmetric positive definite).  P^-T s = w delta (1, 1) for
    s = (+, +): dlacn2's iteration, which only ever shows it that sign vector, never sees more of it than w delta, while
    J5's alternating vector meets w (2 + delta) (alt_i + alt_i+1): the block that makes J5 win after ANY path of the rest
    of the matrix.  (Without it J5 wins only where the iteration stalls, which it does not on the long paths.)"""
    return np.linalg.inv(w * np.array([[1.0 + delta, -1.0], [-1.0, 1.0 + delta]]))


def generic_values(D, pad, n=GEN_N, k=GEN_K):
    """Ax of blkdiag(D, pad I) on generic_pattern(n, k)."""
    B = pad * np.eye(k)
    B[:len(D), :len(D)] = D
    return np.concatenate([B.T.reshape(-1), np.full(n - k, pad)])     # column by column


def block_solvers(D, pad, n=GEN_N):
    """(solve, solve_t) of blkdiag(D, pad I) through a dense partial-pivoting LU of D."""
    lu, k = sla.lu_factor(D), len(D)

    def make(trans):
        def fn(b):
            x = b / pad
            x[:k] = sla.lu_solve(lu, b[:k], trans=trans)
            return x
        return fn
    return make(0), make(1)


@functools.lru_cache(maxsize=None)
def handle_order(n=GEN_N, k=GEN_K, cholesky=False):
    """The pivot order q of a handle on generic_pattern(n, k) (the analysis needs no device)."""
    from csparse3_amd import csc_hip
    Ap, Ai = generic_pattern(n, k)
    with csc_hip.Factorization(n, n, Ap, Ai, kind=csc_hip.CS3_CHOLESKY if cholesky else csc_hip.CS3_LU) as F:
        return F.ordering()["q"].copy()


def max_multiplier(B):
    """max |L| of the LU of B without pivoting (inf at a zero pivot)."""
    B = np.array(B, dtype=np.float64, copy=True)
    worst = 0.0
    for j in range(len(B) - 1):
        if B[j, j] == 0.0:
            return np.inf
        l = B[j + 1:, j] / B[j, j]
        worst = max(worst, float(np.abs(l).max()))
        B[j + 1:, j + 1:] -= np.outer(l, B[j, j + 1:])
    return worst if B[-1, -1] != 0.0 else np.inf


def lu_accepts(D, pad, n=GEN_N, k=GEN_K):
    """The library's acceptance rule on blkdiag(D, pad I) in the handle's order: only the block has multipliers."""
    q = handle_order(n, k)
    qb = q[q < k]
    B = pad * np.eye(k)
    B[:len(D), :len(D)] = D
    return max_multiplier(B[np.ix_(qb, qb)]) <= 1.0 / TOL


def path_class(solves, tr):
    """What a case is planned by: (solves, J3 exit, J4 exit, J5 won)."""
    return solves, tr["j3_exit"], tr["j4_exit"], bool(tr["j5_won"])


def trace_generic(D, pad, n=GEN_N, **mutant):
    solve, solve_t = block_solvers(D, pad, n)
    return lacn2_traced(n, solve, solve_t, **mutant)


def classify_generic(seed, spd=False):
    """The path class of seed's matrix, or None where |x_i| ties, a margin is below MARGIN, J5 wins by less than 1e-3 or (LU) the
    acceptance rule refuses the factorisation."""
    D, pad = generic_block(seed, spd)
    est, solves, tr = trace_generic(D, pad)
    if tr["nonfinite"] or tr["ties"] or tr["margin"] < MARGIN or (tr["j5_won"] and tr["t"] < tr["est_j3"][-1] * (1.0 + 1e-3)):
        return None
    if not spd and not lu_accepts(D, pad):
        return None
    return path_class(solves, tr)


def generic_case(seed, spd=False, bare=False):
    """-> dict(n, Ap, Ai, Ax, solve, solve_t, D, pad) of seed's matrix; bare: D alone on a dense pattern (n = its order)."""
    D, pad = generic_block(seed, spd)
    if bare:
        k = len(D)
        Ap, Ai = generic_pattern(k, k)
        lu = sla.lu_factor(D)
        return dict(n=k, Ap=Ap, Ai=Ai, Ax=D.T.reshape(-1).copy(), D=D, pad=None,
                    solve=lambda b: sla.lu_solve(lu, b), solve_t=lambda b: sla.lu_solve(lu, b, trans=1))
    Ap, Ai = generic_pattern()
    solve, solve_t = block_solvers(D, pad)
    return dict(n=GEN_N, Ap=Ap, Ai=Ai, Ax=generic_values(D, pad), D=D, pad=pad, solve=solve, solve_t=solve_t)


# name -> (seed or (seed, w, delta) with a blind block, spd, bare, (solves, J3 exit, J4 exit, J5 won)): the first seed of its class that search_generic(range(12000))
# or search_bare(range(300)) returns; 10 solves and the 11 solves that end at the cap with x[jlast] != max |x_i| came out
# of longer runs of the same search (the first in range(225000, 300000) and in range(1000000, 1400000)).
GENERIC = {
    "4 same signs": (1, False, False, (4, "same_signs", None, False)),
    "5": (0, False, False, (5, None, "repeat", False)),
    "6": (587, False, False, (6, "same_signs", None, False)),
    "7": (3, False, False, (7, None, "repeat", False)),
    "8": (9699, False, False, (8, "same_signs", None, False)),
    "9": (639, False, False, (9, None, "repeat", False)),
    "10": (236810, False, False, (10, "same_signs", None, False)),
    "11": (9754, False, False, (11, None, "repeat", False)),
    "11 cap": (1294922, False, False, (11, None, "cap", False)),
    "J5 wins": (200, False, True, (4, "same_signs", None, True)),
    # 11 solves AND J5 decides (blind_block): the only matrices on which one slot too few changes the result
    "11 J5 wins": ((80786, 1024.0, 2.0 ** -9), False, False, (11, None, "repeat", True)),
    "11 cap J5 wins": ((1294922, 2048.0, 2.0 ** -10), False, False, (11, None, "cap", True)),
}
SPD = {
    "spd 4": (23, True, False, (4, "same_signs", None, False)),
    "spd 5": (0, True, False, (5, None, "repeat", False)),
    "spd 7": (2, True, False, (7, None, "repeat", False)),
    "spd 9": (41, True, False, (9, None, "repeat", False)),
    "spd 11": (5966, True, False, (11, None, "repeat", False)),
    "spd 11 J5 wins": ((5966, 1024.0, 2.0 ** -9), True, False, (11, None, "repeat", True)),
}


def search_generic(seeds, spd=False):
    """{class: first seed of `seeds` in it} (the committed search; about 1 ms per seed)."""
    found = {}
    for seed in seeds:
        c = classify_generic(seed, spd)
        if c is not None:
            found.setdefault(c, seed)
    return found


def search_bare(seeds):
    """The same over D alone (n = its order), where J5's t = 2 ||A^-1 alt||_1 / (3 n) is not diluted by a diagonal."""
    found = {}
    for seed in seeds:
        g = generic_case(seed, bare=True)
        est, solves, tr = lacn2_traced(g["n"], g["solve"], g["solve_t"])
        if tr["nonfinite"] or tr["ties"] or tr["margin"] < MARGIN or (tr["j5_won"] and tr["t"] < tr["est_j3"][-1] * (1.0 + 1e-3)):
            continue
        q = handle_order(g["n"], g["n"])
        if max_multiplier(g["D"][np.ix_(q, q)]) <= 1.0 / TOL:
            found.setdefault(path_class(solves, tr), seed)
    return found


# ------------------------------------------------------------------------------------------------------------- exact --

def exact_block(seed, k=3):
    """A seeded block B = T S of order k: T unit lower (or upper) triangular with entries in -2 .. 2, S = diag(+-2^e),
    e in -1 .. 1."""
    rng = np.random.default_rng(seed)
    T = np.tril(rng.integers(-2, 3, (k, k)), -1).astype(np.float64) + np.eye(k)
    if rng.integers(2):
        T = T.T.copy()
    S = np.ldexp(rng.choice([-1.0, 1.0], k), rng.integers(-1, 2, k))
    return T * S[None, :]


def exact_matrix(n, blocks, diag):
    """A = the diagonal `diag` (n values +-2^e) with the dense blocks [(first index, B)] laid over it, as
    dict(n, Ap, Ai, Ax, A, solve, solve_t); the blocks' zeros are not stored.  The inverse is built block by block and
    checked: B B^-1 = B^-1 B = I in float64 with every entry a small multiple of 2^-12, hence exactly."""
    diag = np.array(diag, dtype=np.float64, copy=True)
    rows, cols, vals, irows, icols, ivals = [], [], [], [], [], []
    inblock = np.zeros(n, dtype=bool)
    for pos, B in blocks:
        k = len(B)
        assert 0 <= pos and pos + k <= n and not inblock[pos:pos + k].any()
        inblock[pos:pos + k] = True
        Binv = np.linalg.inv(B)
        Binv = np.round(Binv * 4096.0) / 4096.0
        assert np.array_equal(B @ Binv, np.eye(k)) and np.array_equal(Binv @ B, np.eye(k)) and np.abs(Binv).max() < 2.0 ** 20
        for M, (r, c, v) in ((B, (rows, cols, vals)), (Binv, (irows, icols, ivals))):
            i, j = np.nonzero(M)
            r.append(i + pos); c.append(j + pos); v.append(M[i, j])
    rest = np.flatnonzero(~inblock)
    m, e = np.frexp(np.abs(diag[rest]))
    assert np.all(m == 0.5), "the diagonal is +-2^e"
    for (r, c, v), d in (((rows, cols, vals), diag[rest]), ((irows, icols, ivals), 1.0 / diag[rest])):
        r.append(rest); c.append(rest); v.append(d)
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    Ainv = sp.csr_matrix((np.concatenate(ivals), (np.concatenate(irows), np.concatenate(icols))), shape=(n, n))
    AinvT = Ainv.T.tocsr()
    return dict(n=n, Ap=A.indptr.astype(np.int32), Ai=A.indices.astype(np.int32), Ax=A.data.copy(), A=A,
                solve=lambda b: Ainv @ b, solve_t=lambda b: AinvT @ b, blocks=blocks)


def is_pow2(v):
    return v > 0.0 and np.frexp(v)[0] == 0.5


def tie_case(n, pos, partner, step, seed, pad=4.0, norm_col=None, second=None):
    """The exact matrix of order n with exact_block(seed) at `pos` on a diagonal of `pad`, and at index `partner` the
    value 1 / v, v = the largest |x_i| the port meets at its `step` ("J2": the first argmax; "J4": the second): the
    partner then TIES with the block's entry there.  norm_col: that diagonal entry becomes 2^12 (the largest column of A;
    its 2^-12 in A^-1 decides nothing).  second: (pos, seed) of one more block.  -> (case, v), or None where v is no
    power of two, the block's own largest entry is not unique or no such step is met."""
    B = exact_block(seed)
    blocks = [(pos, B)] + ([(second[0], exact_block(second[1]))] if second else [])
    diag = np.full(n, pad)
    if norm_col is not None:
        diag[norm_col] = 4096.0
    c = exact_matrix(n, blocks, diag)
    est, solves, tr = lacn2_traced(n, c["solve"], c["solve_t"])
    k = 0 if step == "J2" else 1
    if len(tr["amax"]) <= k or tr["ties"]:
        return None
    v = tr["amax"][k]
    if not is_pow2(v) or 1.0 / v == pad:
        return None
    diag[partner] = 1.0 / v
    return exact_matrix(n, blocks, diag), v


def tie_facts(c):
    """(est, solves, trace) of the port on an exact case with the first and with the last argmax."""
    first = lacn2_traced(c["n"], c["solve"], c["solve_t"])
    last = lacn2_traced(c["n"], c["solve"], c["solve_t"], last_argmax=True)
    return first, last


def find_tie(n, pos, partner, step, seeds, **kw):
    """The first seed whose tie_case has the planned tie (block entry and partner, at `step`, nowhere else), a J1
    comparison with a margin >= MARGIN, no win of J5 and a different estimate with the last argmax."""
    for seed in seeds:
        got = tie_case(n, pos, partner, step, seed, **kw)
        if got is None:
            continue
        c, v = got
        (est, solves, tr), (est_l, _, _) = tie_facts(c)
        want_at = 1 if step == "J2" else 3
        if (len(tr["ties"]) == 1 and tr["ties"][0][0] == want_at and tr["ties"][0][1][-1] == partner
                and len(tr["ties"][0][1]) == 2 and pos <= tr["ties"][0][1][0] < pos + len(c["blocks"][0][1])
                and tr["margin"] >= MARGIN and not tr["j5_won"] and est_l != est):
            return seed
    return None


def block_only(seed, k):
    """exact_block(seed, k) as the whole matrix (k a power of two: J1's 1 / n is exact too)."""
    return exact_matrix(k, [(0, exact_block(seed, k))], np.ones(k))


def find_no_growth(k, seeds):
    """The first seed whose block_only leaves J3 by est == estold with other signs (dlacn2's `<=`), where `<` goes on to a
    different estimate."""
    for seed in seeds:
        c = block_only(seed, k)
        est, solves, tr = lacn2_traced(k, c["solve"], c["solve_t"])
        if tr["j3_exit"] == "no_growth" and lacn2_traced(k, c["solve"], c["solve_t"], strict_growth=True)[0] != est:
            return seed
    return None


def straddle_case(n, pos, seed, pad=4.0):
    return exact_matrix(n, [(pos, exact_block(seed))], np.full(n, pad))


def find_straddle(n, pos, seeds, edge=EST_CHUNK):
    """The first seed whose block at pos .. pos + 2 (across `edge`) changes sign at the first J3 only at indices >= edge,
    after which the estimate still grows: a part 1 that loses its flag ends the estimate one round early."""
    for seed in seeds:
        c = straddle_case(n, pos, seed)
        est, solves, tr = lacn2_traced(n, c["solve"], c["solve_t"])
        d = tr["sign_diff"][0] if tr["sign_diff"] else []
        if (d and min(d) >= edge and solves >= 5 and not tr["ties"] and tr["margin"] >= MARGIN and not tr["j5_won"]
                and est != tr["est_j3"][0]):
            return seed
    return None


def pair_case(n, pos, pos2, seed, seed2, pad=4.0, norm_col=None):
    """Two blocks, exact_block(seed) at pos and exact_block(seed2) at pos2 > pos.  (A single diagonal entry cannot tie at
    J4 alone: its |x_i| is the same in every A^-T s, so it would have won J2 outright.)"""
    diag = np.full(n, pad)
    if norm_col is not None:
        diag[norm_col] = 4096.0
    return exact_matrix(n, [(pos, exact_block(seed)), (pos2, exact_block(seed2))], diag)


def find_pair_tie(n, pos, pos2, seeds, **kw):
    """The first (seed, seed2) whose only tie is at the first J4, between an entry of each block, decided differently by
    the last argmax, with every other margin >= MARGIN and no win of J5."""
    for seed in seeds:
        for seed2 in seeds:
            c = pair_case(n, pos, pos2, seed, seed2, **kw)
            est, solves, tr = lacn2_traced(n, c["solve"], c["solve_t"])
            if (len(tr["ties"]) == 1 and tr["ties"][0][0] == 3 and len(tr["ties"][0][1]) == 2
                    and pos <= tr["ties"][0][1][0] < pos + 3 and pos2 <= tr["ties"][0][1][1] < pos2 + 3
                    and tr["margin"] >= MARGIN and not tr["j5_won"]
                    and lacn2_traced(n, c["solve"], c["solve_t"], last_argmax=True)[0] != est):
                return seed, seed2
    return None


ISSUE_EXAMPLE = np.array([[1.0, 0, 0, 0], [0, 2, 0, 0], [0, -4, 2, 0], [0, 2, 0, 2]])   # first argmax 1.0, last 2.0
BIG_N = 64 * EST_CHUNK + EST_CHUNK + 1                                                # 66 parts: k_est_finish's second round

# name -> (kind, arguments): "tie" (n, pos, partner, step, seed, norm_col) -> tie_case; "pair" (n, pos, pos2, seed, seed2,
# norm_col) -> pair_case; "straddle" (n, pos, seed); "block" (seed, k) -> block_only; "dense" (matrix).  The seeds are
# the first that find_tie / find_pair_tie / find_straddle / find_no_growth return over range(3000) (pairs: range(400)).
EXACT = {
    "issue example": ("dense", (ISSUE_EXAMPLE,)),
    "no growth n2": ("block", (406, 2)),
    "no growth n4": ("block", (3230, 4)),
    "tie J2 n2047 entry 0": ("tie", (2047, 0, 2046, "J2", 14, 255)),
    "tie J2 n2048 stride": ("tie", (2048, 254, 2047, "J2", 14, 258)),
    "tie J2 n2048 entry 255": ("tie", (2048, 253, 256, "J2", 14, 257)),
    "tie J2 n4097 chunk edge": ("tie", (4097, 2045, 2048, "J2", 14, 4095)),
    "tie J2 n2049 chunk 1": ("tie", (2049, 2044, 2048, "J2", 14, 2047)),
    "tie J2 n4097 straddle": ("tie", (4097, 2046, 4096, "J2", 14, 4095)),
    "tie J2 n4097 norm last": ("tie", (4097, 0, 300, "J2", 14, 4096)),
    "tie J4 n2047 stride": ("pair", (2047, 254, 300, 110, 301, 257)),
    "tie J4 n2048 ends": ("pair", (2048, 0, 2045, 110, 301, 256)),
    "tie J4 n4097 straddle": ("pair", (4097, 2047, 2050, 110, 301, 255)),
    "tie J4 n4097 last": ("pair", (4097, 2047, 4094, 110, 301, 255)),
    "straddle n2049": ("straddle", (2049, 2046, 85)),
    "straddle n4097": ("straddle", (4097, 2046, 85)),
    "big J2 part 64": ("tie", (BIG_N, 64 * EST_CHUNK + 100, 65 * EST_CHUNK, "J2", 14, 16384 + 255)),
    "big J2 same lane": ("tie", (BIG_N, EST_CHUNK + 10, 65 * EST_CHUNK, "J2", 14, 16384 + 255)),
    "big J4": ("pair", (BIG_N, 64 * EST_CHUNK + 100, 65 * EST_CHUNK - 2, 110, 301, 20000)),
}


def exact_case(name):
    kind, a = EXACT[name]
    if kind == "dense":
        return exact_matrix(len(a[0]), [(1, a[0][1:, 1:])], np.diag(a[0]).copy())
    if kind == "block":
        return block_only(*a)
    if kind == "straddle":
        return straddle_case(*a)
    if kind == "pair":
        return pair_case(*a[:5], norm_col=a[5])
    n, pos, partner, step, seed, norm_col = a
    return tie_case(n, pos, partner, step, seed, norm_col=norm_col)[0]


def planned(tr, solves):
    """What a test asserts of a run's trace: (solves, J3 exit, J4 exit, J5 won, ties)."""
    return path_class(solves, tr) + (tr["ties"],)


# what the port does on every exact case: (solves, J3 exit, J4 exit, J5 won, ties); every GPU test asserts it again from
# the trace of its own run
PLANNED = {
    "issue example": (4, "same_signs", None, False, [(1, [0, 1])]),
    "no growth n2": (4, "no_growth", None, True, [(1, [0, 1]), (2, "est")]),
    "no growth n4": (4, "no_growth", None, True, [(1, [0, 1, 2, 3]), (2, "est")]),
    "tie J2 n2047 entry 0": (5, None, "repeat", False, [(1, [2, 2046])]),
    "tie J2 n2048 stride": (5, None, "repeat", False, [(1, [256, 2047])]),
    "tie J2 n2048 entry 255": (5, None, "repeat", False, [(1, [255, 256])]),
    "tie J2 n4097 chunk edge": (5, None, "repeat", False, [(1, [2047, 2048])]),
    "tie J2 n2049 chunk 1": (5, None, "repeat", False, [(1, [2046, 2048])]),
    "tie J2 n4097 straddle": (5, None, "repeat", False, [(1, [2048, 4096])]),
    "tie J2 n4097 norm last": (5, None, "repeat", False, [(1, [2, 300])]),
    "tie J4 n2047 stride": (9, None, "repeat", False, [(3, [254, 301])]),
    "tie J4 n2048 ends": (9, None, "repeat", False, [(3, [0, 2046])]),
    "tie J4 n4097 straddle": (9, None, "repeat", False, [(3, [2047, 2051])]),
    "tie J4 n4097 last": (9, None, "repeat", False, [(3, [2047, 4095])]),
    "straddle n2049": (7, None, "repeat", False, []),
    "straddle n4097": (7, None, "repeat", False, []),
    "big J2 part 64": (5, None, "repeat", False, [(1, [131174, 133120])]),
    "big J2 same lane": (5, None, "repeat", False, [(1, [2060, 133120])]),
    "big J4": (9, None, "repeat", False, [(3, [131172, 133119])]),
}


# ----------------------------------------------------------------------------------------------------------- slogdet --

SLOGDET_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def slogdet_matrix(n, seed=0, spd=False):
    """A diagonal in (0.5, 2) with up to eight 2 x 2 blocks at (3 i, 3 i + 1) -> (Ap, Ai, Ax, dpos): dpos[j] = the
    position in Ax of the diagonal entry of column j.  spd: the blocks are symmetric and positive definite."""
    rng = np.random.default_rng(1000 + seed + n)
    d = rng.uniform(0.5, 2.0, n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [d]
    for i in range(min(8, (n - 1) // 3)):
        a, b = 3 * i, 3 * i + 1
        off = rng.uniform(0.2, 0.4, 2) * (1.0 if spd else -1.0) ** np.arange(2)
        if spd:
            off[1] = off[0]
        rows.append(np.array([b, a])); cols.append(np.array([a, b])); vals.append(off)
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    Ap, Ai = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    dpos = np.array([Ap[j] + int(np.flatnonzero(Ai[Ap[j]:Ap[j + 1]] == j)[0]) for j in range(n)])
    return Ap, Ai, A.data.copy(), dpos


def pure_diagonal(n):
    """The columns of slogdet_matrix(n) outside every block: their pivot is the entry of A itself."""
    inblock = np.zeros(n, dtype=bool)
    for i in range(min(8, (n - 1) // 3)):
        inblock[3 * i:3 * i + 2] = True
    return ~inblock
