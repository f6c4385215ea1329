"""Engineered cases of the extra-precise refinement (tests/test_xp_cpu.py, tests/test_gpu_refine_xp.py,
tests/golden/make_xp_refs.py).

chain(nb, m, c, seed): nb diagonal blocks fl(L U) of order m, L unit lower bidiagonal with subdiagonal c + 0.1 u, U upper
bidiagonal with diagonal 1 + 0.1 u and superdiagonal c + 0.1 u (u uniform from the seeded generator); consecutive blocks are
coupled by the entries 0.37 (above the diagonal) and 0.41 (below), which continue the tridiagonal.  The inverse of a bidiagonal factor grows like c^m, so
cond(A) is about c^(2 m) while natural-order LU with diagonal pivots reproduces factors close to the L, U multiplied.  The
products are written out entry by entry (no BLAS), so the arrays are the same bits on every machine.

Every case is a namedtuple Case(name, n, Ap, Ai, Ax, Ax0, b, kind, trans): CSC with sorted rows, Ax the values to refine
against, Ax0 the values to factorise (the same array unless the case says otherwise), one right-hand side."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name n Ap Ai Ax Ax0 b kind trans")

C_ILL = 3.0
SHAPES = [(4, 8), (4, 11), (3, 13), (3, 15), (3, 17), (2, 20)]          # cond_1 from 1e7 to 3e17 at c = 3
SEED = 4
# The two shapes at the edge of 1 / eps react to HOW the inner solver rounds.  Their seeds were chosen among 1 .. 60 so that
# SuperLU and the four arithmetic variants of tridiagonal_solver() below (division or reciprocal pivots, with or without
# FMA) agree on what happens: (3, 17) with seed 4 converges in 6 to 8 corrections under all five, (2, 20) with seed 19 is
# still iterating after 10 under all five, rates 0.2 to 0.4 (tests/test_xp_cpu.py asserts both).
SHAPE_SEED = {(2, 20): 19}


def _dense_csc(D, mask):
    """CSC (rows sorted) of the entries of D that mask marks."""
    n = D.shape[0]
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        rows = np.nonzero(mask[:, j])[0]
        Ai.extend(rows); Ax.extend(D[rows, j])
        Ap.append(len(Ai))
    return np.array(Ap, dtype=np.int32), np.array(Ai, dtype=np.int32), np.array(Ax, dtype=np.float64)


def chain_dense(nb, m, c, seed, noise=0.1, n_pad=None):
    """chain() as a dense matrix and the mask of its stored entries, every product and sum rounded on its own.  The two
    coupling entries of blocks b, b + 1 continue the tridiagonal: 0.37 from the last row of block b to the first column of
    block b + 1, 0.41 mirrored below the diagonal.  n_pad: continued by an identity block up to that order."""
    rng = np.random.default_rng(seed)
    n = nb * m
    N = n if n_pad is None else n_pad
    D, mask = np.zeros((N, N)), np.zeros((N, N), dtype=bool)
    idx = np.arange(m - 1)
    for blk in range(nb):
        lo = blk * m
        l = c + noise * rng.random(m - 1)            # subdiagonal of L
        d = 1.0 + noise * rng.random(m)              # diagonal of U
        s = c + noise * rng.random(m - 1)            # superdiagonal of U
        D[lo, lo] = d[0]
        D[lo + 1 + idx, lo + 1 + idx] = l * s + d[1:]
        D[lo + 1 + idx, lo + idx] = l * d[:-1]
        D[lo + idx, lo + 1 + idx] = s
        if blk + 1 < nb:
            D[lo + m - 1, lo + m] = 0.37
            D[lo + m, lo + m - 1] = 0.41
    for i in range(n, N):
        D[i, i] = 1.0
    mask = D != 0.0
    return D, mask


def rhs(n, seed):
    return np.random.default_rng(seed + 1000).standard_normal(n)


def chain(nb, m, c=C_ILL, seed=None, trans=False, name=None):
    seed = SHAPE_SEED.get((nb, m), SEED) if seed is None else seed
    n = nb * m
    Ap, Ai, Ax = _dense_csc(*chain_dense(nb, m, c, seed))
    return Case(name or "chain_%d_%d" % (nb, m), n, Ap, Ai, Ax, Ax, rhs(n, seed), "lu", trans)


def chain_spd(nb=4, m=6, c=C_ILL, seed=SEED):
    """Blocks fl(L L') with L lower bidiagonal (diagonal 1 + 0.1 u, subdiagonal c + 0.1 u); the last variables of consecutive
    blocks are coupled by 0.37, symmetrically (only the last pivot of a block feels it: the matrix stays positive
    definite).  The full symmetric matrix is stored."""
    rng = np.random.default_rng(seed + 7)
    n = nb * m
    D = np.zeros((n, n))
    idx = np.arange(m - 1)
    for blk in range(nb):
        lo = blk * m
        d = 1.0 + 0.1 * rng.random(m)
        l = c + 0.1 * rng.random(m - 1)
        dia = d * d
        dia[1:] = l * l + dia[1:]
        D[lo + np.arange(m), lo + np.arange(m)] = dia
        D[lo + 1 + idx, lo + idx] = l * d[:-1]
        D[lo + idx, lo + 1 + idx] = l * d[:-1]
        if blk + 1 < nb:
            D[lo + m - 1, lo + 2 * m - 1] = D[lo + 2 * m - 1, lo + m - 1] = 0.37
    Ap, Ai, Ax = _dense_csc(D, D != 0.0)
    return Case("chain_spd", n, Ap, Ai, Ax, Ax, rhs(n, seed + 7), "chol", False)


def stale_pair(seed=SEED):
    """Factors of A0 = A (1 + 1e-12 noise), refined against A."""
    base = chain(4, 8, seed=seed)
    noise = np.random.default_rng(seed + 11).standard_normal(base.Ax.size)
    return base._replace(name="stale", Ax0=base.Ax * (1.0 + 1e-12 * noise))


def hopeless_pair(seed=SEED):
    """c = 0.5, factors of A0 = A (1 + 0.3 noise): the corrections do not shrink."""
    base = chain(4, 8, c=0.5, seed=seed)
    noise = np.random.default_rng(seed + 13).standard_normal(base.Ax.size)
    return base._replace(name="hopeless", Ax0=base.Ax * (1.0 + 0.3 * noise))


def row_permutation(n, seed=SEED):
    """Row i of the chain goes to row perm[i] of the permuted case."""
    return np.random.default_rng(seed + 17).permutation(n)


def permuted(seed=SEED):
    """The (4, 8) chain with its rows permuted (for a matched handle): no diagonal to pivot on.  -> Case (kind "matched")."""
    base = chain(4, 8, seed=seed)
    n = base.n
    perm = row_permutation(n, seed)
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        rows = perm[base.Ai[base.Ap[j]:base.Ap[j + 1]]]
        vals = base.Ax[base.Ap[j]:base.Ap[j + 1]]
        order = np.argsort(rows)
        Ai.extend(rows[order]); Ax.extend(vals[order])
        Ap.append(len(Ai))
    Ax = np.array(Ax, dtype=np.float64)
    b = np.zeros(n)
    b[perm] = base.b
    return Case("permuted", n, np.array(Ap, dtype=np.int32), np.array(Ai, dtype=np.int32), Ax, Ax, b, "matched", False)


def natural_pivots(case):
    """The pivots of natural-order LU without pivoting (dense host elimination, n is small)."""
    A = dense(case, case.Ax0)
    for k in range(case.n - 1):
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return np.diag(A).copy()


def perturbed(seed=SEED):
    """One block of order 11 (no coupling: every pivot is positive) with a delta just above its smallest pivot: exactly that pivot is replaced, by a relative change of
    2^-30, far above the rounding differences between this recurrence and the device's pivots and far below the gap to the
    next pivot.  -> (Case, delta)."""
    base = chain(1, 11, seed=seed)._replace(name="perturbed")
    piv = natural_pivots(base)
    i = int(np.argmin(np.abs(piv)))
    low = np.sort(np.abs(piv))
    assert piv[i] > 0 and low[1] > low[0] * (1.0 + 2.0 ** -20)
    delta = float(low[0] * (1.0 + 2.0 ** -30))
    # what the device then holds are the factors of A with a_ii raised by delta - p_i: pivot i becomes delta, the pivots
    # before it are untouched, those after it follow from it.  That matrix is Ax0 (the CPU tests factorise it).
    Ax0 = base.Ax.copy()
    at = base.Ap[i] + list(base.Ai[base.Ap[i]:base.Ap[i + 1]]).index(i)
    Ax0[at] += delta - piv[i]
    return base._replace(Ax0=Ax0), delta


def arrowhead(n=200, seed=SEED):
    """Order n with a full first row, a full first column and a diagonal; rows in DESCENDING order inside every column
    (unsorted storage).  Residual tests only.  -> (n, Ap, Ai, Ax)."""
    rng = np.random.default_rng(seed + 19)
    Ap, Ai = [0], []
    for j in range(n):
        rows = list(range(n)) if j == 0 else [0, j]
        Ai.extend(sorted(rows, reverse=True))
        Ap.append(len(Ai))
    Ax = rng.standard_normal(len(Ai))
    return n, np.array(Ap, dtype=np.int32), np.array(Ai, dtype=np.int32), Ax


def one_by_one():
    return Case("n1", 1, np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([3.0]), np.array([3.0]),
                np.array([1.0]), "lu", False)


def refinement_cases():
    """Every case that is refined and has a fixture solution, by name."""
    cases = [chain(nb, m) for nb, m in SHAPES]
    cases.append(chain(4, 11, trans=True, name="chain_4_11_t"))
    cases += [chain_spd(), stale_pair(), hopeless_pair(), permuted(), perturbed()[0], one_by_one()]
    return {c.name: c for c in cases}


def padded_pair():
    """(4, 8) values and (3, 17) values on ONE pattern, the union of the two (explicit zeros where one has no entry; the
    smaller matrix continues with an identity block): a batch of two whose systems need different numbers of corrections.
    -> (n, Ap, Ai, AX [2, nnz], B [2, n])."""
    big, small = chain(3, 17), chain(4, 8)
    n = big.n
    Db, mb = chain_dense(3, 17, C_ILL, SEED)
    Ds, ms = chain_dense(4, 8, C_ILL, SEED, n_pad=n)
    Ap, Ai, Ax_small = _dense_csc(Ds, mb | ms)
    _, _, Ax_big = _dense_csc(Db, mb | ms)
    b_small = np.zeros(n)
    b_small[:small.n] = small.b
    return n, Ap, Ai, np.stack([Ax_small, Ax_big]), np.stack([b_small, big.b])


def dense(case, Ax=None):
    A = np.zeros((case.n, case.n))
    Ax = case.Ax if Ax is None else Ax
    for j in range(case.n):
        A[case.Ai[case.Ap[j]:case.Ap[j + 1]], j] = Ax[case.Ap[j]:case.Ap[j + 1]]
    return A


def tridiagonal_solver(case, recip, fma):
    """r -> A0^-1 r by natural-order LU of a TRIDIAGONAL case without pivoting, in one of four arithmetics: multipliers and
    back-substitution by division or by the pivot's reciprocal (what the device forms), updates c - a b rounded twice or
    once (fma, emulated exactly with fractions).  For seeing what depends on the inner solver's rounding."""
    from fractions import Fraction as Fr
    n, A = case.n, dense(case, case.Ax0)
    assert not np.triu(A, 2).any() and not np.tril(A, -2).any() and not case.trans
    d, sub, sup = np.diag(A).copy(), np.diag(A, -1).copy(), np.diag(A, 1).copy()

    def msub(c, a, b):
        return float(Fr(float(c)) - Fr(float(a)) * Fr(float(b))) if fma else c - a * b

    p, l = np.zeros(n), np.zeros(max(n - 1, 0))
    p[0] = d[0]
    for i in range(n - 1):
        l[i] = sub[i] * (1.0 / p[i]) if recip else sub[i] / p[i]
        p[i + 1] = msub(d[i + 1], l[i], sup[i])
    rp = 1.0 / p

    def solve(r):
        y = np.array(r, dtype=np.float64)
        for i in range(n - 1):
            y[i + 1] = msub(y[i + 1], l[i], y[i])
        x = y.copy()
        x[n - 1] = x[n - 1] * rp[n - 1] if recip else x[n - 1] / p[n - 1]
        for i in range(n - 2, -1, -1):
            t = msub(y[i], sup[i], x[i + 1])
            x[i] = t * rp[i] if recip else t / p[i]
        return x

    return solve


def superlu_solver(case):
    """r -> op(A0)^-1 r with SuperLU in double, natural order, diagonal pivots, no equilibration: the factors the device
    would hold."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    A0 = sp.csc_matrix((case.Ax0, case.Ai, case.Ap), shape=(case.n, case.n))
    if case.kind == "matched":
        # the matching of the device puts the rows back (the chain's diagonal is the maximum-product transversal): the held
        # factors are those of the chain itself, and a residual r of the permuted system is r[perm] in the chain's rows
        base, perm = chain(4, 8), row_permutation(case.n)
        inner = superlu_solver(base)
        return lambda r: inner(np.asarray(r)[perm])
    lu = spla.splu(A0, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(Equil=False, SymmetricMode=False))
    return (lambda r: lu.solve(r, trans="T")) if case.trans else lu.solve
