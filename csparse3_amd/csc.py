"""Host-side mirror of the reference's matrix class for the factor/solve path.

`CscMat` keeps the reference's constructor, attributes and accessors
(/root/reference/src/CSparse3/csc.py:44-141, 459-538: m, n, indptr, indices,
data, nzmax, get_nnz, shape, copy, todense, t) and adds the entry points the
reference lacks at this snapshot: lu / chol / solve on the
object, lusol / cholsol / lsolve / usolve as module functions.  Kernel names
are star-imported from the backend module exactly as csc.py:34-41 does, so
`from csparse3_amd.csc import *` exposes csc_lu_f, csc_lsolve_f, ... next to
the class.
"""
import hashlib

import numpy as np

from csparse3_amd import __config__

if __config__.BACKEND != "hip":
    raise ImportError("csparse3_amd has one numeric backend, 'hip' (got %r); there is no CPU fallback"
                      % __config__.BACKEND)
from csparse3_amd.csc_hip import *                       # noqa: F401,F403  (kernel names, reference style)
from csparse3_amd import csc_hip as _k


class CscMat:
    """Matrix in compressed-column form (same fields as the reference's CscMat)."""

    def __init__(self, m=0, n=0, nz_max=0, indptr=None, indices=None, data=None, zeros=False):
        self.m, self.n = m, n
        if indptr is None:
            self.nzmax = max(nz_max, 1)
            alloc = np.zeros if zeros else np.empty
            self.indptr = alloc(n + 1, dtype=np.int32)
            self.indices = alloc(nz_max, dtype=np.int32)
            self.data = alloc(nz_max, dtype=np.float64)
        else:
            self.indptr, self.indices, self.data = indptr, indices, data
            self.nzmax = len(self.data)
        self._factorization = None

    # ---- what the reference class already offers, kept for drop-in use
    def get_nnz(self):
        return self.indptr[self.n]                       # csc.py:480: nnz is indptr[n], not len(data)

    @property
    def shape(self):
        return self.m, self.n

    def copy(self):
        return CscMat(self.m, self.n, indptr=self.indptr.copy(), indices=self.indices.copy(),
                      data=self.data.copy())

    def todense(self):
        val = np.zeros((self.m, self.n), dtype=np.result_type(np.asarray(self.data).dtype, np.float64))     # (complex data: complex128)
        for j in range(self.n):
            for p in range(self.indptr[j], self.indptr[j + 1]):
                val[self.indices[p], j] = self.data[p]
        return val

    # ---- operators of the reference class whose kernels live on the device (csc.py:143-346, 425-457)
    def __getitem__(self, key):
        """The eight slicing forms of the reference (csc.py:143-283; src/test/test2_slicing.py:6-79), same kernels, same
        results: A[a, :], A[:, b], A[:, :], A[a, list], A[list, b], A[:, list], A[list, :], A[list, list].  The row
        selections run cs3_csc_sub_matrix on the device and keep the reference's row numbering (a running match counter:
        csc_numba.py:464-502, 541-578 -- csc_sub_matrix_rows is csc_sub_matrix over all columns, loop for loop); a column
        selection copies whole columns with their original row indices (csc_sub_matrix_cols, csc_numba.py:505-538)."""
        from collections.abc import Iterable
        if not isinstance(key, tuple):
            raise Exception('The indices must be a tuple :/')
        a, b = key
        is_int = lambda v: isinstance(v, (int, np.integer))
        as_idx = lambda v: np.asarray([v] if is_int(v) else v, dtype=np.int32)
        if is_int(a) and is_int(b):
            raise NotImplementedError('Single value extraction not implemented')       # csc.py:150
        if isinstance(a, slice) and isinstance(b, slice):
            return self                                                                # csc.py:180-182
        if isinstance(a, slice):                         # (:, b) / (:, list_b): whole columns
            cols = as_idx(b)
            Bp, Bi, Bx = _sub_matrix_cols(self.indptr, self.indices, self.data, cols)
            return CscMat(self.m, len(cols), indptr=Bp, indices=Bi, data=Bx)
        if not (is_int(a) or isinstance(a, Iterable)) or not (is_int(b) or isinstance(b, slice) or isinstance(b, Iterable)):
            raise Exception('The indices must be a tuple :/')
        rows = as_idx(a)
        cols = np.arange(self.n, dtype=np.int32) if isinstance(b, slice) else as_idx(b)      # (a, :) / (list_a, :): every column
        _, Bp, Bi, Bx = _k.csc_sub_matrix(self.m, self.nzmax, self.indptr, self.indices, self.data, rows, cols)
        return CscMat(len(rows), len(cols), indptr=Bp, indices=Bi, data=Bx)

    def __setitem__(self, key, value):
        raise Exception('Setting values is not allowed in a CSC Matrix, use a Lil Matrix instead and convert it to CSC')

    def _add(self, other, beta):
        if isinstance(other, CscMat):
            assert other.m == self.m                     # csc.py:309-310
            assert other.n == self.n
            m, n, Cp, Ci, Cx = _k.csc_add_ff(self.m, self.n, self.indptr, self.indices, self.data,
                                             other.m, other.n, other.indptr, other.indices, other.data, 1.0, beta)
            return CscMat(m, n, indptr=Cp, indices=Ci, data=Cx)
        if isinstance(other, (float, int)):
            raise NotImplementedError('Adding a nonzero scalar to a sparse matrix would make it a dense matrix.')
        raise NotImplementedError('Type not supported')

    def __add__(self, other):
        """A + B on the device through the package's own kernel csc_add_ff (csc_numba.py:183-219: entries in its order,
        explicit zeros kept); the reference's operator goes through SciPy's csc_plus_csc (csc.py:301-322) -- the dense
        results are equal, which is what its test compares (src/test/test1_operations.py:12-72)."""
        return self._add(other, 1.0)

    def __sub__(self, other):
        return self._add(other, -1.0)

    def __neg__(self):
        return self.__mul__(-1.0)                        # csc.py:425-430

    def __eq__(self, other):
        """Same shape and the same three arrays, entry by entry (csc.py:432-457)."""
        if not isinstance(other, CscMat) or self.shape != other.shape:
            return False
        same = lambda x, y: all(p == q for p, q in zip(x, y))
        return bool(same(self.indices, other.indices) and same(self.indptr, other.indptr) and same(self.data, other.data))

    __hash__ = None

    def __mul__(self, other):
        """A * B for a CscMat, on the device through the package's own kernel csc_multiply_ff (entries in its order, not
        sorted; the reference's operator goes through SciPy's csc_matmat passes, csc.py:354-370 -- the dense results are
        equal, which is what its test compares); A * x for a vector or an [n, k] block (csc.py:372-415 semantics)."""
        if isinstance(other, CscMat):
            return self.dot(other)
        if isinstance(other, np.ndarray):
            return _k.csc_mat_vec_ff(self.m, self.n, self.indptr, self.indices, self.data, other)
        if isinstance(other, (int, float)):
            C = self.copy()
            C.data *= other
            return C
        raise Exception("Type not supported")

    def dot(self, o):
        """A B on the device (csc.py:483-500 -> csc_multiply_ff), nzmax as that kernel returns it."""
        C = CscMat()
        C.m, C.n, C.indptr, C.indices, C.data, C.nzmax = _k.csc_multiply_ff(self.m, self.n, self.indptr, self.indices, self.data,
                                                                            o.m, o.n, o.indptr, o.indices, o.data)
        return C

    def multiply_plan(self, o, transpose_self=False):
        """The plan of A B (transpose_self: A' B) for these two patterns: SpgemmPlan.values / values_dev then refresh the
        values of the product while the patterns stay (the matrix of a Gauss-Newton step, H' (W H))."""
        return _k.SpgemmPlan(self.m, self.n, self.indptr, self.indices, o.m, o.n, o.indptr, o.indices,
                             transpose_a=transpose_self)

    def union_plan(self, others):
        """The UnionPlan of this matrix (member 0) and `others` (members 1, 2, ...), square and of one order: their
        value arrays then go to one batched handle on the union pattern (csparse3_amd.streams.UnionBatch)."""
        mats = [self] + list(others)
        assert all(a.m == self.n and a.n == self.n for a in mats), "square matrices of one order required"
        return _k.UnionPlan(self.n, [(a.indptr, a.indices[:int(a.indptr[a.n])]) for a in mats])

    def to_csr(self):
        """CSR arrays (Bp, Bi, Bx) of this matrix, on the device (csc.py:466-478 -> csc_to_csr)."""
        nnz = int(self.indptr[self.n])
        Bp = np.zeros(self.m + 1, dtype=np.int32)
        Bi = np.empty(nnz, dtype=np.int32)
        Bx = np.empty(nnz, dtype=np.float64)
        _k.csc_to_csr(self.m, self.n, self.indptr, self.indices, self.data, Bp, Bi, Bx)
        return Bp, Bi, Bx

    def t(self):
        """Transpose, on the device (csc.py:502-513 -> csc_transpose)."""
        C = CscMat()
        C.m, C.n, C.indptr, C.indices, C.data = _k.csc_transpose(self.m, self.n, self.indptr, self.indices, self.data)
        C.nzmax = len(C.data)
        return C

    def islands(self):
        """Islands of the (structurally symmetric) pattern, each sorted (csc.py:515-521 -> find_islands)."""
        return _k.find_islands(self.n, self.indptr, self.indices)

    def norm(self):
        """1-norm (csc_norm, csc_numba.py:723-739)."""
        return _k.csc_norm(self.n, self.indptr, self.data)

    # ---- new: factor / solve
    def _pattern_fingerprint(self):
        """(m, n, nnz, digest of indptr / indices): the symbolic analysis is valid for exactly this pattern.
        indptr / indices may be changed in place or reassigned between two lu() calls; comparing the digest
        (a few ms at 500k entries) is what makes "mutate, then refactor" safe."""
        n = self.n
        indptr = np.ascontiguousarray(self.indptr[:n + 1], dtype=np.int32)
        nnz = int(indptr[n]) if n > 0 else 0
        h = hashlib.blake2b(digest_size=16)
        h.update(indptr.tobytes())
        h.update(np.ascontiguousarray(self.indices[:nnz], dtype=np.int32).tobytes())
        return self.m, n, nnz, h.digest()

    def _is_complex(self):
        return bool(np.iscomplexobj(self.data))

    def _analysis(self, kind, order, q, match=False, schur=None, rotate=None):
        cplx = self._is_complex()
        key = (kind, order, None if q is None else bytes(np.asarray(q, dtype=np.int32)), self._pattern_fingerprint(), bool(match),
               None if schur is None else bytes(np.asarray(schur, dtype=np.int32)), "complex128" if cplx else "float64", rotate)
        f = self._factorization
        if f is None or f[0] != key:
            if f is not None:
                f[1].close()
            if cplx:
                assert self.m == self.n, "square matrix required"
                fac = _k.ComplexFactorization(self.n, self.indptr, self.indices, kind=kind, order=order, q=q, rotate=rotate)
            else:
                fac = _k.Factorization(self.m, self.n, self.indptr, self.indices, kind=kind, order=order, q=q,
                                       match_values=self.data if match else None, schur=schur)
            self._factorization = f = (key, fac)
        return f[1]

    def _complex_scope(self, **given):
        """Complex data goes through the real-equivalent plan (csc_hip.ComplexFactorization), which packages LU, Cholesky
        and the N / T / H solves; what it does not package says so."""
        used = [name for name, v in given.items() if v]
        if used:
            raise NotImplementedError("complex matrices: %s is outside the scope of the real-equivalent plan (LU, Cholesky and "
                                      "solves with trans 'N', 'T', 'H'); the real handle is at ComplexFactorization.real"
                                      % ", ".join(used))

    def lu(self, tol=0.0, order=_k.ORDER_AMD, q=None, match=False, perturb=0.0, schur=None, rotate=True):
        """Numeric LU on the device; the symbolic analysis is cached on the object, so calling
        lu() again after changing .data is a refactorisation with the pattern reused.
        match: permute rows by the maximum-product transversal and scale before the analysis (matrices without a strong
        diagonal); the matching is computed from .data at the first analysis and kept across refactorisations.
        perturb: static pivot perturbation -- a pivot below delta becomes +delta instead of failing the factorisation
        (a number: delta itself; True: sqrt(eps), times max |data| when match is false).  The analysis is reused whatever
        perturb is; F.perturbed() counts the replaced pivots and solutions then need F.refine / solve(perturb=...).
        schur: the variables that are not eliminated (Factorization(schur=...)): the interior is factorised and F.schur()
        is the dense Schur complement on that set; order / q then refer to the interior.
        Complex .data: a csc_hip.ComplexFactorization comes back (LU of the real-equivalent form, cached the same way);
        rotate as there; match, perturb and schur raise NotImplementedError.  Real data ignores rotate."""
        if self._is_complex():
            self._complex_scope(match=match, perturb=perturb, schur=schur is not None)
            return self._analysis(_k.CS3_LU, order, q, rotate=bool(rotate)).factor(self.data, tol)
        F = self._analysis(_k.CS3_LU, order, q, match, schur)
        delta = _k.perturbation_delta(perturb, self.data, match)
        if delta != F.perturbation:
            F.set_perturbation(delta)
        F.factor(self.data, tol)
        return F

    def chol(self, order=_k.ORDER_AMD, q=None, schur=None):
        """Numeric Cholesky on the device (complex .data: Hermitian positive definite, through ComplexFactorization)."""
        if self._is_complex():
            self._complex_scope(schur=schur is not None)
            return self._analysis(_k.CS3_CHOLESKY, order, q, rotate=False).factor(self.data)
        F = self._analysis(_k.CS3_CHOLESKY, order, q, schur=schur)
        F.factor(self.data)
        return F

    def schur_complement(self, idx, kind="lu", tol=0.0):
        """S = A22 - A21 A11^-1 A12 on the variables idx (in that order), dense [len(idx), len(idx)]: the interior is
        factorised by LU (kind "lu") or Cholesky ("chol"), the Schur variables are never pivots."""
        assert kind in ("lu", "chol")
        F = self.lu(tol, schur=idx) if kind == "lu" else self.chol(schur=idx)
        return F.schur()

    def solve(self, b, tol=0.0, trans=False, match=False, perturb=0.0, max_refine=10, refine="stationary"):
        """x = A \\ b by LU (factorises if needed); trans: A' x = b on the same factors; match, perturb: as in lu().
        With perturb the solution is refined against A when pivots were replaced (Factorization.solve_refined; not
        offered together with trans); refine="gmres": by GMRES on the held factors instead of the stationary rounds.
        refine="extra": the solve is followed by the extra-precise refinement (Factorization.refine_xp, at most max_refine
        corrections), with or without perturb, with or without trans.
        Complex .data: trans is "N", "T" (A^T, no conjugate; True means this) or "H"; match, perturb and a refine other
        than the default raise NotImplementedError."""
        if self._is_complex():
            self._complex_scope(match=match, perturb=perturb, refine=refine != "stationary")
            return self.lu(tol).solve(b, trans=trans)
        F = self.lu(tol, match=match, perturb=perturb)
        if refine == "extra":
            return F.refine_xp(self.data, b, max_iters=max_refine, trans=trans)[0]
        if F.perturbation == 0.0:
            return F.solve(b, trans=trans)
        assert not trans, "perturb refines A x = b only"
        return F.solve_refined(self.data, b, max_refine, refine)

    def solve_modified(self, b, deltas, tol=0.0, sing_tol=0.0):
        """x_c = (A + dA_c) \\ b for a list of sparse modifications, `deltas` = [(rows, cols, vals), ...] (triplets of dA_c;
        duplicates add), from ONE LU factorisation of A (factorises as solve does).  -> (X [n, len(deltas)], rpiv); a
        case whose modified matrix is singular (rpiv <= sing_tol, or an exactly zero pivot) has a NaN column."""
        self._complex_scope(solve_modified=self._is_complex())
        F = self.lu(tol)
        with F.updates_plan([(d[0], d[1]) for d in deltas]) as plan:
            vals = [np.atleast_1d(np.asarray(d[2], dtype=np.float64)) for d in deltas]
            cx = np.concatenate(vals) if vals else np.zeros(0)
            return F.solve_updates(plan, cx, b, sing_tol)

    def sensitivities(self, B, C=None, tol=0.0, trans=False, side="auto"):
        """Y = C op(A)^-1 B for a sparse B (CscMat, n x k) and a sparse C (CscMat, p x n; None: the identity, Y = the
        solution itself), op(A) = A' with `trans`, from ONE LU factorisation of A (factorises as solve does).  Only the
        dense Y [p, k] comes back; side "auto" solves for the fewer of k and p columns.  C is turned into the CSC form
        of C' (its rows) with csc_transpose, values included."""
        self._complex_scope(sensitivities=self._is_complex())
        assert B.m == self.n and (C is None or C.n == self.n)
        F = self.lu(tol)
        Ct, Ctx = None, None
        if C is not None:
            _, p, Ctp, Cti, Ctx = _k.csc_transpose(C.m, C.n, C.indptr, C.indices, C.data)
            Ct = (p, Ctp, Cti)
        nb = int(B.indptr[B.n])
        with F.sens_plan((B.n, B.indptr, B.indices[:nb]), Ct, side=side, trans=trans) as plan:
            return F.sens_solve(plan, B.data[:nb], Ctx)

    def condest(self, tol=0.0):
        """1-norm condition estimate ||A||_1 * est(||A^-1||_1) from the LU factors (factorises as solve does)."""
        self._complex_scope(condest=self._is_complex())
        cond, _ = self.lu(tol).condest(self.data)
        return float(cond[0])

    def slogdet(self, tol=0.0):
        """(sign, log|det A|) from the LU factors (factorises as solve does)."""
        self._complex_scope(slogdet=self._is_complex())
        sign, logabs = self.lu(tol).slogdet()
        return float(sign[0]), float(logabs[0])

    def selected_inverse(self, kind="lu", tol=0.0, trans=False):
        """The entries of A^-1 on the pattern of A, as a CscMat with A's pattern (with `trans`: of (A^-1)'), by selected
        inversion on the LU (kind "lu") or Cholesky ("chol") factors (factorises as solve does)."""
        self._complex_scope(selected_inverse=self._is_complex())
        assert kind in ("lu", "chol")
        F = self.lu(tol) if kind == "lu" else self.chol()
        nz = int(self.indptr[self.n])
        return CscMat(self.m, self.n, indptr=self.indptr.copy(), indices=self.indices[:nz].copy(), data=F.inverse_entries(trans=trans))

    def inverse_diagonal(self, kind="lu", tol=0.0):
        """diag(A^-1) [n] by selected inversion on the LU or Cholesky factors (factorises as solve does)."""
        self._complex_scope(inverse_diagonal=self._is_complex())
        assert kind in ("lu", "chol")
        F = self.lu(tol) if kind == "lu" else self.chol()
        return F.inverse_diagonal()

    @staticmethod
    def _rows_of(C):
        """A CscMat (p x n) as the CSC form of its transpose, (p, indptr, indices) and the values: its rows."""
        _, p, Ctp, Cti, Ctx = _k.csc_transpose(C.m, C.n, C.indptr, C.indices, C.data)
        return (p, Ctp, Cti), Ctx

    def quad_forms(self, C, B=None, kind="lu", tol=0.0):
        """t_i = c_i' A^-1 b_i for the rows c_i of a sparse C and b_i of a sparse B (CscMat, m x n; None: B = C), by
        selected inversion on the LU (kind "lu") or Cholesky ("chol") factors (factorises as solve does): every pair of
        columns of one row pair must lie on the pattern of the factors.  With an incidence matrix as C: Z_ii + Z_jj - Z_ij
        - Z_ji of every branch.  C and B are turned into their rows with csc_transpose, values included."""
        self._complex_scope(quad_forms=self._is_complex())
        assert kind in ("lu", "chol")
        assert C.n == self.n and (B is None or (B.n == self.n and B.m == C.m))
        F = self.lu(tol) if kind == "lu" else self.chol()
        Ct, Cx = self._rows_of(C)
        Bt, Bx = (None, None) if B is None else self._rows_of(B)
        with F.quad_plan(Ct, Bt) as plan:
            return F.quad_forms(plan, Cx, Bx)

    def normalized_residuals(self, H, w, r, crit_tol=1e-8):
        """The largest-normalised-residual test of a state estimate whose gain matrix G = H' W H this is: H (CscMat, m x n)
        the measurement Jacobian, w [m] the weights, r [m] the residuals.  By selected inversion on the Cholesky factors.
        -> (rn, info) as Factorization.normalized_residuals: rn_i = |r_i| / sqrt(1/w_i - h_i' G^-1 h_i), 0 for a critical
        measurement (1 - w_i h_i' G^-1 h_i <= crit_tol); info holds omega, t, worst, worst_row, J and critical."""
        self._complex_scope(normalized_residuals=self._is_complex())
        assert H.n == self.n
        F = self.chol()
        Ht, Hx = self._rows_of(H)
        with F.quad_plan(Ht) as plan:
            return F.normalized_residuals(plan, Hx, w, r, crit_tol)


def _sub_matrix_cols(Ap, Ai, Ax, cols):
    """Whole columns `cols` of a CSC matrix with their original row indices (csc_sub_matrix_cols, csc_numba.py:505-538):
    a copy of contiguous slices, done on the host where the arrays live."""
    counts = np.asarray([Ap[j + 1] - Ap[j] for j in cols], dtype=np.int64)
    Bp = np.zeros(len(cols) + 1, dtype=np.int32)
    Bp[1:] = np.cumsum(counts)
    if len(cols):
        take = np.concatenate([np.arange(Ap[j], Ap[j + 1]) for j in cols]) if counts.sum() else np.zeros(0, dtype=np.int64)
    else:
        take = np.zeros(0, dtype=np.int64)
    return Bp, np.asarray(Ai)[take].astype(np.int32), np.asarray(Ax)[take].astype(np.float64)


def scipy_to_mat(scipy_mat):
    """Alias SciPy's CSC arrays without copying (csc.py:541-553)."""
    m, n = scipy_mat.shape
    return CscMat(m, n, indptr=scipy_mat.indptr, indices=scipy_mat.indices, data=scipy_mat.data)


def lusol(A, b, order=1, tol=0.0, match=False, perturb=0.0, max_refine=10, refine="stationary"):
    """x = A \\ b (cs_lusol).  match: with the maximum-product matching and scaling in front (CscMat.lu).  perturb: small
    pivots are replaced instead of rejected and the solution is refined, at most max_refine rounds (csc_lusol_f);
    refine="gmres": by GMRES on the held factors; refine="extra": extra-precise refinement (doubled-precision residuals)
    after the solve, with or without perturb.  Complex A.data: through A.lu (the analysis is cached on A); match, perturb
    and a refine other than the default raise NotImplementedError."""
    if np.iscomplexobj(A.data):
        A._complex_scope(match=match, perturb=perturb, refine=refine != "stationary")
        return A.lu(tol, order=order).solve(b)
    return _k.csc_lusol_f(order, A.m, A.n, A.indptr, A.indices, A.data, b, tol, match=match, perturb=perturb,
                          max_refine=max_refine, refine=refine)


def cholsol(A, b, order=1):
    """x = A \\ b for symmetric positive definite A (cs_cholsol); complex A.data: Hermitian positive definite, through A.chol."""
    if np.iscomplexobj(A.data):
        return A.chol(order=order).solve(b)
    return _k.csc_cholsol_f(order, A.m, A.n, A.indptr, A.indices, A.data, b)


def lsolve(L, x):
    """x = L \\ x in place, L a lower-triangular CscMat with the diagonal first in each column."""
    _k.csc_lsolve_f(L.n, L.indptr, L.indices, L.data, x)
    return x


def usolve(U, x):
    """x = U \\ x in place, U an upper-triangular CscMat with the diagonal last in each column."""
    _k.csc_usolve_f(U.n, U.indptr, U.indices, U.data, x)
    return x


def ltsolve(L, x):
    """x = L' \\ x in place, L a lower-triangular CscMat with the diagonal first in each column (cs_ltsolve)."""
    _k.csc_ltsolve_f(L.n, L.indptr, L.indices, L.data, x)
    return x


def utsolve(U, x):
    """x = U' \\ x in place, U an upper-triangular CscMat with the diagonal last in each column (cs_utsolve)."""
    _k.csc_utsolve_f(U.n, U.indptr, U.indices, U.data, x)
    return x


def pack_4_by_4(A11, A12, A21, A22):
    """[[A11, A12], [A21, A22]] assembled on the device (csc.py:588-606: the power-flow Jacobian layout)."""
    m, n, Pi, Pp, Px = _k.csc_stack_4_by_4_ff(A11.m, A11.n, A11.indices, A11.indptr, A11.data,
                                              A12.m, A12.n, A12.indices, A12.indptr, A12.data,
                                              A21.m, A21.n, A21.indices, A21.indptr, A21.data,
                                              A22.m, A22.n, A22.indices, A22.indptr, A22.data)
    return CscMat(m, n, indptr=Pp, indices=Pi, data=Px)
