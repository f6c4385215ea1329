/*
 * csparse3_amd.h -- C ABI of the MI355X (gfx950) sparse direct-solve backend.
 *
 * This is the drop-in boundary for the factor/solve path of SanPen/CSparse3.
 * The reference selects its kernel module by name at import
 * (/root/reference/src/CSparse3/csc.py:29-41, __config__.NATIVE) and calls
 * kernels with loose flat arrays: scalars int64, index arrays int32, values
 * float64, matrices as (m, n, Ap, Ai, Ax)
 * (/root/reference/src/CSparse3/csc_numba.py:183,331,400 signature strings).
 * Every entry point below keeps that convention: plain pointers and sizes,
 * no torch / numpy types.  The reference has no factor/solve kernel at this
 * snapshot, so each function names the CSparse-lineage
 * kernel it stands for and the reference convention it follows, not a line it
 * replaces.  The ctypes binding a maintainer would add is in INTEGRATION.md.
 *
 * Return value: 0 on success, negative cs3_status otherwise;
 * cs3_last_error() gives the message for the calling thread.
 * Pointers named *_dev are device (HBM) addresses, everything else is host.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).
 * A handle may be used by one host thread at a time.
 */
#ifndef CSPARSE3_AMD_H
#define CSPARSE3_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cs3_handle_s *cs3_handle;
typedef struct cs3_updates_s *cs3_updates;     /* a list of sparse modifications of a handle's matrix (below) */

enum cs3_status {
    CS3_OK = 0,
    CS3_ERR_ARG = -1,        /* bad argument / shape (the reference asserts, csc_numba.py:240,322) */
    CS3_ERR_ALLOC = -2,
    CS3_ERR_HIP = -3,        /* HIP runtime error, no device, launch failure */
    CS3_ERR_PIVOT = -4,      /* zero / rejected static pivot; column in cs3_info.fail_col */
    CS3_ERR_NOT_SPD = -5,    /* non-positive Cholesky pivot; column in cs3_info.fail_col */
    CS3_ERR_STATE = -6       /* call out of order (solve before factor ...) */
};

enum cs3_kind { CS3_LU = 0, CS3_CHOLESKY = 1 };
enum cs3_order { CS3_ORDER_NATURAL = 0, CS3_ORDER_AMD = 1, CS3_ORDER_GIVEN = 2 };

typedef struct cs3_info {
    int64_t n, nnz_a;
    int64_t nnz_l, nnz_u;          /* entries of L (incl. diagonal) and U (incl. diagonal) */
    int64_t nsuper, nlevels;       /* supernodes, levels of the supernodal tree */
    int64_t max_front, max_width;  /* largest front order r and supernode width w */
    int64_t factor_bytes;          /* dense panel storage in HBM, bytes per matrix */
    int64_t update_bytes;          /* contribution-block pool in HBM, bytes per matrix */
    int64_t batch;                 /* matrices factorised together (same pattern) */
    int64_t fail_col;              /* first failing pivot column (permuted index), -1 if none */
    double  flops_factor;          /* floating-point operations of the numeric phase */
    double  t_order_s, t_symbolic_s; /* host seconds spent in ordering / symbolic analysis */
} cs3_info;

const char *cs3_last_error(void);
int cs3_version(void);
int cs3_device_count(void);        /* 0 when no GPU is visible */

/* ---- ordering and symbolic kernels (host side of the library) ----------
 * Flat-array functions in the style of csc_numba.py; integer outputs are
 * bit-exact with the oracle.  They need no GPU. */

/* cs_amd lineage.  order 0: natural, 1: amd(A+A').  q[n] out. */
int cs3_amd(int64_t order, int64_t m, int64_t n, const int32_t *Ap,
            const int32_t *Ai, int32_t *q);
/* cs_etree lineage: (Ap, Ai) is the upper triangle of a symmetric pattern. */
int cs3_etree(int64_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent);
/* cs_post lineage. */
int cs3_post(int64_t n, const int32_t *parent, int32_t *post);
/* cs_counts lineage: column counts of the Cholesky factor of that pattern. */
int cs3_counts(int64_t n, const int32_t *Ap, const int32_t *Ai,
               const int32_t *parent, const int32_t *post, int32_t *colcount);

/* ---- analysis: ordering + symbolic + supernodes + schedule --------------
 * cs_sqr / cs_schol lineage.  Pattern only; values come with cs3_factor*.
 * kind: cs3_kind.  order: cs3_order; with CS3_ORDER_GIVEN q_given[n] is the
 * fill-reducing order to use.  For CS3_CHOLESKY (Ap, Ai) may hold the full
 * symmetric pattern or only one triangle.  Rows inside a column need not be
 * sorted (csc_numba.py:334-335); nnz is Ap[n], not the array length
 * (csc.py:138,480).  batch >= 1 matrices share this pattern. */
int cs3_analyze(int64_t kind, int64_t order, int64_t n, const int32_t *Ap,
                const int32_t *Ai, const int32_t *q_given, int64_t batch,
                cs3_handle *out);
int cs3_free(cs3_handle h);
int cs3_get_info(cs3_handle h, cs3_info *info);
/* Ordering results.  Any pointer may be NULL.
 * q_amd[n]:   the fill-reducing order before postordering (what cs_amd returns)
 * parent[n], post[n], colcount[n]: etree / postorder / column counts of
 *             A(q_amd,q_amd) + its transpose, as cs_schol computes them
 * q[n]:       the pivot order actually used = q_amd[post[.]]
 * pinv[n]:    row permutation of the factorisation, pinv[q[k]] = k
 * On a matched handle these are the orderings of B (cs3_get_matching has the row matching in front of them). */
int cs3_get_ordering(cs3_handle h, int32_t *q_amd, int32_t *parent, int32_t *post,
                     int32_t *colcount, int32_t *q, int32_t *pinv);
/* Supernode partition: sn_ptr[nsuper+1] first pivot column of each supernode,
 * sn_parent[nsuper], sn_level[nsuper]. */
int cs3_get_supernodes(cs3_handle h, int32_t *sn_ptr, int32_t *sn_parent, int32_t *sn_level);

/* ---- matching + scaling: LU for matrices without a strong diagonal ------
 * Every pivot of cs3_factor is a diagonal entry, only checked against tol.  A row-permuted identity, a saddle-point
 * system [[H, G'], [G, 0]] or a badly scaled Jacobian fails that check.  The step that makes static pivots safe there
 * (Duff & Koster, MC64 job 5; the weighted relative of cs_maxtrans; what SuperLU_DIST, PARDISO and cuDSS do): before the
 * analysis, permute the rows by a maximum-product transversal and scale rows and columns so that the diagonal is 1 and
 * everything else at most 1 in magnitude.
 *
 * For A (n x n, CSC, nnz = Ap[n]) a matching is rowperm[n], dr[n] > 0, dc[n] > 0:
 *   rowperm[j] is the row of A matched to column j; it becomes row j of B.  rowinv is its inverse.
 *   B[rowinv[i], j] = (dr[i] * A[i, j]) * dc[j], in exactly this product order (two roundings), so a host can rebuild B bit
 *     for bit.  Column j of B holds the entries of column j of A in the same storage order: Ax keeps its entry order, only
 *     the row indices change.
 *   |B| <= 1 everywhere and |B[j, j]| = 1, up to the rounding of exp / log (a few 1e-15).
 *   Among all transversals sum_j log |A[rowperm[j], j]| is maximal.
 * An entry whose value is exactly 0 counts as absent (entries stored twice count as two entries).  Costs
 * c_ij = log max_i |a_ij| - log |a_ij|, shortest augmenting paths with duals u_i + v_j <= c_ij, dr_i = exp(u_i),
 * dc_j = exp(v_j) / max_i |a_ij|; ties go to the lowest index, so the result is bitwise the same on every run.  Host
 * code, sequential.
 *
 * cs3_match_scale: the matching alone; needs no GPU (like cs3_amd).  Rows inside a column need not be sorted.
 * cs3_analyze_matched: cs3_analyze for CS3_LU with the matching computed from Ax[nnz] -- ONE representative matrix, also
 *   when batch > 1; the matching is then fixed for the life of the handle (refactorisations keep it).  The handle
 *   analyses the pattern of B, (Ap, rowinv[Ai]); order / q_given apply to B.
 * cs3_get_matching: any pointer may be NULL; t_match_s = host seconds the matching took (next to cs3_info.t_order_s).
 *   A handle made by cs3_analyze gives CS3_ERR_STATE.
 * Checks of the first two, in this order: null pointers or a bad pattern (Ap[0] != 0, Ap not monotone, a row index
 * outside [0, n)): CS3_ERR_ARG; a non-finite value in Ax: CS3_ERR_ARG; no full transversal (structurally singular, stored
 * zeros absent): CS3_ERR_PIVOT, and the message says how many columns could be matched.
 *
 * On a MATCHED handle every entry point keeps speaking in terms of A where it takes or returns values, right-hand sides
 * and solutions -- Ax in A's entry order, b and x in A's rows and columns -- and in terms of B where it exposes the
 * factorisation itself:
 *   cs3_factor, cs3_factor_dev, cs3_factor_solve_dev, cs3_factor_solve_bx_dev: factorise B; the values are scaled on the device into the
 *     library's own copy (one more launch, no further pass over the values).  tol and fail_col refer to B in its pivot order.
 *   cs3_solve(_dev): A x = b as x = Dc B^-1 (Dr P b).  cs3_solve_t(_dev): A' x = b as z = B^-T (Dc b),
 *     x[i] = dr[i] z[rowinv[i]].  The scalings ride in the two row permutations of the solve.
 *   cs3_residual / matvec / refine(_t)_dev, cs3_condest(_dev), cs3_slogdet(_dev), cs3_updates_*: of A (||A||_1 from the
 *     caller's Ax; sign = sign(det B) * parity(rowperm), log|det A| = log|det B| - sum log dr - sum log dc).
 *   cs3_lsolve / usolve / ltsolve / utsolve, cs3_get_factors, cs3_get_ordering, cs3_get_info: the factors and orderings of B.
 *   cs3_export_factor_dev / cs3_import_factor_dev: CS3_ERR_ARG (not available on matched handles).
 * A handle made by cs3_analyze behaves as before, bit for bit and launch for launch. */
int cs3_match_scale(int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                    int32_t *rowperm, double *dr, double *dc);
int cs3_analyze_matched(int64_t order, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                        const int32_t *q_given, int64_t batch, cs3_handle *out);
int cs3_get_matching(cs3_handle h, int32_t *rowperm, double *dr, double *dc, double *t_match_s);

/* ---- numeric factorisation (cs_lu / cs_chol lineage) --------------------
 * P A Q = L U with P = Q' (static diagonal pivots in AMD order), L unit lower,
 * U upper; or P A P' = L L'.  Ax[batch][nnz_a] in the entry order of the
 * analysed (Ap, Ai).  tol as in cs_lu: a diagonal pivot is accepted when
 * |pivot| >= tol * max|column below|; rejected pivots give CS3_ERR_PIVOT
 * (there is no CPU fallback).  tol <= 0 disables the test.  On a matched handle (cs3_analyze_matched) Ax are still the
 * values of A; B is factorised and tol refers to B. */
int cs3_factor(cs3_handle h, const double *Ax, double tol);
int cs3_factor_dev(cs3_handle h, const double *Ax_dev, double tol, void *stream);
/* cs_lusol / cs_cholsol as one call on resident data: numeric (re)factorisation of Ax AND the full
 * solve of X [batch][n, k] in place.  Same results as cs3_factor_dev followed by cs3_solve_dev, bit
 * for bit; the forward sweep of a tree level runs beside the factorisation of the next level, so
 * the call is shorter than the two in sequence.  Status via cs3_factor_status. */
int cs3_factor_solve_dev(cs3_handle h, const double *Ax_dev, double tol, double *X_dev, int64_t k, void *stream);
/* The same, out of place: right-hand sides read from B_dev, solutions written to X_dev (x = A^-1 b without
 * the copy of b that the in-place form needs when b is kept). */
int cs3_factor_solve_bx_dev(cs3_handle h, const double *Ax_dev, double tol, const double *B_dev, double *X_dev, int64_t k, void *stream);
/* Deferred status of the last cs3_factor_dev / cs3_factor_solve_dev (synchronises the stream). */
int cs3_factor_status(cs3_handle h, void *stream);

/* ---- static pivot perturbation: LU that never stops on a tiny pivot ------
 * Matching + scaling makes the diagonal of B equal to 1 BEFORE elimination; it says nothing about what elimination
 * leaves there.  A Newton chain on a KKT system or an ill-scaled Jacobian meets a cancelling pivot sooner or later, and
 * a static-pivot LU then either stops (CS3_ERR_PIVOT) or, with tol <= 0, returns 1e16 of growth.  The other half of what
 * SuperLU_DIST, PARDISO and cuDSS do next to the matching: a pivot that is too small is REPLACED, and iterative
 * refinement (cs3_refine_dev, cs3_refine) removes the error.
 *
 * The rule, for delta > 0: during the numeric LU of every matrix of the batch a pivot p with |p| < delta is replaced
 * by +delta -- always plus delta, whatever the sign of p (a pivot that is rounding noise has no sign worth keeping, and
 * one rule for both signs keeps every wave that derives the pivot in agreement).  NaN and +-inf are not smaller than
 * delta: they stay as they are and are rejected as before.  The tol test is unchanged and sees the replaced pivot; with
 * tol <= 0 and finite values an LU with delta > 0 cannot fail.
 *
 * The factors are then the exact factors (to rounding) of A(q, q) + diag(E), with E_kk != 0 only at the replaced
 * pivots, E_kk = delta - p_k.  Everything that reads the factors sees delta as U_kk: the solves, cs3_get_factors, the
 * export, cs3_slogdet and cs3_condest -- the last two describe the PERTURBED matrix.  A solution is x = (A + E')^-1 b and
 * needs refinement against A: cs3_refine_dev / cs3_refine, whose corrections shrink by about |E| |A^-1| per round.
 *
 * cs3_set_pivot_perturbation: delta for this handle, kept across refactorisations; 0 (the default) switches it off, and
 *   the handle then runs the kernels it ran before, instruction for instruction.  Null handle, delta < 0 or not finite,
 *   or a Cholesky handle: CS3_ERR_ARG.  On a matched handle delta refers to B, where |B| <= 1: sqrt(DBL_EPSILON) is the
 *   usual choice; on a plain handle sqrt(DBL_EPSILON) * max|Ax|.  A changed delta takes effect with the next
 *   factorisation (captured graphs of the old value are dropped then).
 * cs3_get_perturbed: count[batch], the number of pivots the last factorisation replaced in every matrix (synchronises
 *   the stream, like cs3_factor_status).  CS3_ERR_STATE before any factorisation.  A perturbation is not a failure:
 *   cs3_factor_status stays CS3_OK.
 * Not offered: Cholesky, a relative delta read from device memory, a list of the perturbed columns. */
int cs3_set_pivot_perturbation(cs3_handle h, double delta);
int cs3_get_perturbed(cs3_handle h, int64_t *count, void *stream);

/* ---- solves (cs_lsolve / cs_usolve / cs_ltsolve / cs_lusol / cs_cholsol) -
 * X is [n, k] row-major (the reference's multi-vector layout, csc.py:409-414),
 * overwritten in place.  With batch > 1, X is [batch, n, k].
 * cs3_solve:   full solve A x = b including both permutations
 * cs3_lsolve:  x = L \ x     in the permuted (pivot-order) space
 * cs3_usolve:  x = U \ x     (for Cholesky: x = L' \ x)
 * On a matched handle cs3_solve solves with A (scalings and row matching included); cs3_lsolve / cs3_usolve apply the
 * factors of B. */
int cs3_solve(cs3_handle h, double *X, int64_t k);
int cs3_lsolve(cs3_handle h, double *X, int64_t k);
int cs3_usolve(cs3_handle h, double *X, int64_t k);
int cs3_solve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_lsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_usolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
/* Transposed solves on the same factors (cs_ltsolve / cs_utsolve lineage), same layouts and error codes:
 * cs3_solve_t:  full solve A' x = b, both permutations included (x = P' (L' \ (U' \ (Q' b))))
 * cs3_utsolve:  x = U' \ x   in pivot order (Cholesky handles: CS3_ERR_ARG, there is no U)
 * cs3_ltsolve:  x = L' \ x   in pivot order, unit diagonal for LU (Cholesky: what cs3_usolve does)
 * On a Cholesky handle A' = A: cs3_solve_t is cs3_solve, bit for bit.  On a matched handle cs3_solve_t solves with A',
 * cs3_utsolve / cs3_ltsolve apply the factors of B. */
int cs3_solve_t(cs3_handle h, double *X, int64_t k);
int cs3_utsolve(cs3_handle h, double *X, int64_t k);
int cs3_ltsolve(cs3_handle h, double *X, int64_t k);
int cs3_solve_t_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_utsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_ltsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);

/* ---- residual and iterative refinement on resident data ----
 * R = B - A X with the handle's analysed pattern and the values Ax_dev [batch][nnz]; X, B, R [batch][n, k] row-major.
 * Every row of A X is summed as csc_mat_vec_ff sums it (csc_numba.py:309-328: ascending column, product rounded before
 * the add), so results are reproducible and A X equals the reference's matvec bit for bit.  On a matched handle these
 * are products with A itself (the pattern the caller passed), and refinement solves with A. */
int cs3_residual_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, double *R_dev,
                     int64_t k, void *stream);
/* Y = A X alone, same summation (the device-resident csc_mat_vec_ff; cs3_csc_matvec is the host-pointer form). */
int cs3_matvec_dev(cs3_handle h, const double *Ax_dev, const double *X_dev, double *Y_dev, int64_t k, void *stream);
/* `steps` rounds of  x += A \ (b - A x)  with the factors the handle holds (e.g. factors of an earlier Newton iterate
 * refining the solution for the current values Ax_dev).  last_correction (optional): max |dx| of the last round
 * (reading it synchronises the stream). */
int cs3_refine_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t steps,
                   double *last_correction, void *stream);
/* The host-array form of cs3_refine_dev (Ax [batch][nnz], B and X [batch][n, k] in host memory, the null stream): the
 * same kernels in the same order, so the same bits. */
int cs3_refine(cs3_handle h, const double *Ax, const double *B, double *X, int64_t k, int64_t steps, double *last_correction);
/* The transposed counterparts: R = B - A' X, Y = A' X, and x += A^-T (b - A' x).  Row j of A' X sums column j of A in
 * storage order with the same rounding discipline (bit-exact with csc_mat_vec_ff applied to A' when the columns of A are
 * sorted). */
int cs3_residual_t_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, double *R_dev,
                       int64_t k, void *stream);
int cs3_matvec_t_dev(cs3_handle h, const double *Ax_dev, const double *X_dev, double *Y_dev, int64_t k, void *stream);
int cs3_refine_t_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t steps,
                     double *last_correction, void *stream);

/* ---- GMRES refinement on the held factors --------------------------------
 * cs3_refine_dev is the stationary iteration x += M^-1 (b - A x), M = the held factors: it converges only while the
 * spectral radius of I - M^-1 A is below 1, and diverges beyond -- factors of an earlier Newton iterate against values
 * that moved far, or a pivot perturbation (cs3_set_pivot_perturbation) with a large delta.  The Krylov half of what
 * SuperLU_DIST, PARDISO and cuDSS pair with static pivoting: restarted GMRES(restart), right-preconditioned with the held
 * factors.  When A M^-1 - I has rank r it ends in r iterations, whatever the size of the change.
 *
 * Systems: column t of matrix b of the batch is one system, batch * k independent systems advancing in lock-step; one
 * solve and one product per iteration serve them all.  X, B [batch][n, k] row-major; X holds x0 on entry and the
 * solution on exit.  iters, relres: HOST arrays [batch * k], either may be NULL: the Krylov iterations the system used,
 * and its true final ||b - A x||_2 / ||b||_2.
 *
 * Per cycle: r = b - A x, v0 = r / ||r||, then w = A M^-1 v_j orthogonalised by classical Gram-Schmidt applied twice,
 * Givens rotations per system, and at the end x += M^-1 (V y) -- one more solve.  trans != 0: A' and the transposed
 * solve.  A system whose recurrence residual is <= rtol ||b||, or with a lucky breakdown (h_{j+1,j} == 0), or that has
 * used max_iters iterations, is FROZEN: its next basis vectors are zero and it contributes nothing further.  A cycle
 * ends when no system is active or after `restart` iterations.  Convergence is decided on the TRUE residual at the end
 * of the cycle; a system still above rtol enters the next one.  The call ends when every system has converged or used
 * max_iters iterations.  Not converging is not an error: CS3_OK, and relres tells.
 *   ||b||_2 == 0: x = 0, iters = 0, relres = 0.  An x0 that already satisfies rtol: iters = 0, X untouched bit for bit.
 *   A non-finite norm or Hessenberg entry freezes that system alone: relres = NaN, its column of X as the last completed
 *   cycle left it; the other systems are unaffected.
 * The reductions run in a fixed order without float atomics: the same bits on every run.
 *
 * HOST INVOLVEMENT: the call is host-driven.  After every iteration (and at the start of every cycle) it reads one
 * 4-byte "systems still active" word, which synchronises `stream`, and it reads the two result arrays at the end.  It
 * cannot be captured into a graph.
 *
 * Checks, in this order: null handle, a Schur handle, null Ax / B / X, k < 1, restart outside 1 .. max_restart,
 * max_iters < 0, rtol negative or not finite: CS3_ERR_ARG; no factorisation: CS3_ERR_STATE (none of these needs a
 * device).  LU and Cholesky handles; products over the stored entries as in cs3_residual_dev.  On a matched handle
 * products and solves are with A, as in refinement.  Work memory ((restart + 1) basis vectors and two work vectors
 * [batch][n, k], per system the Hessenberg factor, rotations, g and y, the partial sums) belongs to the handle, grows on
 * demand with k and `restart`, and goes with cs3_free.
 * cs3_gmres_limits: max_restart (32), the rows per chunk of the fixed-order reductions, the right-hand sides per tile of
 *   the kernels; needs no device.
 * cs3_gmres: the host-array form (the null stream): the same kernels in the same order, the same bits.
 * Not offered: a capture-safe fixed-length form, block or deflated variants, CG for Cholesky handles, left
 * preconditioning. */
typedef struct { int64_t max_restart, chunk_rows, rhs_tile; } cs3_gmres_limits_t;
int cs3_gmres_limits(cs3_gmres_limits_t *out);
int cs3_gmres_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k,
                  int64_t restart, int64_t max_iters, double rtol, int64_t trans,
                  int32_t *iters, double *relres, void *stream);
int cs3_gmres(cs3_handle h, const double *Ax, const double *B, double *X, int64_t k,
              int64_t restart, int64_t max_iters, double rtol, int64_t trans, int32_t *iters, double *relres);
/* diagnostics: est [count] = the residual estimate of the recurrence, |g_{j+1}| / ||b||, that every system of the last
 * cs3_gmres* call on this handle ended its last cycle with (count = batch * k of that call; synchronises the device) */
int cs3_debug_gmres_estimates(cs3_handle h, double *est, int64_t count);
/* diagnostics: one vector kernel of iteration j alone on the work memory of the last cs3_gmres* call on this handle
 * (which = 0: the multi-dot, 1: the first update, 2: the second update with the norm), for timing */
int cs3_debug_gmres_kernel(cs3_handle h, int64_t which, int64_t j, void *stream);
/* diagnostics: V [nvec][batch][n, k] = the first nvec <= restart + 1 basis vectors as the last cs3_gmres* call on this
 * handle left them (read-only; synchronises the device).  Vector 0 is what the call's closing residual check left (zeros
 * once every system has finished), vectors 1 .. are the last iterating cycle's, exact zeros behind a system's last
 * column.  CS3_ERR_STATE before any cs3_gmres* call, CS3_ERR_ARG on a null V or a count outside 0 .. restart + 1. */
int cs3_debug_gmres_basis(cs3_handle h, double *V, int64_t nvec);

/* ---- extra-precise refinement: doubled-precision residuals, berr and ferr ----
 * Neither refinement above can make a solution more accurate than cond(A) * eps: the residual b - A x is summed in
 * working precision, and once the true residual is below that sum's rounding error the correction A \ r is noise.  This
 * is the extra-precise refinement of LAPACK's xGERFSX (Demmel, Hida, Kahan, Li, Mukherjee, Riedy 2006): only the
 * residual is accumulated in doubled precision and x is carried as a head and a tail; the solves are the handle's own.
 * For cond(A) below 1 / eps it reaches the correctly rounded solution; the componentwise backward error berr and a
 * normwise forward error bound ferr are by-products.
 *
 * Layouts are cs3_refine_dev's: X, XT, B, R, S [batch][n, k] row-major, Ax [batch][nnz]; column t of matrix b is one
 * system, index b * k + t in the result arrays.
 *
 * cs3_residual_xp_dev: R = B - op(A) (X + XT) accumulated in doubled precision and rounded once, S = |B| + |op(A)| |X|
 * (S_dev may be NULL; XT_dev may be NULL = no tail).  trans != 0: op(A) = A'.  Row i, system t, the entries (a, j) of the
 * row in cs3_residual_dev's order (ascending column through the row view; trans: storage order of column i), no
 * floating-point contraction:
 *     (sh, sl) = (b_i, 0);  den = |b_i|
 *     per entry:  ph = fl(a * x_j);  pl = fma(a, x_j, -ph)               the exact error of the product
 *                 (sh, e) = TwoSum(sh, -ph)                              Knuth's, six operations
 *                 sl = fl(sl + fl(fl(e - pl) - fl(a * xt_j)))            without a tail: sl = fl(sl + fl(e - pl))
 *                 den = fl(den + fl(|a| * |x_j|))
 *     r_i = fl(sh + sl);  s_i = den
 * One thread per (row, right-hand side), a grid-stride loop under grid_cap workgroups of `block` threads, no atomics,
 * every output written: the same bits on every run.  Needs the analysis only (no factorisation).
 *
 * cs3_refine_xp_dev: X holds x0 on entry (typically from cs3_solve_dev), the tail xt starts at 0.  All batch * k systems
 * advance in lock-step; pass s = 0 .. max_iters - 1, while any system is active:
 *   1. r = b - op(A) (x + xt) as above, dx = op(A)^-1 r by the handle's solve (matched and perturbed handles as in
 *      cs3_refine_dev).
 *   2. nd = max_i |dx_i|, nx = max_i |x_i| (x before the update): maxima only, exact and independent of order.
 *   3. Per system: nd or nx not finite: stop, flag 3, dx not applied.  With an earlier applied correction nd_prev:
 *      rate = max(rate, nd / nd_prev), and nd > stall_ratio * nd_prev: stop, flag 2, dx not applied.  Otherwise dx is
 *      applied, iters += 1, nd_prev = nd, and nd <= eps * nx (0 <= 0 included): stop, flag 1 (converged).
 *   4. For the systems that apply: (s, e) = TwoSum(x, dx); t = fl(xt + e); (x, xt) = TwoSum(s, t).  The columns of a
 *      stopped system are not touched again, bit for bit.
 *   5. The host reads one 4-byte word, the systems still active: this synchronises `stream` (as cs3_gmres_dev does; the
 *      call cannot be captured into a graph).
 * Systems still active after the last pass have flag 0.  A closing pass evaluates the residual of the returned x alone
 * (the tail dropped): berr = max_i |r_i| / s_i (0 / 0 counts as 0, non-zero over zero is +inf), nxf = max_i |x_i|.
 * ferr, first match wins: NaN for flag 3; +inf when iters == 0; +inf when rate >= 1; 0 when nd_prev == 0 and nxf == 0
 * (the zero solution of a zero right-hand side); otherwise max(eps, (nd_prev / nxf) / (1 - rate)), xGERFSX's
 * geometric-series bound on the normwise relative error in the infinity norm, with eps as its floor.
 * max_iters == 0 is valid: X untouched, iters = 0, flag = 0, ferr = +inf, berr that of x0.
 * XT_dev, when not NULL, receives the tail: x + xt is the solution in doubled precision.
 * iters, flag (int32), ferr, berr, rate (double): HOST arrays [batch * k], any may be NULL.
 *
 * Checks, in this order: null handle, a Schur handle, null Ax / B / X (cs3_residual_xp_dev: R too), k < 1,
 * max_iters < 0: CS3_ERR_ARG; no factorisation (cs3_refine_xp* only): CS3_ERR_STATE; none needs a device.  LU and
 * Cholesky handles, batches, matched and perturbed handles.  Work memory (the tail [batch][n, k]; per system the two
 * maxima, nd_prev, rate, iters, flag, the apply mask) belongs to the handle, grows with k and goes with cs3_free; a
 * second call with the same k allocates nothing.
 * cs3_refine_xp_limits: the launch shape of the residual kernel, the default max_iters (10), eps = 2^-52,
 *   stall_ratio = 0.5, maxima_grid_cap = the workgroups over the rows of the maxima kernel; needs no device.
 * cs3_refine_xp, cs3_residual_xp: the host-array forms (the null stream): the same kernels, the same bits.
 * Not offered: a capture-safe form of fixed length, a componentwise forward bound, Schur handles, residuals in more
 * than doubled precision. */
typedef struct { int64_t block, grid_cap, max_iters_default; double eps, stall_ratio; int64_t maxima_grid_cap; } cs3_refine_xp_limits_t;
int cs3_refine_xp_limits(cs3_refine_xp_limits_t *out);
int cs3_residual_xp_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, const double *XT_dev,
                        double *R_dev, double *S_dev, int64_t k, int64_t trans, void *stream);
int cs3_residual_xp(cs3_handle h, const double *Ax, const double *B, const double *X, const double *XT, double *R, double *S,
                    int64_t k, int64_t trans);
int cs3_refine_xp_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, double *XT_dev,
                      int64_t k, int64_t max_iters, int64_t trans,
                      int32_t *iters, int32_t *flag, double *ferr, double *berr, double *rate, void *stream);
int cs3_refine_xp(cs3_handle h, const double *Ax, const double *B, double *X, double *XT, int64_t k, int64_t max_iters,
                  int64_t trans, int32_t *iters, int32_t *flag, double *ferr, double *berr, double *rate);

/* ---- condition estimates and log-determinants from the held factors -----
 * Static diagonal pivots say nothing about how far a solution can be trusted; these are the cheap reliability signal
 * next to the factors (klu_condest, LAPACK xGECON, MATLAB condest).  Results are per matrix of the batch, [batch] each.
 * After a cs3_factor_dev / cs3_factor_solve_dev whose status has not been polled (cs3_factor_status) they carry the same
 * caveat as a solve: they are only meaningful if that factorisation succeeded.
 * Checks, in this order: a null Ax / cond (sign, logabs) gives CS3_ERR_ARG; no successful factorisation CS3_ERR_STATE.
 *
 * cs3_condest_dev: inv_norm[b] = LAPACK dlacn2's estimate of ||A_b^-1||_1 (ITMAX 5, every A^-1 a full solve, every A^-T a
 *   transposed solve on the same factors; Cholesky: both the plain solve), cond[b] = ||A_b||_1 * inv_norm[b] with
 *   ||A_b||_1 from Ax_dev [batch][nnz_a] (the analysed entry order, as for cs3_residual_dev) summed exactly as
 *   cs3_csc_norm sums it: the STORED entries, so on a Cholesky handle analysed from one triangle cond is ||tril(A)||_1 *
 *   inv_norm, not kappa_1 of the symmetric matrix (inv_norm is unaffected).  inv_norm may be NULL.  A non-finite value in a solution gives +inf.  Asynchronous on `stream`:
 *   a fixed sequence of 11 solves (A^-1, A^-T alternating), no synchronisation after the first call's allocations.
 * cs3_condest: the same from host arrays; synchronises after every solve (one 8-byte read) and runs only the solves some
 *   matrix still needs (4 or 5 for most matrices).  Both forms give the same bits.
 * cs3_slogdet_dev: sign[b] and logabs[b] = log|det A_b| from the pivots (LU: det A = prod u_jj since P = Q'; Cholesky:
 *   sign +1, 2 sum log l_jj).  Pivots that only imported factors can hold follow numpy.linalg.slogdet: a zero pivot
 *   gives (0, -inf); an infinite one log|det| = +inf; a NaN one log|det| = NaN with the sign of the other pivots.
 *   Asynchronous.
 * cs3_slogdet: the same into host arrays (synchronises).
 * On a matched handle all four are of A: kappa_1(A) through the matched solves, det A from det B, the parity of rowperm
 * and the scalings. */
int cs3_condest_dev(cs3_handle h, const double *Ax_dev, double *cond_dev, double *inv_norm_dev, void *stream);
int cs3_condest(cs3_handle h, const double *Ax, double *cond, double *inv_norm);
int cs3_slogdet_dev(cs3_handle h, double *sign_dev, double *logabs_dev, void *stream);
int cs3_slogdet(cs3_handle h, double *sign, double *logabs);

/* ---- many low-rank-modified systems (A + dA_c) x = b on the held factors -
 * Contingency screening ("compensation" in the power-systems literature): the factors of A are held, case c changes a
 * handful of entries, and x_c is wanted for a thousand cases.  Nothing is refactorised (so a modified matrix that would
 * fail the static pivot test is no obstacle): Sherman-Morrison-Woodbury on the base factors, one small dense system
 * per case, all on the device.
 *
 * Case c is a sparse matrix dA_c given as triplets (i, j, v); duplicates of one (i, j) inside a case ADD.  With R_c its
 * distinct rows (r of them, ascending), C_c its distinct columns (s, ascending), D_c the dense r x s block,
 * x0 = A^-1 b and Z = A^-1 E_R (the columns of A^-1 of the touched rows):
 *     G_c = Z[C_c, R_c]   S_c = I_r + D_c G_c   y_c = S_c^-1 (D_c x0[C_c])   x_c = x0 - Z[:, R_c] y_c
 * S_c is eliminated with partial pivoting (largest |.|, ties to the lowest row).  A case without entries gives x0, bit for
 * bit what cs3_solve_dev gives for b.  S_c singular means A + dA_c is singular (an outage that islands the network):
 * an answer, not an error.  rpiv[c] = min_k |pivot_k| / max(1, max |S_c|) (1.0 for an empty case): the smallest pivot on
 * the scale of the identity that S_c perturbs -- normalising by max |S_c| alone would give 1.0 for EVERY case of rank 1,
 * singular or not.  A case with rpiv[c] <= sing_tol has its column of X filled with NaN (sing_tol <= 0 disables the test;
 * an exactly zero pivot always counts); the other cases of the call are unaffected.  A case with a NaN among its values
 * has rpiv[c] = NaN and a NaN column whatever sing_tol is, and the other cases are unaffected too (infinite values:
 * undefined).
 *
 * Two phases, as analysis and factorisation are: the case list of a screening run is fixed while values change.
 * cs3_updates_plan: host, pattern only, needs no GPU.  cp[ncases + 1] (cp[0] = 0), ci / cj[cp[ncases]] rows and columns
 *   of the triplets of each case.  Checks, in this order: null pointers, ncases < 1, cp not monotone, an index outside
 *   [0, n), a case with more than 16 distinct rows or more than 16 distinct columns (the message names the case), a
 *   handle with batch > 1 (not supported): CS3_ERR_ARG.
 *   Cases are grouped, in their order, into TILES whose union of touched rows is at most 1024 columns of A^-1 (and at
 *   most 1024 cases); a tile is one many-right-hand-side solve, and a row that cases of two tiles touch is solved for in
 *   both.  CS3_UPD_TILE in the environment, read by this call, lowers the width (for tests that must cross tile
 *   boundaries; a case always fits a tile of its own).
 * cs3_updates_info: number of cases, distinct touched rows over all cases, largest r or s, number of tiles.  Any pointer
 *   may be NULL.
 * cs3_updates_solve_dev: cx_dev[cp[ncases]] the values in the plan's triplet order; b_dev[n]; X_dev [n, ncases] row-major
 *   (the library's multi-vector layout: case c is column c); rpiv_dev[ncases] may be NULL.  Asynchronous on `stream`.
 *   Checks, in this order: null arguments, a plan made for another handle: CS3_ERR_ARG; no successful factorisation:
 *   CS3_ERR_STATE.  LU and Cholesky handles both work, and dA_c need not be symmetric on a Cholesky handle.
 *   Workspace: n x 1024 doubles (less when every tile is narrower) + n doubles on the handle, a few hundred bytes per case
 *   on the plan, allocated by the first call; later calls neither allocate nor synchronise.
 * cs3_updates_solve: the same from host arrays (synchronises); the same bits.
 * A plan survives refactorisations of its handle.  Plans and handle may be freed in either order: freeing the handle
 * releases the device memory of its plans, which can then only be freed (a solve with one is CS3_ERR_ARG).
 *
 * On a matched handle the plan's indices and the solutions are in A's rows and columns, as everywhere.
 *
 * Out of scope: batched handles; transposed systems; several base right-hand sides per call; more than 16 distinct rows
 * or columns per case; exploiting the sparsity of the unit right-hand sides inside the sweeps; solving with A^-T E_C
 * instead of A^-1 E_R when a list has fewer distinct columns than rows. */
int cs3_updates_plan(cs3_handle h, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj,
                     cs3_updates *out);
int cs3_updates_free(cs3_updates u);
int cs3_updates_info(cs3_updates u, int64_t *ncases, int64_t *nrows_unique, int64_t *max_rank, int64_t *ntiles);
int cs3_updates_solve_dev(cs3_handle h, cs3_updates u, const double *cx_dev, const double *b_dev,
                          double sing_tol, double *X_dev, double *rpiv_dev, void *stream);
int cs3_updates_solve(cs3_handle h, cs3_updates u, const double *cx, const double *b,
                      double sing_tol, double *X, double *rpiv);

/* ---- sparse right-hand sides: Y = C op(A)^-1 B on the held factors -------
 * PTDF and LODF tables, rows and columns of Z-bus, sensitivities of a few monitored quantities to many injections,
 * selected entries of A^-1: B (n x k) is sparse with a few entries per column, C (p x n) is sparse with a few entries per
 * row, and only the small dense Y [p, k] is wanted.  Nothing dense crosses PCIe: the right-hand sides are written on the
 * device, tile by tile, go through the handle's many-right-hand-side solves, and are combined with the other operand
 * there.  op(A) is A, or A' with `trans` (a Cholesky handle: trans changes nothing).
 *
 * B is given by columns: Bp[k + 1], Bi, values Bx.  C is given by ROWS, as the CSC arrays of C': Ctp[p + 1], Cti, Ctx
 * (column r of C' = row r of C).  Y is [p, k] row-major.  Rows inside a column may be unsorted; duplicates of one index
 * inside a column ADD, in storage order; an empty column of B gives a zero column of Y, an empty row of C a zero row.
 * Bp == NULL: B = I (k must be n).  Ctp == NULL: C = I (p must be n).  Both NULL (the dense inverse) is refused.
 *
 * side 1 ("right"): solves op(A) T = B for tiles of columns of B, then Y[:, tile] = C T.
 * side 2 ("left"): solves op(A)' T = C' for tiles of rows of C, then Y[tile, :] = (B' T)'.
 * side 0: the side with fewer columns to solve for, k against p; a tie goes right.  An identity operand forces the other
 *   side (B = I: left, C = I: right).  With p = 100 monitored rows and k = 50 000 injections, left is 100 transposed
 *   solves instead of 50 000 plain ones.
 *
 * cs3_sens_plan: host, pattern only, needs no GPU; copies the patterns.  Checks, in this order: a null handle or out
 *   pointer; k < 1 or p < 1; both operands the identity; an identity operand with k (p) != n; pointer arrays not monotone
 *   from 0 (or null index arrays behind them); an index outside [0, n); side not 0, 1 or 2; a side that an identity
 *   operand rules out; a handle with batch > 1; a Schur handle: CS3_ERR_ARG, and the message names what failed.
 *   The solved-for columns are grouped, in order, into TILES of at most 1024; every tile but the last is solved at the
 *   full width, the last at its own (padded with zero columns to 16 when it is narrower than that): at most two solve
 *   widths per plan, on one tile buffer, so a plan keeps two captured graphs per handle and never evicts a caller's.
 *   CS3_SENS_TILE in the environment, read by this call, lowers the tile width (for tests that must cross tile boundaries
 *   at small sizes); below 16 nothing is padded and the tiles run on the few-right-hand-side sweeps.
 * cs3_sens_info: k, p, the side chosen (1 or 2), trans, the number of tiles, the widest solve width, nnz(B), nnz(C) (n for
 *   an identity operand).
 * cs3_sens_limits: the constants that shape tiles and launches; needs no device.
 * cs3_sens_solve_dev: Bx_dev / Ctx_dev the values in the plan's entry order (the value pointer of an identity operand is
 *   ignored), Y_dev [p, k].  Asynchronous on `stream`.  Checks, in this order: null arguments, a plan made for another
 *   handle: CS3_ERR_ARG; no successful factorisation: CS3_ERR_STATE.
 *   Workspace: one tile buffer of n x (widest width) doubles on the handle and the plan's tables, allocated by the first
 *   call; later calls neither allocate nor synchronise.
 * cs3_sens_solve: the same from host arrays (synchronises); the same bits.  Its device copies of the values and of Y
 *   stay on the plan.
 * Every sum runs in storage order, product rounded before the add, without atomics: the same bits on every run; a unit
 * value hands the solution's bits over unchanged.  A NaN value in B reaches exactly its column of Y, one in C its row.
 * A plan survives refactorisations of its handle.  Plans and handle may be freed in either order: freeing the handle
 * releases the device memory of its plans, which can then only be freed (a solve with one is CS3_ERR_ARG).
 * On a matched handle indices are in A's rows and columns, as everywhere.
 *
 * Out of scope: skipping the fronts off the elimination-tree paths of the nonzero rows inside the sweeps; batched and
 * Schur handles; a sparse Y; the dense inverse; more than one op per plan. */
typedef struct cs3_sens_s *cs3_sens;
typedef struct cs3_sens_info_t {
    int64_t k, p, side, trans, ntiles, max_width, nnz_b, nnz_c;
} cs3_sens_info_t;
typedef struct cs3_sens_limits_t {
    int64_t max_tile;          /* solved-for columns per tile (CS3_SENS_TILE lowers it per plan) */
    int64_t pad_width;         /* a narrower last tile is padded to this width; a lower CS3_SENS_TILE runs unpadded */
    int64_t scatter_rows;      /* rows of the tile per k_sens_scatter workgroup */
    int64_t scatter_threads;   /* its threads: thread j owns tile columns j, j + scatter_threads, ... */
    int64_t combine_cols;      /* columns of the other operand per k_sens_combine workgroup */
    int64_t combine_lanes;     /* tile columns per k_sens_combine workgroup */
    int64_t tblock;            /* block edge of the transposing store (side left): contiguous doubles per row of Y */
} cs3_sens_limits_t;
int cs3_sens_limits(cs3_sens_limits_t *out);
int cs3_sens_plan(cs3_handle h, int64_t k, const int32_t *Bp, const int32_t *Bi, int64_t p, const int32_t *Ctp,
                  const int32_t *Cti, int64_t side, int64_t trans, cs3_sens *out);
int cs3_sens_free(cs3_sens s);
int cs3_sens_info(cs3_sens s, cs3_sens_info_t *out);
int cs3_sens_solve_dev(cs3_handle h, cs3_sens s, const double *Bx_dev, const double *Ctx_dev, double *Y_dev, void *stream);
int cs3_sens_solve(cs3_handle h, cs3_sens s, const double *Bx, const double *Ctx, double *Y);

/* ---- selected inversion: A^-1 on the pattern of L + U from the held factors -----
 * Many entries of A^-1 at about the cost of a factorisation: the diagonal (fault levels at every bus from diag(Z-bus),
 * variances of a state estimate), the entries on the pattern of A (Thevenin impedances of all branches,
 * Z_ii + Z_jj - Z_ij - Z_ji), the entries on the pattern of the factors.  With B = Q' A Q = L U in pivot order and
 * Z = B^-1, a front with pivots P and update rows C, X = L21 L11^-1 and Y = U11^-1 U12 satisfies (Takahashi)
 *     Z_CP = -Z_CC X,   Z_PC = -Y Z_CC,   Z_PP = U11^-1 L11^-1 - Y Z_CP,
 * and Z_CC lies inside the parent's front: one pass over the assembly tree, parents first, gives Z on the whole
 * pattern of L + U (explicit zeros of amalgamated fronts included).  Cholesky: U = L'.  The handle keeps one dense
 * r x r block per front (cs3_selinv_info_t.zpool_doubles per matrix); a batch below 128 runs in the same launches.
 *
 * cs3_selinv_limits: the orders up to which a front runs as one wave and inside the LDS of one workgroup, the edge of
 *   the matrix-core tiles, the pivots per chunk of the big fronts' triangular solves.  Needs no device.
 * cs3_selinv_dev: computes Z of the current factors into memory the handle owns, asynchronously on `stream`.  The first
 *   call builds the plan and allocates; later calls issue launches only (no host read, no synchronisation).
 * cs3_selinv_info: sizes of the plan (built on first use from the analysis alone: needs no device).
 * cs3_selinv_entries_dev: Zx_dev [batch][nnz(A)], entry p of column j: A^-1(Ai[p], j); trans != 0: A^-1(j, Ai[p]).
 * cs3_selinv_diag_dev: d_dev [batch][n], d[i] = A^-1(i, i) in the caller's labels.
 * cs3_selinv_entries, cs3_selinv_diag: the same into host memory (synchronise); they compute Z first when the handle does
 *   not hold that of the current factors.
 * cs3_selinv_factors: matrix b of the batch on the patterns cs3_get_factors returns, in its (pivot-order) labels:
 *   Zl[p] = Z(Li[p], j) for entry p of column j of L (its unit diagonal maps to the diagonal of Z), Zu[p] = Z(Ui[p], j).
 *   Either may be NULL; Zu must be NULL for Cholesky.  Host form, computes Z when needed.
 * cs3_debug_selinv_plan: returns the number of fronts and, for arrays that are not null, the supernodes in the order they
 *   are computed (parents first), the index of the launch that computes each, the offset in the handle's block of Z of
 *   A^-1(Ai[p], j) for every entry of A and of A^-1(i, i) for every i.  Needs no device.  -1: error.
 *
 * Checks, in this order, none of which needs a device: a null handle or null output: CS3_ERR_ARG; a Schur handle, a
 * matched handle (cs3_analyze_matched: the row permutation makes the pattern unsymmetric) or a matrix-interleaved batch
 * (128 or more matrices): CS3_ERR_ARG with a message that names the reason; no successful factorisation: CS3_ERR_STATE;
 * a *_dev getter before cs3_selinv_dev, or after any later factorisation (cs3_factor*, the fused steps and
 * cs3_import_factor_dev invalidate Z): CS3_ERR_STATE.  Solves, estimates and refinements leave Z alone.
 * With static pivot perturbation the result is the inverse of what the factors represent, not of A.
 * The same factors give the same bits on every run, and a matrix of a batch the bits it gets alone.
 *
 * A handle on the real form of a complex matrix: see "complex selected inversion" below (cs3_cplx_selinv_*).
 * Out of scope: matched, Schur and matrix-interleaved handles; entries outside the pattern of L + U; a variant for
 * transposed handles (trans on the getter covers it); sharding. */
typedef struct cs3_selinv_limits_t { int64_t lds_max_order, wave_max_order, gemm_tile, diag_block; } cs3_selinv_limits_t;
typedef struct cs3_selinv_info_t { int64_t zpool_doubles, nfronts_small, nfronts_big, nlaunches; } cs3_selinv_info_t;
int cs3_selinv_limits(cs3_selinv_limits_t *out);
int cs3_selinv_dev(cs3_handle h, void *stream);
int cs3_selinv_info(cs3_handle h, cs3_selinv_info_t *out);
int cs3_selinv_entries_dev(cs3_handle h, int64_t trans, double *Zx_dev, void *stream);
int cs3_selinv_diag_dev(cs3_handle h, double *d_dev, void *stream);
int cs3_selinv_entries(cs3_handle h, int64_t trans, double *Zx);
int cs3_selinv_diag(cs3_handle h, double *d);
int cs3_selinv_factors(cs3_handle h, int64_t b, double *Zl, double *Zu);
int64_t cs3_debug_selinv_plan(cs3_handle h, int32_t *front, int32_t *launch, int64_t *entry_map, int64_t *diag_map);

/* ---- bilinear forms on the selected inverse: t_i = c_i' A^-1 b_i, the bad-data test of a state estimate -----
 * After a state estimate has been solved with the gain matrix G = H' W H, the largest-normalised-residual test needs
 * Omega_ii = 1/w_i - h_i' G^-1 h_i for every measurement row h_i of H.  Every pair of columns that occurs in one row of H is
 * an entry of H' W H, so all of diag(H G^-1 H') is a short sum over entries that cs3_selinv_dev has already computed: m
 * gathers, not m solves.  The same form with the incidence rows c_l of a real network gives Z_ii + Z_jj - Z_ij - Z_ji of
 * every branch (the self-PTDF and LODF denominators).  In general: m sparse row pairs (c_i, b_i) whose index pairs all lie
 * on the pattern of L + U, and
 *     t_i = sum over the entries a of c_i and b of b_i of (c_a * Z(Cti[a], Bti[b])) * b_b,   Z = A^-1,
 * read from the held selected inverse in one launch.
 *
 * (m, Ctp, Cti) is the CSC pattern of C', that is the rows of C, as cs3_sens_plan takes Ct; (m, Btp, Bti) the same for B.
 * Btp == NULL: B = C, pattern and values (one value array at solve time).  Rows may be unsorted, empty (t_i = +0) or hold a
 * column twice: the terms simply add.
 *
 * cs3_quad_limits: the term counts up to which a row is summed by one lane and by one wave (beyond: by one workgroup), the
 *   threads per workgroup, the positions a lane loads together, the rows per workgroup of the residual reduction.  No
 *   launch has a grid cap: the grids grow with the rows.  Needs no device.
 * cs3_quad_plan: host, from the analysis alone, needs no device.  Checks, in this order: a null handle, out pointer or
 *   Ctp, m < 1 or m > 2^30; pointer arrays not monotone from 0 (or a null index array behind one); an index outside
 *   [0, n); a Schur, matched or matrix-interleaved handle (the refusals of cs3_selinv_*); 2^31 - 1024 terms or more
 *   (a row has nnz(c_i) * nnz(b_i)); a pair (Cti[a], Bti[b]) outside the pattern of L + U, where the message names the row
 *   and the two columns: all CS3_ERR_ARG.  The plan stores, per row and a-major (all b of the first a, then the second a),
 *   the offset of Z(Cti[a], Bti[b]) in the handle's block of Z, and the rows sorted into the three classes.
 * cs3_quad_info: m, nnz(C), nnz(B), the terms, whether B = C, the rows per class.
 * cs3_quad_dev: Cx_dev / Bx_dev [batch][nnz] the values in the plan's entry order (Bx_dev is ignored when B = C), t_dev
 *   [batch][m].  Asynchronous on `stream`.  Checks, in this order: null arguments, a plan made for another handle (or whose
 *   handle was freed): CS3_ERR_ARG; no successful factorisation: CS3_ERR_STATE; no selected inverse of the current factors
 *   (before cs3_selinv_dev, or after any later factorisation): CS3_ERR_STATE.  The first call with a plan uploads its
 *   tables; later calls neither allocate nor synchronise.
 * cs3_quad: the same from host arrays (synchronises); computes Z first when the handle does not hold that of the current
 *   factors; the same bits.
 * cs3_quad_normres_dev (plans with B = C only, CS3_ERR_ARG otherwise): with Hx_dev [batch][nnz] the values of the rows,
 *   w_dev and r_dev [batch][m] the weights and the residuals, per row
 *       t_i as above,  omega_i = 1/w_i - t_i,  rn_i = |r_i| / sqrt(omega_i),
 *   but rn_i = 0 where 1 - w_i t_i <= crit_tol: a critical measurement, whose residual carries no information.
 *   summary_dev [batch][4] = (the largest rn, its row as a double, J = sum w_i (r_i r_i) over all rows, the number of
 *   critical rows).  Ties take the lowest row; a NaN rn ranks above every number.  Any of t_dev, omega_dev, rn_dev may be
 *   NULL.  Two launches beyond the forms: per-workgroup partials over 256 consecutive rows, then one closing workgroup
 *   per matrix.  Checks and state rules of cs3_quad_dev.
 * cs3_quad_normres: the same from and to host arrays (t, omega, rn may be NULL); computes Z first when needed.
 * cs3_debug_quad_plan: for arrays that are not null, the class of every row (0 lane, 1 wave, 2 workgroup), term_ptr
 *   [m + 1] and the offsets term_pos [term_ptr[m]].  Needs no device.
 *
 * Every sum has a fixed order, (c * z) * b with both products rounded, and there are no atomics: the same bits on every run,
 * from both forms, and for a matrix of a batch the bits it gets alone.  A lane-class row adds its terms in order; a
 * wave-class row gives lane l the terms l, l + 64, ... in order, then adds lane l + off into lane l for off = 32, 16, ..., 1;
 * a workgroup-class row does the same with thread j of 256 taking terms j, j + 256, ..., then adds the four waves in order.
 * The reductions of cs3_quad_normres* use the same tree over rows 256 g + j, and thread j of the closing workgroup takes
 * the partials j, j + 256, ... in order.
 * A plan survives refactorisations of its handle.  Plans and handle may be freed in either order: freeing the handle
 * releases the device memory of its plans, which can then only be freed.
 *
 * Out of scope: a complex form (complex C and B behind a complex plan); matched, Schur and matrix-interleaved handles; pairs
 * outside the pattern of L + U;
 * off-diagonal entries of C A^-1 B' (cs3_sens_* covers them); removing the bad measurement and estimating again
 * (cs3_updates_* is the tool); sharding. */
/* (the plan's type is cs3_quadplan: cs3_quad is the host form of the call) */
typedef struct cs3_quad_s *cs3_quadplan;
typedef struct cs3_quad_limits_t {
    int64_t lane_max_terms;    /* rows with at most this many terms: one lane each */
    int64_t wave_max_terms;    /* ... up to this many: one wave each; beyond: one workgroup each */
    int64_t block;             /* threads per workgroup of every kernel */
    int64_t lane_chunk;        /* lane class: positions loaded together before their entries of Z */
    int64_t reduce_rows;       /* rows per workgroup of the partial reduction of cs3_quad_normres* */
} cs3_quad_limits_t;
typedef struct cs3_quad_info_t { int64_t m, nnz_c, nnz_b, nterms, same_operand, rows_lane, rows_wave, rows_workgroup; } cs3_quad_info_t;
int cs3_quad_limits(cs3_quad_limits_t *out);
int cs3_quad_plan(cs3_handle h, int64_t m, const int32_t *Ctp, const int32_t *Cti, const int32_t *Btp, const int32_t *Bti,
                  cs3_quadplan *out);
int cs3_quad_free(cs3_quadplan q);
int cs3_quad_info(cs3_quadplan q, cs3_quad_info_t *out);
int cs3_quad_dev(cs3_handle h, cs3_quadplan q, const double *Cx_dev, const double *Bx_dev, double *t_dev, void *stream);
int cs3_quad(cs3_handle h, cs3_quadplan q, const double *Cx, const double *Bx, double *t);
int cs3_quad_normres_dev(cs3_handle h, cs3_quadplan q, const double *Hx_dev, const double *w_dev, const double *r_dev, double crit_tol,
                         double *t_dev, double *omega_dev, double *rn_dev, double *summary_dev, void *stream);
int cs3_quad_normres(cs3_handle h, cs3_quadplan q, const double *Hx, const double *w, const double *r, double crit_tol, double *t,
                     double *omega, double *rn, double *summary);
int cs3_debug_quad_plan(cs3_quadplan q, int32_t *row_class, int64_t *term_ptr, int64_t *term_pos);

/* ---- Schur complements: factor the interior, return the dense border -----
 * A partial factorisation, as cuDSS, PARDISO, MUMPS and SuperLU_DIST offer it: the caller names ns variables that are NOT
 * eliminated (boundary buses of a network equivalent, the constraint rows of a saddle-point system [[H, G'], [G, 0]], the
 * interface of a subdomain).  With the matrix split as [[A11, A12], [A21, A22]], the Schur variables last, a
 * factorisation returns the dense Schur complement  S = A22 - A21 A11^-1 A12,  and two half-solves carry right-hand sides
 * onto the border and solutions back.  The Schur variables are never pivots, so a zero diagonal there is no obstacle.
 *
 * One design decision: where the factors of the Schur front would go, the handle stores the IDENTITY.  After a
 * factorisation it holds the factors [L11 0; L21 I] [U11 U12; 0 I] (Cholesky: [L11 0; L21 I] and its transpose) of A
 * with A22 replaced by A22 - S + I, and S sits in a buffer the handle owns.  The unchanged forward sweep then leaves
 * b2 - A21 A11^-1 b1 in the Schur rows, the unchanged backward sweep entered with x2 there returns
 * x1 = U11^-1 (y1 - U12 x2), and no sweep kernel knows about Schur sets.
 *
 * cs3_analyze_schur: cs3_analyze with a Schur set schur_idx[ns] (indices of A).  Checks, in this order: those of
 *   cs3_analyze; then a null schur_idx, ns < 1 or ns >= n, an index outside [0, n), a repeated index (the message names
 *   it): CS3_ERR_ARG.  `order` applies to the INTERIOR, the n1 = n - ns other variables: CS3_ORDER_AMD orders the
 *   symmetrised pattern of A11 alone (Schur rows and columns removed, as MUMPS does; q_amd[0 .. n1) is
 *   interior[cs3_amd(A11)] bit for bit), CS3_ORDER_NATURAL takes the interior ascending, CS3_ORDER_GIVEN takes
 *   q_given[n1], a permutation of the interior in A's indices.  The Schur variables follow in the caller's order: the
 *   last ns entries of q are schur_idx, they form the last supernode [n1, n), analysed as if A22 were dense, and no
 *   interior column joins it.  cs3_info.nnz_l, nnz_u and flops_factor count the eliminated columns only (the borders L21
 *   and U12 included, the Schur block not); max_front may be ns.  ns is bounded by the factor pool (ns^2 doubles inside
 *   2^30 per matrix).
 * cs3_schur_info: ns and the list.  Either pointer may be NULL.  On a handle without a Schur set: CS3_ERR_STATE.
 * cs3_schur_get_dev: S_dev [batch][ns, ns] row-major, S[i, j] belongs to (schur_idx[i], schur_idx[j]); an asynchronous
 *   copy of the S of the last factorisation on `stream`.  Cholesky: the full symmetric matrix, S == S' bit for bit.
 * cs3_schur_get: the same into host memory (synchronises).
 * cs3_schur_fwd_dev: X [batch][n, k] row-major in A's rows, as for cs3_solve.  On return row schur_idx[i] holds the
 *   condensed right-hand side (b2 - A21 A11^-1 b1)_i; the interior rows hold the half-solved interior, opaque, to be
 *   handed back unchanged.
 * cs3_schur_bwd_dev: on entry the Schur rows hold x2, the caller's solution of S x2 = g, the interior rows are as fwd
 *   left them; on return X solves A x = b.  After the first call with a given k, fwd and bwd neither allocate nor
 *   synchronise.  cs3_schur_fwd / cs3_schur_bwd: the host forms, the same kernels and bits.
 * All of them before a successful factorisation: CS3_ERR_STATE.
 *
 * On a Schur handle these work as on any other: cs3_factor(_dev), cs3_factor_status (fail_col can only be an interior
 * column), cs3_get_info, cs3_get_ordering, cs3_get_supernodes, cs3_set_pivot_perturbation / cs3_get_perturbed (interior
 * pivots), cs3_residual / matvec(_t)_dev, the cs3_debug_* calls, cs3_free -- and cs3_slogdet(_dev), which reads the pivots
 * and therefore returns sign and log|det| of A11 (log|det A| = log|det A11| + log|det S|).
 * These return CS3_ERR_ARG with a message that says why -- they would silently answer for A22 - S + I in place of A22:
 * cs3_solve*, cs3_solve_t*, the one-sided sweeps (cs3_lsolve, cs3_usolve, cs3_ltsolve, cs3_utsolve and their _dev forms),
 * cs3_factor_solve_dev, cs3_factor_solve_bx_dev, cs3_refine*, cs3_condest*, cs3_updates_plan, cs3_sens_plan, cs3_get_factors, cs3_export_factor_dev,
 * cs3_import_factor_dev.
 *
 * Out of scope: matched handles (a row matching breaks the symmetric partition into interior and border); transposed
 * half-solves; a dense solver for S (rocSOLVER or torch have one); a Schur set with ns = n; sharding one matrix over
 * several GPUs on top of this; a sparse S. */
int cs3_analyze_schur(int64_t kind, int64_t order, int64_t n, const int32_t *Ap, const int32_t *Ai,
                      const int32_t *q_given, int64_t batch, int64_t ns, const int32_t *schur_idx, cs3_handle *out);
int cs3_schur_info(cs3_handle h, int64_t *ns, int32_t *schur_idx);
int cs3_schur_get_dev(cs3_handle h, double *S_dev, void *stream);
int cs3_schur_get(cs3_handle h, double *S);
int cs3_schur_fwd_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_schur_bwd_dev(cs3_handle h, double *X_dev, int64_t k, void *stream);
int cs3_schur_fwd(cs3_handle h, double *X, int64_t k);
int cs3_schur_bwd(cs3_handle h, double *X, int64_t k);

/* ---- factors back to the host in CSparse's CSC form ---------------------
 * L: diagonal FIRST in each column (unit for LU); U: diagonal LAST; row
 * indices sorted otherwise.  Sizes from cs3_info.nnz_l / nnz_u.  NumPy-style
 * ownership: the caller allocates, the library fills.  b = matrix index in
 * the batch.  For Cholesky Up/Ui/Ux must be NULL.  On a matched handle these are the factors of B.  The structure is
 * that of the analysed pattern plus its transpose: on a structurally unsymmetric pattern (B usually is one) positions
 * that the unsymmetric elimination never fills are stored as explicit zeros. */
int cs3_get_factors(cs3_handle h, int64_t b, int32_t *Lp, int32_t *Li, double *Lx,
                    int32_t *Up, int32_t *Ui, double *Ux);

/* ---- moving a factorisation between GPUs (BASELINE config 4) -----------
 * The numeric state of a handle is its factor panels: cs3_info.factor_bytes
 * per matrix, batch matrices back to back.  Export copies them into a caller
 * buffer in HBM (which RCCL then broadcasts); import installs such a buffer in
 * a handle that analysed the SAME pattern with the SAME ordering, after which
 * it solves as if it had factorised itself.  Matched handles: CS3_ERR_ARG. */
int cs3_export_factor_dev(cs3_handle h, double *dst_dev, void *stream);
int cs3_import_factor_dev(cs3_handle h, const double *src_dev, void *stream);

/* ---- diagnostics --------------------------------------------------------
 * With CS3_PROFILE=1 in the environment every LDS-resident front records six
 * shader-clock stamps (descriptor read, zeroed, assembled, eliminated, staged,
 * stored) relative to its start; out[nsuper][8] in schedule order.  Not part
 * of the reference-facing surface.  CS3_PROFILE=2: the same, except that a big
 * front's block step stamps its diagonal tile instead of tile (1, 0). */
int cs3_debug_front_stamps(cs3_handle h, int64_t *out);
/* Fills the LDS of every CU with NaN bit patterns (the LDS keeps its contents between kernels): the parity tests call it
 * before the numeric entry points so that a product of a masked zero and an unwritten LDS word cannot hide. */
int cs3_debug_poison_lds(void *stream);
/* on != 0: the producers of the LDS hand-overs between waves (shared eliminations: the pivot blocks of the big fronts in
 * k_big_step, the shared fronts of the bottom forest) keep their counters back, so every consumer runs into its bounded
 * wait and gives up: the step must then be reported as failed by cs3_factor_status (CS3_ERR_STATE), never pass silently.
 * Process-wide; on = 0 restores the normal path.  For the test of that path. */
int cs3_debug_withhold_handover(int on);
/* Diagnostic, for the tests of the "no allocation, no synchronisation" contracts: how many device allocations (graph
 * instantiations included) and host synchronisations the handle has made so far in its solves and in the paths built on
 * them (the low-rank-modified solves).  Either pointer may be NULL. */
int cs3_debug_alloc_counters(cs3_handle h, int64_t *allocs, int64_t *syncs);
/* Diagnostic, for the test of device-memory lifetime: the number of device blocks the library holds right now, over all
 * handles, plans and calls in flight (process-wide, needs no handle and no device).  0 once everything has been freed. */
int64_t cs3_debug_live_device_buffers(void);
/* The tiles of a plan of low-rank-modified solves: returns their number and, for arrays that are not null, per tile its
 * first case, its number of cases, its touched rows and the number of right-hand sides it is solved with (the touched rows
 * rounded up to a multiple of 64, at most the tile width).  Diagnostics, tests and tools. */
int64_t cs3_debug_updates_tiles(cs3_updates u, int32_t *first_case, int32_t *ncases, int32_t *nrows, int32_t *width);
/* diagnostics, for timing: the steps of a cs3_sens_solve_dev call selected by the mask `parts` (1: k_sens_scatter, 2: the
 * solves, 4: k_sens_combine), over all tiles of the plan, on whatever the tile buffer holds.  Arguments and checks as for
 * cs3_sens_solve_dev; parts outside 1 .. 7: CS3_ERR_ARG. */
int cs3_debug_sens_parts(cs3_handle h, cs3_sens s, int64_t parts, const double *Bx_dev, const double *Ctx_dev, double *Y_dev,
                         void *stream);
/* diagnostics, for tests: the first `count` doubles of the handle's tile buffer (the one cs3_sens_* and cs3_cplx_sens_* solve
 * in; it exists after the first solve with a plan) copied to `host`, or with write != 0 from `host` into it, so that a
 * test can look at what a scatter wrote (parts = 1) and choose what a combine reads (parts = 4).  Synchronises.  More
 * than the buffer holds: CS3_ERR_ARG. */
int cs3_debug_sens_tile(cs3_handle h, int64_t write, double *host, int64_t count);
/* Factorisation schedule: supernode id, front order r and width w per schedule slot. */
int cs3_debug_schedule(cs3_handle h, int32_t *sched, int32_t *front_r, int32_t *front_w);
/* The launch plan of an operation on this handle (op 0: factorisation, 1 / 2: forward / backward sweep, 3: the fused step =
 * factorisation with forward sweep, then the backward sweep's plan, 4 / 5: Schur forward / backward) with nrhs right-hand
 * sides (op 0: ignored); trans: the transposed sweeps (op 1 / 2, LU).  Returns the number of steps and writes at most cap
 * of them to rows (may be NULL), 10 int32 each: step kind (StepKind of csrc/cs3_device.hpp: 0 front group, 1 big gather,
 * 2 big block, 3 Schur take, 4 / 5 sweep group forward / backward, 6 / 7 big-sweep forward pre / chunk, 8 / 9 backward
 * pre / chunk, 10 event record, 11 stream wait), stream slot (0: the caller's stream, 1 .. 3: side streams, 4: aux), the
 * group's first, count, cls, level, max_r, max_w (zeros for 10 / 11), argument (block or chunk, else -1), event number
 * (10 / 11, else -1; counted from 0 per plan, so op 3 counts twice).  Needs no device.  -1: error. */
int64_t cs3_debug_launch_plan(cs3_handle h, int32_t op, int64_t nrhs, int32_t trans, int32_t *rows, int64_t cap);
/* The bottom forest (subtrees of small fronts walked by one workgroup each, all in one launch): returns the
 * number of forest fronts (0: no forest) and, for arrays that are not null, per forest front in task order its supernode,
 * its task and its local level inside the task.  tier[] is kept for existing callers and always receives 0 (the forest
 * is one launch).  Diagnostics and tests. */
int64_t cs3_debug_forest(cs3_handle h, int32_t *supernode, int32_t *task, int32_t *level, int32_t *tier);

/* ---- general triangular solves on caller-supplied CSC factors -----------
 * cs_lsolve / cs_usolve lineage, the csc_lsolve_f(n, Lp, Li, Lx, x) shape of
 * x[n, k] row-major, in place; diagonal first (L) /
 * last (U) in each column.  Level-scheduled on the device. */
int cs3_csc_lsolve(int64_t n, const int32_t *Lp, const int32_t *Li, const double *Lx,
                   double *x, int64_t k);
int cs3_csc_usolve(int64_t n, const int32_t *Up, const int32_t *Ui, const double *Ux,
                   double *x, int64_t k);
/* x = L' \ x and x = U' \ x on the same arrays (cs_ltsolve / cs_utsolve): the columns of L and U are the rows of
 * their transposes, so nothing is transposed; level-scheduled on the device. */
int cs3_csc_ltsolve(int64_t n, const int32_t *Lp, const int32_t *Li, const double *Lx,
                    double *x, int64_t k);
int cs3_csc_utsolve(int64_t n, const int32_t *Up, const int32_t *Ui, const double *Ux,
                    double *x, int64_t k);

/* ---- neighbours of the path -----------------------
 * y = A x on the device, csc_mat_vec_ff (csc_numba.py:309-328) semantics;
 * X [n, k] and Y [m, k] row-major as csc_matvecs (sparsetools/csc.h:68-84). */
int cs3_csc_matvec(int64_t m, int64_t n, const int32_t *Ap, const int32_t *Ai,
                   const double *Ax, const double *X, double *Y, int64_t k);

/* [[A, B], [C, D]] in CSC on the device: csc_stack_4_by_4_ff / pack_4_by_4 (csc_numba.py:640-720,
 * csc.py:588-606), the power-flow Jacobian assembly.  Argument order (m, n, indices, indptr, data)
 * as in the reference; outputs Pi[nnz], Pp[an+bn+1], Px[nnz] with nnz = the four blocks' nnz,
 * caller-allocated.  Incompatible block shapes (the reference asserts) give CS3_ERR_ARG. */
int cs3_csc_stack_4_by_4(int64_t am, int64_t an, const int32_t *Ai, const int32_t *Ap, const double *Ax,
                         int64_t bm, int64_t bn, const int32_t *Bi, const int32_t *Bp, const double *Bx,
                         int64_t cm, int64_t cn, const int32_t *Ci, const int32_t *Cp, const double *Cx,
                         int64_t dm, int64_t dn, const int32_t *Di, const int32_t *Dp, const double *Dx,
                         int32_t *Pi, int32_t *Pp, double *Px);

/* The same with every array already in HBM (device pointers in and out, asynchronous on `stream`): the Jacobian is
 * assembled where the factorisation reads it, so  stack -> cs3_factor_solve_dev  runs without a host copy.  nnz_* are
 * the blocks' entry counts (Ap[an] ...), passed by the caller so that nothing has to come back to the host.
 * map (optional, [nnz]): position of every output entry in the concatenation A | B | C | D of the value arrays. */
int cs3_csc_stack_4_by_4_dev(int64_t am, int64_t an, int64_t nnz_a, const int32_t *Ai_dev, const int32_t *Ap_dev, const double *Ax_dev,
                             int64_t bm, int64_t bn, int64_t nnz_b, const int32_t *Bi_dev, const int32_t *Bp_dev, const double *Bx_dev,
                             int64_t cm, int64_t cn, int64_t nnz_c, const int32_t *Ci_dev, const int32_t *Cp_dev, const double *Cx_dev,
                             int64_t dm, int64_t dn, int64_t nnz_d, const int32_t *Di_dev, const int32_t *Dp_dev, const double *Dx_dev,
                             int32_t *Pi_dev, int32_t *Pp_dev, double *Px_dev, int32_t *map_dev, void *stream);
/* Newton-loop restack: the blocks' patterns have not changed, only their values -- Px[p] = (A | B | C | D)[map[p]] with the
 * map of the first stacking.  One gather kernel; its output is what cs3_factor_solve_dev takes as Ax_dev. */
int cs3_restack_values_dev(int64_t nnz, const int32_t *map_dev, int64_t nnz_a, int64_t nnz_b, int64_t nnz_c,
                           const double *Ax_dev, const double *Bx_dev, const double *Cx_dev, const double *Dx_dev,
                           double *Px_dev, void *stream);

/* ---- format conversions and utilities on the device ----
 * Same outputs as the reference's Python kernels, bit for bit (tests/golden/): output ORDER included.
 * Host pointers in and out; results are caller-allocated. */
/* C = A' (csc_transpose, csc_numba.py:400-436); the same three arrays are A in CSR form
 * (csc_to_csr, :360-397).  Cp[m + 1], Ci / Cx[nnz]. */
int cs3_csc_transpose(int64_t m, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                      int32_t *Cp, int32_t *Ci, double *Cx);
/* Triplets to CSC, duplicates kept, triplet order inside a column (coo_to_csc, csc_numba.py:331-357). */
int cs3_coo_to_csc(int64_t m, int64_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, const double *Tx,
                   int32_t *Cp, int32_t *Ci, double *Cx);
/* 1-norm: max column sum of |x| (csc_norm, csc_numba.py:723-739). */
int cs3_csc_norm(int64_t n, const int32_t *Ap, const double *Ax, double *norm);
/* C = alpha A + beta B (csc_add_ff, csc_numba.py:183-219).  Ci / Cx: room for nnz(A) + nnz(B); used: Cp[n]. */
int cs3_csc_add(int64_t m, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                const int32_t *Bp, const int32_t *Bi, const double *Bx, double alpha, double beta,
                int32_t *Cp, int32_t *Ci, double *Cx);
/* B = A[rows, cols] exactly as csc_sub_matrix computes it (csc_numba.py:464-502), its running row counter
 * included.  Bp[ncols + 1]; Bi / Bx: room for b_cap entries (the reference allocates nnz(A)); used: Bp[ncols].
 * Repeated rows / columns can need more than nnz(A): then Bp is filled, nothing else is written and the call
 * returns CS3_ERR_ARG (the reference runs off its arrays there). */
int cs3_csc_sub_matrix(int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                       const int32_t *rows, int64_t nrows, const int32_t *cols, int64_t ncols,
                       int32_t *Bp, int32_t *Bi, double *Bx, int64_t b_cap);
/* label[i] = the node at which find_islands (csc_numba.py:744-808) opens the island that receives node i = the smallest
 * node that reaches i along column -> row edges.  On a structurally symmetric pattern that is the smallest node of i's
 * connected component; on an unsymmetric one it follows the reference's directed search exactly.  find_islands lists
 * islands by ascending start node and CscMat.islands (csc.py:515-521) sorts each -- both follow from the labels. */
int cs3_find_islands(int64_t n, const int32_t *Ap, const int32_t *Ai, int32_t *label);

/* ---- sparse products: C = A B and C = A' B with a reusable plan ----------
 * csc_multiply_ff (csc_numba.py:222-306, Gustavson's product) on the device, bit for bit: for column j of C the products
 * are enumerated as the reference's loops do (pb over B(:, j) in stored order, inside it pa over A(:, Bi[pb]) in stored
 * order; position t); the rows of C(:, j) are the distinct rows in order of FIRST occurrence in t (not sorted), the value
 * of a row is ((v1 + v2) + v3) + ... over its products v = Bx[pb] * Ax[pa] in ascending t, every product rounded on its
 * own (no fused multiply-add) and the first one stored as it is ((-1) * 0 gives -0.0).  Explicit zeros, cancellations,
 * unsorted rows and duplicate entries inside a column of A or B are kept and handled as those loops handle them.  The
 * reference sizes its workspaces by the columns of C and so only runs when Am <= Bn; this one is defined for every shape
 * by the same rule.
 *
 * Two phases, as analysis and factorisation are: a matrix product inside an iteration (the gain matrix H' W H of a
 * Gauss-Newton step, Y = Cf' Yf Cf) has a fixed pattern and new values every step.
 * cs3_spgemm_plan_create: host patterns.  C is Am x Bn; with transpose_a != 0 the plan computes C = T B, An x Bn, where
 *   T = csc_transpose(A) as the reference's kernel defines it (columns of T = rows of A, entries in ascending column of A,
 *   duplicates in stored order) -- the numeric phase reads A's OWN value array through recorded positions, no transposed
 *   copy of the values is ever made.  Checked on the host, in this order, before anything is uploaded: null output,
 *   negative dimensions, dimensions above INT_MAX, inner dimensions (An, or Am when transposing, against Bm), then for A and
 *   for B: null indptr, indptr[0] != 0, a decreasing indptr, null indices with entries, an index outside [0, Am) resp.
 *   [0, Bm); then a product that needs 2^31 - 1024 multiplications or more: CS3_ERR_ARG with a message.  After that the
 *   device is required (CS3_ERR_HIP without one) and the symbolic product runs there; lists that would pad to 2^31 - 1024
 *   pairs or more are CS3_ERR_ARG too.  CS3_SPGEMM_LONG in the environment, read by this call and by cs3_spgemm_limits,
 *   moves the long-list threshold (2 ... 2^20; for measurements and tests).
 * cs3_spgemm_plan_info: sizes, and how much went through each path (the tests use it to prove that every path ran).
 * cs3_spgemm_limits: the constants that separate the paths.
 * cs3_spgemm_plan_pattern: Cp[Bn + 1], Ci[nnz_c] to the host.  cs3_spgemm_plan_pattern_dev: borrowed device pointers,
 *   valid until the plan is freed (either may be NULL).
 * cs3_spgemm_values_dev: Cx_dev[nnz_c] from Ax_dev[nnz(A)], Bx_dev[nnz(B)], asynchronous on `stream`: at most two
 *   launches, no allocation, no host synchronisation.  cs3_spgemm_values: the same from host arrays (synchronises). */
typedef struct cs3_spgemm_s *cs3_spgemm;
typedef struct cs3_spgemm_info {
    int64_t m, n;                  /* shape of C */
    int64_t nnz_a, nnz_b, nnz_c;
    int64_t products;              /* multiplications = pairs over all lists */
    int64_t cols_lds, cols_global; /* symbolic: columns of C through the LDS hash table / the global table (empty ones: neither) */
    int64_t entries_sliced, entries_long;  /* numeric: entries of C added up by one lane of a slice / by a wave of their own */
    int64_t padded_pairs;          /* pairs stored: slices padded to their longest list + the long lists */
    int64_t long_list;             /* the threshold this plan was built with */
} cs3_spgemm_info;
typedef struct cs3_spgemm_limits_t {
    int64_t lds_products;          /* most products of a column that takes the LDS path; one more goes to the global table */
    int64_t lds_table_rows;        /* most distinct rows the LDS table holds (= lds_products: it is at most half full) */
    int64_t long_list;             /* a list of this many pairs or more leaves its slice */
    int64_t slice_width;           /* entries of C per slice */
    int64_t rank_chunk_lds, rank_chunk_global;   /* products ranked together in the two symbolic paths */
} cs3_spgemm_limits_t;
int cs3_spgemm_limits(cs3_spgemm_limits_t *out);
int cs3_spgemm_plan_create(int64_t Am, int64_t An, const int32_t *Ap, const int32_t *Ai,
                           int64_t Bm, int64_t Bn, const int32_t *Bp, const int32_t *Bi, int transpose_a, cs3_spgemm *out);
int cs3_spgemm_plan_free(cs3_spgemm plan);
int cs3_spgemm_plan_info(cs3_spgemm plan, cs3_spgemm_info *info);
int cs3_spgemm_plan_pattern(cs3_spgemm plan, int32_t *Cp, int32_t *Ci);
int cs3_spgemm_plan_pattern_dev(cs3_spgemm plan, const int32_t **Cp_dev, const int32_t **Ci_dev);
int cs3_spgemm_values_dev(cs3_spgemm plan, const double *Ax_dev, const double *Bx_dev, double *Cx_dev, void *stream);
int cs3_spgemm_values(cs3_spgemm plan, const double *Ax, const double *Bx, double *Cx);

/* ---- union plans: matrices whose patterns differ, on ONE batched handle ----
 * A family of matrices of one order whose patterns are all contained in a small common pattern (the contingency cases,
 * switching states or topology scans of one network: the base case minus a few branches) can run as one batched handle on
 * the UNION of the patterns: a matrix padded with explicit zeros to the union has the factors of the unpadded matrix
 * embedded in the union's structure.  The plan computes the union and the place of every entry once; one kernel then moves
 * the ragged per-matrix value arrays into the [nmat][nnz_union] layout that cs3_factor_solve_dev and every other call of
 * a handle with batch = nmat reads, as often as the values change, without a host copy.
 *
 * cs3_union_plan_create: nmat >= 1 host patterns (Ap[b][n + 1], Ai[b][nnz_b]) of order n, as arrays of pointers; rows
 *   inside a column need not be sorted and may repeat.  Host work only, O(entries of the distinct patterns + n) and a sort
 *   per union column; no device is needed.  Checked in this order, each failure CS3_ERR_ARG with a message: null output,
 *   null pointer arrays, nmat < 1, n outside [0, 2^30) (the range cs3_analyze takes), a null Ap[b]; then per member
 *   Ap[b][0] != 0, a decreasing Ap[b], null Ai[b] with entries, a row outside [0, n); then a member, and then a union, of
 *   2^31 - 1024 entries or more.
 *   Union column j = the rows that occur in column j of any member, ASCENDING: independent of the order of the members.
 *   Members whose (Ap, Ai) are equal element for element share one gather map (distinct_patterns counts the maps).
 * cs3_union_plan_pattern: Up[n + 1], Ui[nnz_union] (either may be NULL).  cs3_union_plan_offsets: off[nmat + 1], prefix
 *   sums of nnz_b: the ragged value buffer Ax_cat is the members' value arrays one after the other, member b at off[b].
 * cs3_union_plan_slots: slot[nnz_b], the union entry that every entry of member b lands on.
 * cs3_union_values_dev: Ax_union_dev[nmat][nnz_union] from Ax_cat_dev[off[nmat]], asynchronous on `stream`: ONE launch,
 *   no memset, no atomics, no allocation, no host synchronisation -- it can be captured into a graph once the tables are
 *   on the device (they are uploaded by the first call or by cs3_union_upload).  Every output entry is written:
 *     no source in member b           +0.0
 *     one source s                    the bit pattern of Ax_cat[off[b] + s] (-0.0, infinities, NaN payloads survive)
 *     several, s1, s2, ... as stored  ((v1 + v2) + v3) + ..., plain double additions from v1 as stored
 *   Ax_union_dev must be 8-byte aligned.
 * cs3_union_values: the same from and to host arrays (synchronises).  Both return CS3_ERR_HIP without a device.
 * cs3_union_limits: the constants that shape the launch. */
typedef struct cs3_union_s *cs3_union;
typedef struct cs3_union_info {
    int64_t n, nmat;
    int64_t nnz_union;
    int64_t nnz_total;             /* entries of all members = length of the ragged value buffer */
    int64_t distinct_patterns;     /* gather maps held */
    int64_t padded;                /* nmat * nnz_union - output entries that have a source */
    int64_t dup_slots;             /* output entries with more than one source, over all members */
} cs3_union_info;
typedef struct cs3_union_limits_t {
    int64_t block;                 /* threads of a workgroup */
    int64_t grid_cap;              /* most workgroups of a launch: beyond grid_cap * block * entries_per_lane entries a lane loops */
    int64_t entries_per_lane;
} cs3_union_limits_t;
int cs3_union_limits(cs3_union_limits_t *out);
int cs3_union_plan_create(int64_t n, int64_t nmat, const int32_t *const *Ap, const int32_t *const *Ai, cs3_union *out);
int cs3_union_plan_free(cs3_union p);
int cs3_union_plan_info(cs3_union p, cs3_union_info *info);
int cs3_union_plan_pattern(cs3_union p, int32_t *Up, int32_t *Ui);
int cs3_union_plan_offsets(cs3_union p, int64_t *off);
int cs3_union_plan_slots(cs3_union p, int64_t b, int32_t *slot);
int cs3_union_upload(cs3_union p);
int cs3_union_values_dev(cs3_union p, const double *Ax_cat_dev, double *Ax_union_dev, void *stream);
int cs3_union_values(cs3_union p, const double *Ax_cat, double *Ax_union);

/* ---- complex matrices: A z = b through a real-equivalent plan -------------
 * A complex matrix of order n (an admittance matrix Y of Y v = i) is solved as a REAL matrix of order 2n on an ordinary
 * handle: every entry w becomes the 2 x 2 block [[Re w, -Im w], [Im w, Re w]], rows and columns interleaved (2i, 2i + 1),
 * so the blocks stay dense, the assembly tree is that of the complex pattern with every supernode twice as wide, and the
 * real multiplications are those of complex arithmetic (the factors take twice the memory).  The plan holds the pattern
 * arithmetic, the doubled order and the device glue; the handle runs unchanged behind it:
 *     cs3_cplx_plan_create(n, Ap, Ai, batch, rotate, &p);  cs3_cplx_plan_pattern(p, Rp, Ri);  cs3_cplx_plan_order(p, order, q, q2);
 *     cs3_analyze(kind, CS3_ORDER_GIVEN, 2 n, Rp, Ri, q2, batch, &h);
 *     cs3_cplx_values_dev(p, Az, Rx, st);  cs3_cplx_pack_dev(p, op, B, Y, k, st);
 *     cs3_factor_solve_bx_dev(h, Rx, tol, Y, X2, k, st);   (or cs3_factor_dev, then cs3_solve_dev / cs3_solve_t_dev on Y)
 *     cs3_cplx_unpack_dev(p, op, X2, X, k, 0, st);
 * A complex array is interleaved (re, im) doubles -- numpy.complex128, C's double complex -- typed const double * here and
 * aligned to 16 bytes.
 *
 * ROTATION.  The static pivots of the real form are the REAL PARTS of the diagonal, and the diagonal of an admittance matrix
 * is mostly imaginary (purely imaginary for a lossless network: the first pivot is exactly 0).  With CS3_CPLX_ROTATE_DIAG
 * row i is multiplied by s_i = conj(d_i) / max(|Re d_i|, |Im d_i|), d_i the diagonal entry: M = diag(s) A has a real,
 * positive diagonal, and 1 <= |s_i| <= sqrt(2).  Per matrix of the batch and row i:
 *     d = the stored (i, i) entries added in storage order, starting from the first as stored, Re and Im separately
 *     m = max(|Re d|, |Im d|);  s_i = (Re d / m, (-Im d) / m)
 *     s_i = (1, +0) with CS3_CPLX_ROTATE_NONE, without a stored diagonal, and when m is 0, NaN or infinite.
 * Only divisions and comparisons: a host reproduces s bit for bit.  s [batch][n] lives in the plan and belongs to the
 * last values call, in stream order (before the first one it is (1, +0)).  A row scaling breaks symmetry: Cholesky
 * handles take CS3_CPLX_ROTATE_NONE (the real form of a Hermitian positive definite matrix is symmetric positive definite).
 *
 * ARITHMETIC.  a * b = ((ar*br) - (ai*bi), (ar*bi) + (ai*br)): every product rounded, then the sum, nothing fused;
 * conj() and the -Im w of a block are sign flips (a zero keeps its mirrored sign).
 *
 * cs3_cplx_plan_create: host work only, O(nnz + n).  Checked in this order, each failure CS3_ERR_ARG with a message: null
 *   output; batch < 1; rotate outside the enum; n outside [0, 2^29) (2n stays in the range cs3_analyze takes); a null Ap,
 *   Ap[0] != 0, a decreasing Ap, a null Ai with entries, a row outside [0, n); 4 nnz >= 2^31 - 1024.  Rows inside a column
 *   need not be sorted; an entry stored twice stays two entries.
 * cs3_cplx_plan_pattern: Rp[2n + 1], Ri[4 nnz] (either may be NULL): Rp[2j] = 4 Ap[j], Rp[2j + 1] = 4 Ap[j] + 2 len_j;
 *   entry t of column j (row i, storage order kept) owns Rp[2j] + 2t, + 1 and Rp[2j + 1] + 2t, + 1, with rows
 *   2i, 2i + 1, 2i, 2i + 1 and values Re w, Im w, -(Im w), Re w.
 * cs3_cplx_plan_order: q2[2n] with q2[2t] = 2 q[t], q2[2t + 1] = 2 q[t] + 1, q = cs3_amd(order, ...) of the complex pattern,
 *   or q_given[n] with CS3_ORDER_GIVEN (not a permutation: CS3_ERR_ARG).  Pass it on with CS3_ORDER_GIVEN.
 * cs3_cplx_values_dev: Rx_dev [batch][4 nnz] from Az_dev [batch][nnz] complex: the rotation (one launch, only with
 *   CS3_CPLX_ROTATE_DIAG), then w = s_i * z for every entry (one launch).  Every output entry is written once; no memset,
 *   no atomics; after the first call (which uploads the tables, as cs3_cplx_upload does) nothing allocates or
 *   synchronises, so the call can be captured into a graph.  Both arrays 16-byte aligned.
 * cs3_cplx_pack_dev: Y_dev [batch][2n, k] real row-major from Z_dev [batch][n, k] complex row-major:
 *   Y[2i, c] = Re u, Y[2i + 1, c] = Im u;    op N: u = s_i * z     op H: u = z              op T: u = conj(z)
 * cs3_cplx_unpack_dev: the inverse, y = Y[2i, c] + j Y[2i + 1, c]:
 *                                            op N: y               op H: conj(s_i) * y      op T: s_i * conj(y)
 *   stored to Z, or with accumulate != 0 added to it (z + result, one addition per component).
 *   Between the two: op N cs3_solve_dev, ops H and T cs3_solve_t_dev.  The transpose of the real form of M is the real
 *   form of M^H, so the transposed solve of the handle solves with M^H = A^H diag(conj(s)); A^T x = b is
 *   A^H conj(x) = conj(b).
 * cs3_cplx_residual_dev: R = B - op(A) X on the complex CSC itself, the CALLER's values Az_dev, not the rotated ones;
 *   B, X, R [batch][n, k] complex.  The accumulator starts at b and subtracts term by term, t = a * x (op H: conj(a) * x):
 *   op N over row i's entries by ascending column, storage order inside a column; ops T and H over column j in storage order.
 * cs3_cplx_rotation_dev: the plan's s [batch][n] complex on the device.
 * cs3_cplx_workspace_dev: a block of `count` doubles that the plan owns, slot 0, 1 or 2, grown (after a device
 *   synchronisation) only when count exceeds what the slot holds: for callers that keep no buffers of their own.
 * cs3_cplx_values / _pack / _unpack / _residual / _rotation: the same from and to host arrays: the same kernels, the same
 *   bits (they synchronise).  Everything that touches the device returns CS3_ERR_HIP without one.
 * cs3_cplx_limits: the constants that shape the launches.
 * Not offered: complex arithmetic inside the factor and sweep kernels, matching or perturbation of complex matrices, the
 * phase of a determinant (cs3_slogdet of the handle gives 2 log|det M|). */
typedef struct cs3_cplx_s *cs3_cplx;
enum cs3_cplx_rotate { CS3_CPLX_ROTATE_NONE = 0, CS3_CPLX_ROTATE_DIAG = 1 };
enum cs3_cplx_op { CS3_CPLX_N = 0, CS3_CPLX_T = 1, CS3_CPLX_H = 2 };      /* A, A^T (no conjugate), A^H */
typedef struct cs3_cplx_info {
    int64_t n, nnz, batch, rotate;
    int64_t n_real, nnz_real;      /* 2 n, 4 nnz: what the handle analyses */
    int64_t rows_without_diagonal; /* rows whose s stays (1, +0) whatever the values */
} cs3_cplx_info;
typedef struct cs3_cplx_limits_t {
    int64_t block;                 /* threads of a workgroup */
    int64_t grid_cap;              /* most workgroups of a launch: beyond grid_cap * block complex numbers a lane loops */
} cs3_cplx_limits_t;
int cs3_cplx_limits(cs3_cplx_limits_t *out);
int cs3_cplx_plan_create(int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, cs3_cplx *out);
int cs3_cplx_plan_free(cs3_cplx p);
int cs3_cplx_plan_info(cs3_cplx p, cs3_cplx_info *info);
int cs3_cplx_plan_pattern(cs3_cplx p, int32_t *Rp, int32_t *Ri);
int cs3_cplx_plan_order(cs3_cplx p, int64_t order, const int32_t *q_given, int32_t *q2);
int cs3_cplx_upload(cs3_cplx p);
int cs3_cplx_workspace_dev(cs3_cplx p, int64_t slot, int64_t count, double **out);
int cs3_cplx_values_dev(cs3_cplx p, const double *Az_dev, double *Rx_dev, void *stream);
int cs3_cplx_pack_dev(cs3_cplx p, int64_t op, const double *Z_dev, double *Y_dev, int64_t k, void *stream);
int cs3_cplx_unpack_dev(cs3_cplx p, int64_t op, const double *Y_dev, double *Z_dev, int64_t k, int64_t accumulate, void *stream);
int cs3_cplx_residual_dev(cs3_cplx p, int64_t op, const double *Az_dev, const double *B_dev, const double *X_dev,
                          double *R_dev, int64_t k, void *stream);
int cs3_cplx_rotation_dev(cs3_cplx p, const double **s_dev);
int cs3_cplx_values(cs3_cplx p, const double *Az, double *Rx);
int cs3_cplx_pack(cs3_cplx p, int64_t op, const double *Z, double *Y, int64_t k);
int cs3_cplx_unpack(cs3_cplx p, int64_t op, const double *Y, double *Z, int64_t k, int64_t accumulate);
int cs3_cplx_residual(cs3_cplx p, int64_t op, const double *Az, const double *B, const double *X, double *R, int64_t k);
int cs3_cplx_rotation(cs3_cplx p, double *s);

/* ---- complex sparse right-hand sides: Y = C op(A)^-1 B, entries of Z-bus ----
 * cs3_sens_* for a complex matrix behind a complex plan: Thevenin impedances at p faulted buses, transfer impedances
 * between a few buses, the columns of Z-bus = Y^-1 a short-circuit study needs.  The handle h holds the real form of
 * diag(s) A (above); its sweeps run unchanged, and two kernels of their own (csrc/cplxsens.hip) scatter the complex
 * solved-for columns into the real tile and combine the solutions with the other operand.  ONE complex solved-for column
 * is ONE real column of a [2n, w] tile: side left with p rows of C costs p transposed solves, where cs3_sens_plan on the
 * real form would need the real and the imaginary row of every row of C, 2p -- and could not apply s, which lives on the
 * device.
 *
 * Operands as for cs3_sens_plan, in the indices of the COMPLEX matrix: B (n x k) by columns, C (pr x n) by rows as the CSC
 * arrays of C' (no conjugate); a null Bp / Ctp is the identity.  Bz, Ctz, Y [pr, k] row-major are interleaved complex,
 * typed double *, aligned to 16 bytes.  op is a cs3_cplx_op: A, A^T (no conjugate) or A^H.
 *
 * With Solve_op(r) = unpack_op(real solve(pack_op(r))), pack and unpack exactly those of cs3_cplx_pack_dev /
 * cs3_cplx_unpack_dev, the real solve cs3_solve_dev for N and cs3_solve_t_dev for T and H, s read from the plan as it
 * stands in stream order:
 *     side, op            inner op     conjugate the solved-for values first, and the solution before the product
 *     right, N / T / H    N / T / H    no
 *     left, N             T            no
 *     left, T             N            no
 *     left, H             N            yes      (A^-H = conj(A^-T): conj(A)^-1 c = conj(A^-1 conj(c)))
 *   side right: X = Solve_inner(B[:, tile]),  Y[g, c] = sum_e C[g, i_e] * x[i_e, c]   over the entries of row g of C
 *   side left:  W = Solve_inner(C'[:, tile]), Y[r, g] = sum_e B[i_e, g] * w[i_e, r]   over the entries of column g of B
 *   k_csens_scatter writes u = pack_inner(v) (v conjugated first where the table says so) as Re u in row 2i, Im u in row
 *   2i + 1 of a zeroed tile; duplicates ADD in storage order, each component on its own (the first to +0); an identity
 *   operand STORES pack_inner((1, +0)).  k_csens_combine unpacks the pair (T[2i, j], T[2i + 1, j]), conjugates where the
 *   table says so, multiplies by the other operand's value (ARITHMETIC above); the first product starts the sum, later
 *   ones add component by component in storage order; an identity operand hands the unpacked solution over.  No atomics:
 *   the same bits on every run.
 *
 * cs3_cplx_sens_plan: host, pattern only, needs no GPU.  Checks, in this order: a null p or h (or out); a handle whose
 *   order is not 2 n of the plan; a handle with batch > 1; a Schur handle; then those of cs3_sens_plan from "k < 1" on, in
 *   its order and wording, and op outside the enum.  Side 0, the tiles (CS3_SENS_TILE is read by this call too), the one
 *   tile buffer on the handle and the lifetime rules are cs3_sens_plan's: the plan survives refactorisations -- the new s
 *   is picked up --, handle and plan may be freed in either order, after the first call nothing allocates or synchronises.
 * cs3_cplx_sens_info: as cs3_sens_info; .trans holds op.   cs3_cplx_sens_limits: the constants of the complex kernels
 *   (scatter_rows counts REAL rows of the tile: half as many complex rows; tblock counts complex numbers).
 * cs3_cplx_sens_solve_dev: asynchronous on `stream`.  Checks: null arguments, a plan made for another handle, a complex
 *   plan of another order, misaligned arrays: CS3_ERR_ARG; no successful factorisation: CS3_ERR_STATE.
 * cs3_cplx_sens_solve: the same from host arrays (synchronises); the same bits.
 * cs3_debug_cplx_sens_parts: the steps selected by the mask `parts` as for cs3_debug_sens_parts (1 scatter, 2 solve,
 *   4 combine).
 * Out of scope: batched plans, a sparse Y, skipping fronts off the elimination-tree paths of the right-hand sides; the
 * CscMat sugar (CscMat.sensitivities refuses complex data, and a test pins that refusal: it waits for a change that may
 * edit that test). */
typedef struct cs3_cplx_sens_s *cs3_cplx_sens;
int cs3_cplx_sens_limits(cs3_sens_limits_t *out);
int cs3_cplx_sens_plan(cs3_cplx p, cs3_handle h, int64_t k, const int32_t *Bp, const int32_t *Bi, int64_t pr,
                       const int32_t *Ctp, const int32_t *Cti, int64_t side, int64_t op, cs3_cplx_sens *out);
int cs3_cplx_sens_free(cs3_cplx_sens s);
int cs3_cplx_sens_info(cs3_cplx_sens s, cs3_sens_info_t *out);
int cs3_cplx_sens_solve_dev(cs3_cplx p, cs3_handle h, cs3_cplx_sens s, const double *Bz_dev, const double *Ctz_dev,
                            double *Y_dev, void *stream);
int cs3_cplx_sens_solve(cs3_cplx p, cs3_handle h, cs3_cplx_sens s, const double *Bz, const double *Ctz, double *Y);
int cs3_debug_cplx_sens_parts(cs3_cplx p, cs3_handle h, cs3_cplx_sens s, int64_t parts, const double *Bz_dev,
                              const double *Ctz_dev, double *Y_dev, void *stream);

/* ---- complex low-rank-modified systems (Y + dY_c) v = i on the held factors -
 * Branch-outage, fault and switching studies on an admittance matrix: cs3_updates_* (above) for a complex matrix behind
 * a complex plan, on the factors its real-form handle holds.  ONE complex solved-for column is ONE real column of the
 * tile Z [2n, t], real part in rows 2i, imaginary part in rows 2i + 1: the unit right-hand side pack_N(e_row) is
 * (Re s_row, Im s_row) in the pair of that row, so Z = A^-1 E_R comes out of the handle's unchanged many-right-hand-side
 * solve.  dA_c is never rotated, s never leaves the device, a case may touch 16 complex rows and 16 complex columns, and a
 * tile of 1024 columns holds 1024 buses.
 *
 * Case c is a sparse complex dA_c given as triplets (i, j, v); duplicates of one (i, j) inside a case ADD, in triplet
 * order, component by component, starting from +0.  R_c (r <= 16) its distinct rows ascending, C_c (s <= 16) its distinct
 * columns ascending, D_c the dense r x s block, x0 = A^-1 b, Z = A^-1 E_R:
 *     G_c = Z[C_c, R_c]   S_c = I_r + D_c G_c   y_c = S_c^-1 (D_c x0[C_c])   x_c = x0 - Z[:, R_c] y_c
 * ARITHMETIC, on separate real and imaginary parts, fp contraction off, no atomics:
 *   product   a b = (ar br - ai bi, ar bi + ai br): four rounded products, then the two sums
 *   quotient  a / b: den = br br + bi bi;  ((ar br + ai bi) / den, (ai br - ar bi) / den)
 *   S_c[i, k] starts at (1, +0) on the diagonal and (+0, +0) off it and adds the products D[i, a] G[a, k] over ascending
 *   a, each component on its own; the right-hand side starts at (+0, +0) and adds D[i, a] x0[C_a] likewise.
 *   Elimination by rows with partial pivoting on LAPACK's complex measure cabs1(z) = |Re z| + |Im z| (izamax): the
 *   largest candidate of rows k .. r - 1 of column k, ties to the lowest row, a NaN above every number; the rows are
 *   swapped with their right-hand side entry; l = S[i, k] / pivot (quotient), S[i, j] -= l S[k, j] (product, then the
 *   two differences) for j > k and the right-hand side.  Back substitution from the last row: y_k = rhs_k / S[k, k]
 *   (quotient), rhs_i -= S[i, k] y_k for i < k.
 *   x_c[i] = x0[i] minus the products Z[i, R_j] y_j over ascending j, each component on its own.
 * rpiv[c] = min_k cabs1(pivot_k) / max(1, max cabs1(S_c)); 1.0 for an empty case, NaN when a NaN is met.  A case is
 * flagged on an exactly zero pivot column, on rpiv[c] <= sing_tol when sing_tol > 0, or on a NaN: its column of X is
 * filled with (NaN, NaN); the other cases of the call are unaffected.  An empty case returns, bit for bit, what pack_N, the
 * handle's solve and unpack_N give for b.  Only op N is built.
 *
 * Complex arrays (cz, b, X [n, ncases] row-major) are interleaved, typed double *, and aligned to 16 bytes on the device.
 * cs3_cplx_updates_plan: host, pattern only, needs no GPU; indices are those of the COMPLEX matrix.  Cases and tiles are
 *   exactly those cs3_updates_plan builds for the same lists with n = the complex order (CS3_UPD_TILE is read by this call
 *   too).  Checks, in this order, each CS3_ERR_ARG: null pointers; a handle whose order is not 2 n of the plan;
 *   ncases < 1; cp not monotone (from 0); null index arrays when there are triplets; an index outside [0, n); a case with
 *   more than 16 distinct rows or columns (the message names the case); a plan or handle with batch > 1; a plan or handle
 *   with a border (Schur).
 * cs3_cplx_updates_info, cs3_debug_cplx_updates_tiles: as cs3_updates_info, cs3_debug_updates_tiles.
 * cs3_cplx_updates_limits: the constants that shape the kernels; needs no GPU.
 * cs3_cplx_updates_solve_dev: cz_dev[cp[ncases]] the values in the plan's triplet order; b_dev[n]; X_dev [n, ncases];
 *   rpiv_dev[ncases] real, may be NULL.  Asynchronous on `stream`; s is read from the plan as it stands in stream order.
 *   Checks: null arguments, a plan made for another handle or another complex plan, misaligned arrays: CS3_ERR_ARG; no
 *   successful factorisation: CS3_ERR_STATE.  LU (rotated or not) and Cholesky handles both work; dA_c need not be
 *   Hermitian.  Workspace: the handle's tile buffer (the one cs3_sens_* use), 2 n x 1024 doubles at most, 2 n doubles of
 *   x0, a few hundred bytes per case on the plan, allocated by the first call; later calls neither allocate nor
 *   synchronise.
 * cs3_cplx_updates_solve: the same from host arrays (synchronises); the same bits.
 * cs3_debug_cplx_updates_parts: the steps selected by the mask `parts` (1: x0 and the unit right-hand sides, 2: the
 *   tiles' solves, 4: capacitance and apply), for tests.
 * A plan survives refactorisations (the new s is picked up).  Plans and handle may be freed in either order, as for
 * cs3_updates_plan.
 * Out of scope: ops T and H; batched and Schur handles; several base right-hand sides per call; more than 16 distinct
 * rows or columns; exploiting the sparsity of the unit columns in the sweeps; the CscMat sugar (CscMat.solve_modified
 * refuses complex data, and a test pins that refusal). */
typedef struct cs3_cplx_updates_s *cs3_cplx_updates;
typedef struct cs3_cplx_updates_limits_t {
    int64_t unit_rows, unit_threads;        /* k_cupd_units: complex rows per workgroup, its threads */
    int64_t apply_stage, apply_rows;        /* k_cupd_apply: complex rows of Z in LDS at a time, complex rows per workgroup */
    int64_t apply_threads_min;              /*   ... and the threads of its smallest workgroup */
    int64_t max_rank, max_tile, max_tile_cases;
} cs3_cplx_updates_limits_t;
int cs3_cplx_updates_limits(cs3_cplx_updates_limits_t *out);
int cs3_cplx_updates_plan(cs3_cplx p, cs3_handle h, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj,
                          cs3_cplx_updates *out);
int cs3_cplx_updates_free(cs3_cplx_updates u);
int cs3_cplx_updates_info(cs3_cplx_updates u, int64_t *ncases, int64_t *nrows_unique, int64_t *max_rank, int64_t *ntiles);
int64_t cs3_debug_cplx_updates_tiles(cs3_cplx_updates u, int32_t *first_case, int32_t *ncases, int32_t *nrows, int32_t *width);
int cs3_cplx_updates_solve_dev(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, const double *cz_dev, const double *b_dev,
                               double sing_tol, double *X_dev, double *rpiv_dev, void *stream);
int cs3_cplx_updates_solve(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, const double *cz, const double *b,
                           double sing_tol, double *X, double *rpiv);
int cs3_debug_cplx_updates_parts(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, int64_t parts, const double *cz_dev,
                                 const double *b_dev, double sing_tol, double *X_dev, double *rpiv_dev, void *stream);

/* ---- complex Schur handles: Kron reduction of an admittance matrix ----------
 * Ward and network equivalents: S = A22 - A21 A11^-1 A12 of the complex matrix on its boundary buses, from a real Schur
 * handle (cs3_analyze_schur) on the real form:
 *     cs3_cplx_plan_create_schur(n, Ap, Ai, batch, rotate, ns, idx, &p);  cs3_cplx_plan_pattern(p, Rp, Ri);
 *     cs3_cplx_plan_schur_order(p, order, q, q2_interior, schur2);
 *     cs3_analyze_schur(kind, CS3_ORDER_GIVEN, 2 n, Rp, Ri, q2_interior, batch, 2 ns, schur2, &h);
 *     cs3_cplx_values_dev(p, Az, Rx, st);  cs3_factor_dev(h, Rx, tol, st);  cs3_cplx_schur_get_dev(p, h, S, st);
 * BORDER ROWS ARE NEVER ROTATED: their diagonal lists in the plan's tables are empty, so s_i = (1, +0) there whatever the
 * values (they count in rows_without_diagonal).  With M = diag(s) A and s = 1 on the border,
 * M22 - M21 M11^-1 M12 = A22 - A21 A11^-1 A12: S comes out in A's scaling with no division.  The border is never
 * pivoted, so it needs no rotation (a zero diagonal there is no obstacle).
 *
 * cs3_cplx_plan_create_schur: cs3_cplx_plan_create with a border.  Its checks come first, then those of cs3_analyze_schur on
 *   its set, in that order: a null schur_idx, ns < 1 or ns >= n, an index outside [0, n), a repeated index (named).
 * cs3_cplx_plan_schur_info: ns and the list (either may be NULL); a plan without a border: CS3_ERR_STATE.
 * cs3_cplx_plan_schur_order: q2_interior[2 n1], n1 = n - ns, the doubled order of the interior -- CS3_ORDER_AMD:
 *   q = interior[cs3_amd(A11)] of the complex pattern with border rows and columns removed (what cs3_analyze_schur does
 *   with a real pattern); CS3_ORDER_NATURAL: the interior ascending; CS3_ORDER_GIVEN: q_given[n1] -- doubled as
 *   cs3_cplx_plan_order doubles; schur2[2 ns] = (2 b, 2 b + 1) for every border index b in the caller's order.
 * cs3_cplx_schur_get_dev: S_dev [batch][ns, ns] complex row-major, S[i, j] = (S_R[2i, 2j], S_R[2i + 1, 2j]): the first
 *   column of every 2 x 2 block of the handle's real Schur complement (the twin column agrees to rounding only and is not
 *   read).  One launch on `stream`.  Checks: those of cs3_schur_get_dev, a plan without a border (CS3_ERR_STATE), a handle
 *   whose Schur set is not 2 ns (CS3_ERR_ARG), a misaligned S_dev.  A Cholesky plan (CS3_CPLX_ROTATE_NONE, Hermitian
 *   positive definite) gives a Hermitian S.
 * cs3_cplx_schur_get: the same into host memory (synchronises).
 * HALF-SOLVES are compositions of existing calls, on X2 [batch][2n, k] real:
 *   forward:  cs3_cplx_pack_dev(p, CS3_CPLX_N, B, X2) (s * b, s = 1 on the border); cs3_schur_fwd_dev(h, X2, k);
 *             cs3_cplx_unpack_dev(p, CS3_CPLX_N, X2, Y) (a raw join): border rows hold b2 - A21 A11^-1 b1, the interior
 *             rows are opaque.
 *   backward: the caller writes x2 into the border rows of Y; cs3_cplx_pack_dev(p, CS3_CPLX_H, Y, X2) (a raw split);
 *             cs3_schur_bwd_dev(h, X2, k); cs3_cplx_unpack_dev(p, CS3_CPLX_N, X2, X): X solves A x = b.
 * On the handle cs3_solve* stay refused, as on every Schur handle.  Out of scope: transposed half-solves; the CscMat sugar
 * (CscMat.lu(schur=...), chol(schur=...) and schur_complement refuse complex data, and a test pins those refusals). */
int cs3_cplx_plan_create_schur(int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, int64_t ns,
                               const int32_t *schur_idx, cs3_cplx *out);
int cs3_cplx_plan_schur_info(cs3_cplx p, int64_t *ns, int32_t *schur_idx);
int cs3_cplx_plan_schur_order(cs3_cplx p, int64_t order, const int32_t *q_given, int32_t *q2_interior, int32_t *schur2);
int cs3_cplx_schur_get_dev(cs3_cplx p, cs3_handle h, double *S_dev, void *stream);
int cs3_cplx_schur_get(cs3_cplx p, cs3_handle h, double *S);

/* ---- complex selected inversion: entries, diagonal and Thevenin table of Z-bus ----
 * Z = A^-1 of a complex matrix on its own pattern, from the factors the real-form handle holds: the driving-point
 * impedances diag(Z-bus) of every bus (fault levels), the transfer impedances of every branch, and the Thevenin impedance
 * Z_ii + Z_jj - Z_ij - Z_ji seen between the ends of every branch.  A composition, like the complex sections above:
 *     cs3_cplx_values_dev(p, Az, Rx, st);  cs3_factor_dev(h, Rx, tol, st);  cs3_selinv_dev(h, st);
 *     cs3_cplx_selinv_diag_dev(p, h, d, st);  cs3_cplx_selinv_thevenin_dev(p, h, T, st);
 * Computing the real selected inverse stays cs3_selinv_dev on the handle; the calls here read it.
 *
 * DEFINITIONS.  p is a complex plan of order n on the pattern (Ap, Ai), batch nb; h the handle analysed from
 * cs3_cplx_plan_pattern / cs3_cplx_plan_order, order 2 n.  ZR(a, b) is entry (a, b) of the inverse that cs3_selinv_dev(h)
 * left on the handle, in the caller's real-form labels.  s [nb][n] is the plan's rotation as it stands in stream order,
 * (1, +0) everywhere with CS3_CPLX_ROTATE_NONE.  The handle factorises the real form of M = diag(s) A, and
 * A^-1 = M^-1 diag(s).  Per matrix of the batch:
 *   Minv(i, j) = (ZR(2i, 2j), ZR(2i + 1, 2j)): the first column of the 2 x 2 block, as cs3_cplx_schur_get_dev reads S (the
 *     twin column agrees to rounding only and is not read).
 *   Z(i, j) = Minv(i, j) * s_j, by the ARITHMETIC rule above: four rounded products, then the two sums, nothing fused.
 *     The product is always made, also when s_j = (1, +0), as cs3_cplx_values_dev makes its own.
 *   entries:   Zz[e] = Z(Ai[e], j) for entry e of column j; with trans != 0, Zz[e] = Z(j, Ai[e]), rotated by s of row
 *     Ai[e] of the entry.  An entry stored twice gets the same value twice.
 *   diagonal:  d[i] = Z(i, i).
 *   Thevenin:  T[e] = ((Z(i, i) + Z(j, j)) - Z(i, j)) - Z(j, i) with i = Ai[e], in this order, component by component,
 *     every Z the rounded product above.  A diagonal entry gives whatever that formula gives.
 * All positions (2i, 2j) and (2i + 1, 2j) of stored entries and of their transposes lie in the structure of L + U, and
 * (2i + 1, 2i) does whenever row i has a stored diagonal or 2i, 2i + 1 share a supernode.  If a needed position is outside
 * the structure (only conceivable for a row without a stored diagonal), the first call that needs the maps returns
 * CS3_ERR_STATE with a message that names the complex row; nothing is read out of bounds.
 * The same factors and the same s give the same bits on every run, and a matrix of a batch the bits it gets alone.
 *
 * cs3_cplx_selinv_limits: threads per workgroup and the workgroup cap of the three kernels (one complex number per lane,
 *   grid-stride beyond block * grid_cap numbers).  Needs no device.
 * cs3_cplx_selinv_entries_dev: Zz_dev [nb][nnz] complex.  cs3_cplx_selinv_diag_dev: d_dev [nb][n] complex.
 * cs3_cplx_selinv_thevenin_dev: T_dev [nb][nnz] complex, one fused launch.
 *   Asynchronous on `stream`, one launch each; s is read in stream order, so a refactorisation through
 *   cs3_cplx_values_dev is picked up.  They need a valid ZR exactly as the real *_dev getters do.  Complex arrays are
 *   interleaved doubles, aligned to 16 bytes on the device.  The first call builds the maps (pairs of the handle's own
 *   selinv maps, and the n offsets of ZR(2i + 1, 2i)) and puts them on the device; later calls neither allocate nor
 *   synchronise.  The maps belong to the handle and go with cs3_free; plan and handle may be freed in either order.
 * cs3_cplx_selinv_entries, cs3_cplx_selinv_diag, cs3_cplx_selinv_thevenin: the same into host memory (synchronise); they
 *   compute ZR first when the handle does not hold that of the current factors.  The same bits.
 * cs3_debug_cplx_selinv_maps: for arrays that are not null, the offsets in the handle's block of Z of the pairs
 *   entry [nnz][2] = ZR(2i, 2j), ZR(2i + 1, 2j), entry_t [nnz][2] = ZR(2j, 2i), ZR(2j + 1, 2i) for every entry (i, j), and
 *   diag [n][2] = ZR(2i, 2i), ZR(2i + 1, 2i).  Checks 1 to 3 below (no output to check); from the analysis alone, needs
 *   no device and no factorisation.
 *
 * Checks, in this order, none of which needs a device: (1) a null plan, handle or output: CS3_ERR_ARG; (2) a handle
 * whose order is not 2 n of the plan, whose entry count is not 4 nnz, or whose batch differs: CS3_ERR_ARG; (3) the
 * refusals of cs3_selinv_* with their wording (Schur, matched, 128 matrices or more), so a plan with a border is refused
 * through its handle; (4) a misaligned device output: CS3_ERR_ARG; (5) no successful factorisation: CS3_ERR_STATE; (6) a
 * *_dev getter without a valid ZR: CS3_ERR_STATE.  A handle of the right sizes whose pattern is not the real form of
 * the plan's is refused when the maps are built (CS3_ERR_ARG).
 * LU handles (rotated or not) and Cholesky handles (CS3_CPLX_ROTATE_NONE, Hermitian positive definite) both work; the
 * Cholesky Z is Hermitian to rounding.
 *
 * Out of scope: complex arithmetic inside the selinv kernels (the real form does twice the work and holds Z twice);
 * entries outside the pattern of L + U; a getter on the complex factors' own pattern; op H (the conjugate of trans);
 * matched, Schur and matrix-interleaved handles; a Thevenin getter for real handles; the CscMat sugar
 * (CscMat.selected_inverse and inverse_diagonal refuse complex data, and a test pins that refusal). */
typedef struct cs3_cplx_selinv_limits_t { int64_t block, grid_cap; } cs3_cplx_selinv_limits_t;
int cs3_cplx_selinv_limits(cs3_cplx_selinv_limits_t *out);
int cs3_cplx_selinv_entries_dev(cs3_cplx p, cs3_handle h, int64_t trans, double *Zz_dev, void *stream);
int cs3_cplx_selinv_diag_dev(cs3_cplx p, cs3_handle h, double *d_dev, void *stream);
int cs3_cplx_selinv_thevenin_dev(cs3_cplx p, cs3_handle h, double *T_dev, void *stream);
int cs3_cplx_selinv_entries(cs3_cplx p, cs3_handle h, int64_t trans, double *Zz);
int cs3_cplx_selinv_diag(cs3_cplx p, cs3_handle h, double *d);
int cs3_cplx_selinv_thevenin(cs3_cplx p, cs3_handle h, double *T);
int cs3_debug_cplx_selinv_maps(cs3_cplx p, cs3_handle h, int64_t *entry, int64_t *entry_t, int64_t *diag);

/* ---- AC power flow: batched Newton from the bus admittance matrix to the voltages ----
 * The computation everything above serves ("the real power-flow inner loop"): the two steps between
 * a bus admittance matrix and the factor + solve chain -- the power mismatch and the values of the Jacobian's four blocks
 * -- as kernels, and a host driver around them, cs3_factor_solve_dev and cs3_solve_dev.  `batch` injection scenarios of
 * one network advance in lock-step, one launch chain per iteration (a time series, a Monte-Carlo study).
 *
 * Definitions.  Y is n x n complex CSC, (Yp, Yi) int32, values Yz interleaved complex128 ([y_batch][nnz_y][2] doubles).
 * Rows inside a column may be unsorted; the pattern may be one-sided (Y_ij stored, Y_ji not: a phase shifter) and the
 * values need not be symmetric; a row stored twice in one column is refused.  Bus types are two int32 lists pv[npv] and
 * pq[npq]: disjoint, in range, no repeats, in any order; every bus in neither list is a reference bus (several are
 * allowed).  pvpq = pv ++ pq, nj = npv + 2 npq.  Unknowns x = [theta(pvpq); |V|(pq)] in the order of the lists; equations
 * F = [Re mis(pvpq); Im mis(pq)] with mis = V o conj(I) - S, I = Y V, V = vm o exp(j va).  A Newton step solves J dx = -F,
 * then va[pvpq] += dx[:npv + npq], vm[pq] += dx[npv + npq:].  The Jacobian is the polar form with d/d|V| (not |V| d/d|V|);
 * with Vn = V / |V|:
 *   i != j:  dS_i/dtheta_j = -j V_i conj(Y_ij V_j),        dS_i/d|V|_j = V_i conj(Y_ij Vn_j)
 *            dS_i/dtheta_i =  j V_i conj(I_i - Y_ii V_i),  dS_i/d|V|_i = V_i conj(Y_ii Vn_i) + conj(I_i) Vn_i
 *   H = Re dS/dtheta on [pvpq, pvpq], N = Re dS/d|V| on [pvpq, pq], M = Im dS/dtheta on [pq, pvpq], L = Im dS/d|V| on
 *   [pq, pq], placed as [[H, N], [M, L]] the way pack_4_by_4 places them (cs3_csc_stack_4_by_4).  One stored entry of Y
 *   yields at most four entries of J, and J has exactly those: column c of J comes from column pvpq[c] (c < npv + npq) or
 *   pq[c - npv - npq] of Y and lists its top-block entries in the storage order of that column, then its bottom-block
 *   entries in the same order.
 * S [batch][n] complex, vm and va [batch][n].  The entries of S at reference buses, and the imaginary parts at PV buses,
 * are never read and may hold anything, NaN included.
 *
 * cs3_pf_plan_create: host work only, O(nnz_y + n) plus cs3_analyze of the Jacobian; no device is needed until the first
 *   device call (like union plans).  y_batch is 1 (one Y for all scenarios) or batch (one per scenario); order is
 *   CS3_ORDER_NATURAL or CS3_ORDER_AMD.  Checked in this order, each failure CS3_ERR_ARG with a message: null pointers;
 *   a bad pattern, by the checks of cs3_union_plan_create (n outside [0, 2^30), Yp[0] != 0, a decreasing Yp, null Yi with
 *   entries, a row outside [0, n), 2^29 - 256 entries or more); batch < 1, y_batch neither 1 nor batch, a bad order; a bus
 *   list of bad length, out of range, with repeats, or not disjoint from the other; npv + npq = 0; a row stored twice in
 *   a column; a pv or pq bus without a stored diagonal entry.
 *   It builds the pattern (Jp, Ji); the map jpos[4][nnz_y] (H, N, M, L; struct-of-arrays; -1 where a bus type removes
 *   the entry); Y by rows -- per row the entries in ascending column with their positions in Yz: no transposed copy of
 *   values is ever made; and the unknown behind every bus.
 * cs3_pf_handle: the plan OWNS an ordinary batched LU handle on (Jp, Ji) and lends it out: cs3_set_pivot_perturbation,
 *   cs3_condest, cs3_slogdet, cs3_selinv_dev, cs3_sens_plan and the rest work on the Jacobian of the last factorisation
 *   with no new code.  It is freed with the plan: never pass it to cs3_free, never use it after cs3_pf_plan_free.
 * cs3_pf_plan_info; cs3_pf_plan_pattern: Jp[nj + 1], Ji[nnz_j]; cs3_pf_plan_maps: jpos[4 * nnz_y], Rp[n + 1], Rj[nnz_y],
 *   Rpos[nnz_y], upos_a[n] (the unknown behind theta_i, -1: none), upos_m[n] (behind |V|_i); any output may be NULL.
 * cs3_pf_limits: the constants that shape the launches; needs no device.
 *
 * Kernels (powerflow.hip).  k_pf_mismatch: one lane per bus row, one wave per row of more than wave_row entries (lane l
 * sums entries l, l + 64, ... in order, then a fixed butterfly); reference rows are skipped.  It writes -F into the
 * right-hand side [batch][nj] and I for the next kernel, and per scenario max |F| over the monitored entries by a wave
 * reduction and an INTEGER atomic max on the bit pattern of the non-negative double -- order-independent, the same bits on
 * every run; no float atomics.  A NaN orders above infinity there, so "not finite" is that maximum's exponent field all
 * ones.  k_pf_jacobian: one lane per stored entry of Y, grid-stride past grid_cap workgroups per scenario; up to four
 * values through jpos into Jx [batch][nnz_j]; a scenario that is no longer active gets the identity (1 at the diagonal
 * positions of H and L, 0 elsewhere), whose factorisation is harmless.  k_pf_decide: one workgroup per scenario freezes
 * it when its iteration ends and counts the active scenarios down.  k_pf_update: applies dx to the scenarios still active,
 * and to none when the handle's status word reports a failed factorisation.
 *
 * cs3_pf_solve_dev.  Iteration it = 0, 1, ...: (1) the mismatch; (2) per scenario: not finite -> flag 2; norm <= tol ->
 * flag 0; it == max_iters -> flag 1; each with iters = it, and each makes the scenario inactive and FROZEN: its right-hand
 * side is 0 and vm, va are untouched from then on, bit for bit; (3) stop when no scenario is active; (4) when
 * it % refactor_every == 0 the Jacobian and cs3_factor_solve_dev on the plan's handle with pivot_tol, else cs3_solve_dev on
 * the held factors (dishonest Newton); (5) the update.  iters, norm (the norm at the iteration where the scenario stopped)
 * and flag are HOST arrays [batch]; any may be NULL.
 *   Not converging is not an error: CS3_OK, and flag tells.  vm, va of a scenario flagged 2 are unspecified; the other
 *   scenarios are unaffected.  A rejected pivot in an active scenario ends the call with CS3_ERR_PIVOT (the handle keeps
 *   ONE status word per batch; per-member status is not built); vm, va are then as the last completed update left them.
 *   With cs3_set_pivot_perturbation on the lent handle nothing fails.  max_iters = 0 evaluates the mismatch only.
 *   HOST INVOLVEMENT: the call is host-driven, as cs3_gmres_dev is.  In every iteration, after step 2, it reads one 4-byte
 *   "scenarios still active" word and the handle's status word of the factorisation before, which synchronises `stream`.
 *   It cannot be captured into a graph.
 *   Checks, in this order, all CS3_ERR_ARG before any device work: null plan or arrays, tol negative or not finite,
 *   max_iters < 0, refactor_every < 1.  CS3_ERR_HIP without a device.  CS3_ERR_STATE when the handle reports that a
 *   hand-over between the waves of a shared elimination timed out (as cs3_factor_status does): no update was applied for
 *   that factorisation, and the factors are not valid.
 *   ONE CALL AT A TIME PER PLAN: the right-hand side, the Jacobian values, the currents I and the per-scenario state live
 *   in the plan, so two calls on one plan must not overlap -- not from two host threads, and not on two streams.  The
 *   same holds for cs3_pf_mismatch_dev and cs3_pf_jacobian_dev, which write the plan's current buffer.
 * cs3_pf_mismatch_dev: -F in unknown order into F_dev [batch][nj] and max |F| into norm_dev [batch] (may be NULL; 8-byte
 *   aligned; it is cleared on `stream` first), every scenario active.  cs3_pf_jacobian_dev: Jx_dev [batch][nnz_j] at the
 *   given voltages (it runs the currents' pass of the mismatch kernel first: two launches).  Both asynchronous; users build
 *   their own Newton variants (Q-limit switching) around them: mismatch_dev -> jacobian_dev -> cs3_factor_solve_dev on the
 *   lent handle gives the bits of the driver.
 * cs3_pf_mismatch, cs3_pf_jacobian, cs3_pf_solve: the host-array forms (the null stream): the same kernels in the same
 *   order, the same bits.
 * Not offered: bus-type switching inside the call (a changed pv / pq split is a new plan); fast-decoupled or DC variants;
 * a rectangular or current-injection formulation; per-member pivot status; a graph-capturable fixed-length form; sharding;
 * a matched handle for the Jacobian. */
typedef struct cs3_pf_s *cs3_pf;
typedef struct cs3_pf_info {
    int64_t n, nnz_y, npv, npq, nref, nj, nnz_j, batch, y_batch;
    int64_t rows_lane, rows_wave;  /* non-reference rows of Y summed by one lane / by a wave */
    int64_t max_row;               /* stored entries of the longest non-reference row */
} cs3_pf_info;
typedef struct cs3_pf_limits_t {
    int64_t block;                 /* threads of a workgroup */
    int64_t grid_cap;              /* most workgroups per scenario: beyond grid_cap * block rows or entries a lane loops */
    int64_t wave_row;              /* a row with more stored entries than this is summed by a wave */
} cs3_pf_limits_t;
int cs3_pf_limits(cs3_pf_limits_t *out);
int cs3_pf_plan_create(int64_t n, const int32_t *Yp, const int32_t *Yi, int64_t npv, const int32_t *pv, int64_t npq,
                       const int32_t *pq, int64_t batch, int64_t y_batch, int64_t order, cs3_pf *out);
int cs3_pf_plan_free(cs3_pf p);
int cs3_pf_handle(cs3_pf p, cs3_handle *h);
int cs3_pf_plan_info(cs3_pf p, cs3_pf_info *info);
int cs3_pf_plan_pattern(cs3_pf p, int32_t *Jp, int32_t *Ji);
int cs3_pf_plan_maps(cs3_pf p, int32_t *jpos, int32_t *Rp, int32_t *Rj, int32_t *Rpos, int32_t *upos_a, int32_t *upos_m);
int cs3_pf_mismatch_dev(cs3_pf p, const double *Yz_dev, const double *S_dev, const double *vm_dev, const double *va_dev,
                        double *F_dev, double *norm_dev, void *stream);
int cs3_pf_jacobian_dev(cs3_pf p, const double *Yz_dev, const double *vm_dev, const double *va_dev, double *Jx_dev, void *stream);
int cs3_pf_solve_dev(cs3_pf p, const double *Yz_dev, const double *S_dev, double *vm_dev, double *va_dev, double tol,
                     int64_t max_iters, int64_t refactor_every, double pivot_tol, int32_t *iters, double *norm, int32_t *flag,
                     void *stream);
int cs3_pf_mismatch(cs3_pf p, const double *Yz, const double *S, const double *vm, const double *va, double *F, double *norm);
int cs3_pf_jacobian(cs3_pf p, const double *Yz, const double *vm, const double *va, double *Jx);
int cs3_pf_solve(cs3_pf p, const double *Yz, const double *S, double *vm, double *va, double tol, int64_t max_iters,
                 int64_t refactor_every, double pivot_tol, int32_t *iters, double *norm, int32_t *flag);

/* ---- AC state estimation: weighted least squares, Gauss-Newton from measurements to the voltages ----
 * The estimator that the power flow, the contingency screens and the Z-bus tools start from: it joins three subsystems
 * that exist above -- the sparse product on a fixed pattern (the gain matrix G = H' (W H)), a Cholesky handle that factorises
 * and solves in one graph, and the normalised residuals on the selected inverse -- by the kernels that were missing between
 * them: the AC measurement functions h(x), the measurement Jacobian H(x), the gradient H' W r and the update.
 *     minimise J(x) = sum_i w_i (z_i - h_i(x))^2;   an iteration solves  (H' W H) dx = H' W r,  r = z - h(x),  x += dx.
 *
 * Network.  Y is n x n complex CSC, (Yp, Yi) int32, values Yz interleaved complex128 ([nnz_y][2] doubles), by the rules of
 * the power-flow plan: rows inside a column may be unsorted, the pattern may be one-sided, a row stored twice in a column
 * is refused.
 * Branch ends.  end_from[ne], end_to[ne] (int32 buses, from != to) with values Ye [ne][2] complex = (yff, yft) as four
 * doubles: the flow at end k is Sf_k = V_f conj(yff V_f + yft V_t).  The "to" end of a branch is simply another entry
 * with the buses swapped; ne = 0 is allowed (Ye may then be NULL).
 * State.  ref[nref], nref >= 1, lists the buses whose angle is fixed.  x = [va(non-reference buses, ascending bus);
 * vm(all buses, ascending)], ns = 2 n - nref, the first na = n - nref states are the angles.
 * Measurements.  m rows in the caller's order, kind[m] and where[m] (int32):
 *     kind 0  |V| at bus where          kind 1  Re S_i, bus where        kind 2  Im S_i, bus where
 *     kind 3  Re Sf_k, branch end where kind 4  Im Sf_k, branch end where
 * with S_i = V_i conj((Y V)_i), the power-flow convention.  Rows may repeat (the same quantity measured twice is two rows).
 * z[m] and the weights w[m] (positive, finite) are values given at solve time.
 * Derivatives.  Polar form with d/d|V| (not |V| d/d|V|).  Injections: the formulas of the power-flow section.  For an end k
 * with I_k = yff V_f + yft V_t and Vn = V / |V|:
 *     dSf/dtheta_f =  j V_f conj(yft V_t)        dSf/d|V|_f = V_f conj(yff Vn_f) + conj(I_k) Vn_f
 *     dSf/dtheta_t = -j V_f conj(yft V_t)        dSf/d|V|_t = V_f conj(yft Vn_t)
 * A kind-0 row has the single entry 1.  Entries in the angle column of a reference bus do not exist.
 * Pattern of H (m x ns), fixed by the plan.  Row i lists its angle entries first, then its magnitude entries; an injection
 * row in ascending column of row where[i] of Y (the order of Rj below), a flow row `from` before `to`.  The plan holds H by
 * rows (Rp[m + 1], Rj[nnz_h]: what cs3_quad_plan takes as Ct) and in CSC (Hp[ns + 1], Hi[nnz_h]; inside a column the
 * entries are in ascending measurement row), with cpos[nnz_h] mapping a row-order entry to its CSC position.
 *
 * cs3_se_plan_create: host work only, O(nnz_y + n + ne + nnz_h); needs no device.  order is CS3_ORDER_NATURAL or
 *   CS3_ORDER_AMD and is used for the gain matrix later.  Checked in this order, each failure CS3_ERR_ARG with a message:
 *   (1) null pointers; (2) the pattern checks of cs3_pf_plan_create (n outside [0, 2^30), Yp[0] != 0, a decreasing Yp, null
 *   Yi with entries, a row outside [0, n), 2^29 - 256 entries or more), a bad order, a row stored twice in a column;
 *   (3) nref < 1, a ref out of range or repeated; (4) a bad ne, an end out of range or with from == to; (5) m < 1 or m > 2^31 - 1; (6) a
 *   kind outside 0..4; (7) a where out of range for its kind; (8) a kind-1 or kind-2 row at a bus with no stored diagonal
 *   entry; (9) 2^29 - 256 entries of H or more.
 *   It builds Y by rows (ascending column, with the position in Yz behind every entry: no transposed values), the two forms
 *   of H with cpos, per row-order entry the descriptor k_se_jacobian reads (measurement, position in Yz or branch end, which
 *   derivative, diagonal / from-side or not, the bus of the state), and the lists of rows of Y longer than wave_row and of
 *   columns of H longer than wave_col.
 * cs3_se_plan_info: the sizes; nkind[5] the rows per kind; max_row the longest row of Y (the currents are computed at every
 *   bus); max_col the longest column of H; rows_wave, cols_wave the lengths of the two lists; nnz_g the entries of the gain
 *   matrix, 0 until the solver has been built.
 * cs3_se_plan_pattern: Hp[ns + 1], Hi[nnz_h], Rp[m + 1], Rj[nnz_h].  cs3_se_plan_maps: cpos[nnz_h], upos_a[n] (the state
 *   behind theta_i, -1 at a reference bus), upos_m[n] (behind |V|_i).  Any output may be NULL.
 * cs3_se_limits: block, grid_cap, wave_row, wave_col; needs no device.
 *
 * THE SOLVER is built once, by the first call of cs3_se_solve*, cs3_se_baddata*, cs3_se_handle or cs3_se_gain_pattern
 * (cs3_spgemm_plan_create needs the device, which is why cs3_se_plan_create does not do it): the cs3_spgemm plan H' (W H)
 * (transpose_a = 1, both operands on H's CSC pattern), a CS3_CHOLESKY handle on the product's pattern (batch 1, the
 * plan's order), a cs3_quadplan on that handle from H by rows.  A refusal of the analysis (32-bit pool offsets) comes back
 * as that call's error with its message; the next such call tries again.
 * cs3_se_handle lends the Cholesky handle out under the rules of cs3_pf_handle: cs3_condest, cs3_slogdet, cs3_selinv_dev,
 *   cs3_quad_plan and the rest work on the gain matrix of the last factorisation; it is freed with the plan: never pass it
 *   to cs3_free, never use it after cs3_se_plan_free.  cs3_se_gain_pattern: Gp[ns + 1], Gi[nnz_g] (rows unsorted: the
 *   order of cs3_spgemm).
 *
 * Kernels (stateest.hip).  k_se_currents: I = Y V for every bus, one lane per row, one wave for a row of more than wave_row
 *   stored entries (lane l takes entries l, l + 64, ... in order, then a fixed butterfly); it keeps (cos, sin) of every
 *   bus angle beside the current, so no later kernel evaluates sincos.  The row sums themselves evaluate sincos of the
 *   column's angle at every stored entry of Y, as k_pf_mismatch does: nnz_y + n calls per pass, not n.  k_se_residual: one lane per measurement: r_i, w_i
 *   r_i, and per workgroup the partial of sum w_i (r_i r_i) by a fixed tree over rows 256 g + j; k_se_close, one workgroup:
 *   thread j takes the partials j, j + 256, ... in order, then the same tree -- the scheme of cs3_quad_normres; no atomics,
 *   the same bits on every run.  k_se_jacobian: one lane per row-order entry of H, grid-stride past grid_cap workgroups; up
 *   to three stores: Hr[q], Hc[cpos[q]], WHc[cpos[q]] = w_i H_ij (one rounding).  k_se_gradient: one lane per column of H in
 *   CSC, one wave for a column of more than wave_col entries (strided as above, then lane l += lane l + off, off = 32 .. 1):
 *   g_j = sum Hc * (w r) in stored order, every product and every sum rounded on its own -- defined to the bit.
 *   k_se_update: applies dx, records max |dx| by a wave reduction and an INTEGER atomic max on the bit pattern of the
 *   non-negative double (NaN above infinity; the power flow's device), and applies nothing when the handle's status word
 *   reports a failed factorisation.
 *
 * cs3_se_measure_dev: r = z - h(x) into r_dev [m] and J = sum w r^2 into J_dev [1]; either may be NULL.  Two launches
 *   (three with J).  It also refreshes the residuals the plan keeps.
 * cs3_se_jacobian_dev: H by rows into Hr_dev, in CSC into Hc_dev, w_i H_ij in CSC into WHc_dev [nnz_h]; any may be NULL
 *   (w_dev may be NULL when WHc_dev is).  Two launches.
 * cs3_se_gradient_dev: g_dev [ns] = H' (w r) from Hc_dev [nnz_h] and wr_dev [m].  One launch.
 *   These three need only the plan's tables: no spgemm plan and no handle.  All asynchronous on `stream`.
 * cs3_se_residuals_dev: borrowed device pointers to the plan's r [m] and w r [m] of the last residual pass (cs3_se_measure_dev,
 *   cs3_se_solve*, cs3_se_baddata*); valid until the plan is freed.
 * cs3_se_solve_dev.  Iteration it = 0, 1, ... while it < max_iters: (1) currents + residuals; (2) the Jacobian values;
 *   (3) the gradient g = H' (w o r) into the right-hand side; (4) cs3_spgemm_values_dev; (5) cs3_factor_solve_dev on the
 *   handle (k = 1, tol 0); (6) the update va[non-ref] += dx[:na], vm += dx[na:] with max |dx|.  Five launches of
 *   stateest.hip per iteration beside the product's two and the factor + solve graph.  Then the host reads max |dx| and the
 *   handle's status word -- the ONE synchronisation per iteration, as in cs3_pf_solve_dev, so the call cannot be captured
 *   into a graph.  iters = it + 1; flag 2 if max |dx| is not finite, else flag 0 if it is <= tol, else flag 1 if iters ==
 *   max_iters, else the next iteration.  On exit one more residual pass, so that J and the residuals kept in the plan
 *   belong to the returned state.  max_iters = 0 evaluates r and J only: iters 0, step 0, flag 1, no voltage changes.
 *   iters, step (the last max |dx|), J and flag are HOST scalars; any may be NULL.
 *   A non-positive pivot returns CS3_ERR_NOT_SPD: an unobservable state; vm, va are as the last completed update left
 *   them (k_se_update applied nothing), iters and step are those of the completed iterations (0 and 0 when the first one
 *   fails), flag is 1 and J is not written.  Any other error return writes none of the four.  Not converging is CS3_OK plus the flag; vm, va after flag 2 are unspecified.
 *   Checks, in this order, all CS3_ERR_ARG before any device work: null plan or arrays; tol negative or not finite;
 *   max_iters < 0.  CS3_ERR_HIP without a device.
 *   ONE CALL AT A TIME PER PLAN: the currents, the residuals, H, G and the right-hand side live in the plan, so two calls on
 *   one plan must not overlap -- not from two host threads, and not on two streams; cs3_se_measure_dev and
 *   cs3_se_jacobian_dev, which write the plan's current buffer, included.
 * cs3_se_baddata_dev, at the given voltages: residuals; Jacobian; gain values; cs3_factor_dev; cs3_selinv_dev;
 *   cs3_quad_normres_dev with Hr, w, r.  t_dev, omega_dev, rn_dev [m] (any may be NULL) and summary_dev [4] are exactly
 *   those of cs3_quad_normres_dev.  Asynchronous; the status of the factorisation is deferred (cs3_factor_status on the
 *   lent handle).
 * cs3_se_measure, cs3_se_jacobian, cs3_se_solve, cs3_se_baddata: the host-array forms (the null stream): the same kernels
 *   in the same order, the same bits.  cs3_se_baddata reports a failed factorisation as its return code.
 * Not offered: batches of snapshots; equality constraints or zero-injection handling other than a large weight;
 * current-magnitude, PMU or tap measurements; removing a bad row and estimating again inside the call; observability
 * analysis beyond the failed pivot; an LU or matched handle for G; sharding. */
typedef struct cs3_se_s *cs3_se;
typedef struct cs3_se_info {
    int64_t n, nnz_y, nref, na, ns, ne, m, nnz_h;
    int64_t nkind[5];              /* rows of kind 0 .. 4 */
    int64_t max_row;               /* stored entries of the longest row of Y */
    int64_t max_col;               /* entries of the longest column of H */
    int64_t rows_wave, cols_wave;  /* rows of Y / columns of H summed by a wave */
    int64_t nnz_g;                 /* entries of the gain matrix; 0 until the solver has been built */
} cs3_se_info;
typedef struct cs3_se_limits_t {
    int64_t block;                 /* threads of a workgroup */
    int64_t grid_cap;              /* most workgroups of the entry kernel: beyond grid_cap * block entries a lane loops */
    int64_t wave_row;              /* a row of Y with more stored entries than this is summed by a wave */
    int64_t wave_col;              /* a column of H with more entries than this is summed by a wave */
} cs3_se_limits_t;
int cs3_se_limits(cs3_se_limits_t *out);
int cs3_se_plan_create(int64_t n, const int32_t *Yp, const int32_t *Yi, int64_t nref, const int32_t *ref, int64_t ne,
                       const int32_t *end_from, const int32_t *end_to, int64_t m, const int32_t *kind, const int32_t *where,
                       int64_t order, cs3_se *out);
int cs3_se_plan_free(cs3_se p);
int cs3_se_plan_info(cs3_se p, cs3_se_info *info);
int cs3_se_plan_pattern(cs3_se p, int32_t *Hp, int32_t *Hi, int32_t *Rp, int32_t *Rj);
int cs3_se_plan_maps(cs3_se p, int32_t *cpos, int32_t *upos_a, int32_t *upos_m);
int cs3_se_handle(cs3_se p, cs3_handle *h);
int cs3_se_gain_pattern(cs3_se p, int32_t *Gp, int32_t *Gi);
int cs3_se_residuals_dev(cs3_se p, const double **r_dev, const double **wr_dev);
int cs3_se_measure_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev,
                       const double *vm_dev, const double *va_dev, double *r_dev, double *J_dev, void *stream);
int cs3_se_jacobian_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *w_dev, const double *vm_dev,
                        const double *va_dev, double *Hr_dev, double *Hc_dev, double *WHc_dev, void *stream);
int cs3_se_gradient_dev(cs3_se p, const double *Hc_dev, const double *wr_dev, double *g_dev, void *stream);
int cs3_se_solve_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev, double *vm_dev,
                     double *va_dev, double tol, int64_t max_iters, int32_t *iters, double *step, double *J, int32_t *flag, void *stream);
int cs3_se_baddata_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev,
                       const double *vm_dev, const double *va_dev, double crit_tol, double *t_dev, double *omega_dev, double *rn_dev,
                       double *summary_dev, void *stream);
int cs3_se_measure(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, const double *vm, const double *va,
                   double *r, double *J);
int cs3_se_jacobian(cs3_se p, const double *Yz, const double *Ye, const double *w, const double *vm, const double *va, double *Hr,
                    double *Hc, double *WHc);
int cs3_se_solve(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, double *vm, double *va, double tol,
                 int64_t max_iters, int32_t *iters, double *step, double *J, int32_t *flag);
int cs3_se_baddata(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, const double *vm, const double *va,
                   double crit_tol, double *t, double *omega, double *rn, double *summary);

#ifdef __cplusplus
}
#endif
#endif
