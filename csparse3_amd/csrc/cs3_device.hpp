// Device-side descriptors shared by kernels.hip and api.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <type_traits>
#include <vector>

#include "cs3_internal.hpp"

namespace cs3 {

// One front (supernode) as the factorisation kernels see it, stored in SCHEDULE order
// so that block b of a launch group reads entry first + b with no indirection.
struct FrontDesc {
    long long lpan, upan, cb;     // pool offsets: L panel (ld r), U panel, contribution block
    long long a_begin;            // first of its entries of A in fa_tgt / fa_src (FC_IL fronts: first pair in ila_pairs)
    long long dbuf;               // big fronts: parked diagonal blocks, BIG_NB^2 doubles per block step
    int a_count;                  // ... and how many
    int ch_begin, ch_count;       // its children in ch_tab (4 ints each)
    int c0, r, w;
    int cb_ld, u_sk, u_sj;
    int parent;
};

// Doubles allocated past the end of the factor pool.  Nothing relies on them: every load in kernels.hip goes through
// load_if or an explicit bound (audited in round 2: all base pointers are front buffers, the two call sites whose base
// depends on a right-hand-side slot clamp the slot, the lane = right-hand-side sweeps predicate i < r && k < w).  Kept
// as a margin, not as part of any kernel's contract.
constexpr size_t POOL_SLACK = 2048;

// Fused permutations (many right-hand sides): the forward sweep takes row k of the permuted right-hand sides from
// src[q[k]], the backward sweep writes solution row k to dst[q[k]] as well; null pointers = off (X holds pivot order).
struct XMap {
    const double *src = nullptr;
    double *dst = nullptr;
    const int *q = nullptr;
};

// What the solve kernels read per front, in SOLVE-schedule order.
struct SolveDesc {
    long long lpan, upan, cv, st, fasm_begin;
    long long bv;                 // SK_BIG fronts: offset of the full front vector in bigv
    long long gv, dinv;           // fronts of order > 64: first row in the gv buffer, offset of the inverted diagonal blocks
    long long rl_begin;           // what the children add to the front vector: SK_IL fronts, first (target, source) pair in rl_pairs
    int rl_count;                 //   and the number of pairs (a multiple of 16); other fronts, first entry in sl_src and the
                                  //   number of slot rounds (a round = 16 ceil(r / 16) sources, -1 = none)
    int fasm_count;
    int c0, r, w;
    int u_sk, u_sj;               // U(k, j) = pool[upan + k*u_sk + (j-w)*u_sj]
    int parent;
};

// Everything the kernels read, resident in HBM for the life of the handle.
struct DeviceFactor {
    int kind = CS3_LU;
    long long n = 0, nnz_a = 0, batch = 1;
    long long vals_size = 0, pool_size = 0, cv_size = 0;
    long long big_begin = 0;      // big-front buffers: pool[big_begin, vals_size), zeroed per factorisation
    bool zero_big = true;         //   ... by the prologue, unless every big front runs in k_front_wg (which zeroes its own)
    FrontDesc *fdesc = nullptr;
    int *st_idx = nullptr;        // row structures (backward sweep: rows of the ancestors)
    int *fa_tgt = nullptr, *fa_src = nullptr, *ch_tab = nullptr, *rel_idx = nullptr;   // assembly: entries of A, children tables, row maps
    SolveDesc *sdesc = nullptr;
    SolveDesc *sdesc1 = nullptr;  // one right-hand side with a bottom forest: descriptors in the order of Symbolic::ssched1
    // bottom forest (cs3_internal.hpp): tasks, their fronts and lists; axf = the values of A in the order of sub_a_tgt
    SubForest sub_forest;
    SubTask *sub_tasks = nullptr;
    SubFront *sub_fronts = nullptr;
    int *sub_lvl = nullptr, *sub_rel = nullptr, *sub_st = nullptr, *sub_child = nullptr, *sub_a_tgt = nullptr, *sub_a_src = nullptr;
    double *axf = nullptr;        // [batch][n_sub_a]
    long long n_sub_a = 0;
    int *fasm_src = nullptr, *fasm_tgt = nullptr, *flong_src = nullptr;
    int *rl_pairs = nullptr, *sl_src = nullptr;
    int *q = nullptr;             // [n] pivot order
    double *ax = nullptr;         // [batch][nnz_a] values of A (stable address for the graph)
    double *pool = nullptr;       // the allocation: [groups][il_len][64] interleaved block, then [batch][pm_stride]
    // What the kernels see.  A pool offset `off` is VIRTUAL: off < il_len lives in the matrix-interleaved block
    // (entry off of matrix m at pool_il[(m / 64) * 64 * il_len + off * 64 + m % 64]), anything else at
    // pool_pm[m * pm_stride + off] -- pool_pm is shifted by -il_len so that virtual offsets index it directly.
    double *pool_il = nullptr, *pool_pm = nullptr;
    long long il_len = 0, pm_stride = 0, ngroups = 1;
    int *ila_pairs = nullptr;     // assembly pairs of the FC_IL fronts
    double *dbuf = nullptr;       // [batch][dbuf_size] diagonal blocks of the big fronts in flight
    long long dbuf_size = 0;
    double *cv = nullptr;         // [batch][cv_size * nrhs_cap]
    double *xp = nullptr;         // [batch][n * nrhs_cap] right-hand sides in pivot order
    double *bigv = nullptr;       // [batch][nrhs_cap][bv_size] front vectors of the wide big fronts
    long long bv_size = 0;
    double *gv = nullptr;         // [batch][gv_size][nrhs_cap] front vectors of the GEMM sweeps, row-major [row][rhs]
    double *dinv = nullptr;       // [batch][dinv_size] inverted 64 x 64 diagonal blocks of the fronts of order > 64
    long long gv_size = 0, dinv_size = 0;
    int *inv_tasks = nullptr;     // (position in the solve schedule, chunk) pairs
    int n_inv_tasks = 0;
    std::vector<int> inv_tasks_host;
    long long nrhs_cap = 0;
    int *status = nullptr;        // [0] first failing pivot column, 0x7f7f7f7f when clean; [3]: a hand-over between waves timed out;
                                  // [4 + b]: pivots of matrix b that the perturbation replaced (PivotCtl::count)
    long long *tbuf = nullptr;    // diagnostics (CS3_PROFILE=1): 8 shader-clock stamps per front, schedule order
    bool tbuf_diag = false;       //   CS3_PROFILE=2: the same, with k_big_step stamping its diagonal tile instead of tile (1, 0)
    // Schur handle (cs3_analyze_schur): the held Schur complements [batch][ns, ns] row-major, the order of the Schur
    // front and the pool offset of its dense buffer (schur.hip); null / 0 on a plain handle
    double *schur = nullptr;
    int schur_ns = 0;
    long long schur_lpan = 0;
};

// What one solve, factorisation or fused step needs beyond the handle's resident state: built per call by api.cpp and
// passed down to every launcher (nothing of it is left on the DeviceFactor).
struct SweepCall {
    const std::vector<LaunchGroup> *groups = nullptr;   // the sweeps' launch groups (Symbolic::sgroups, or sgroups1 for one
    const SolveDesc *sd = nullptr;                      //   right-hand side on a forest handle) and their descriptors (sdesc / sdesc1)
    XMap xm;                      // fused permutations: the sweeps read and write the caller's X through q
    bool trans = false;           // LU: the forward sweep solves with U', the backward sweep with L'
    bool inverses_in_sweep = false;   // the forward sweep inverts the diagonal blocks group by group (fused factor + solve)
    bool fwd_in_factor = false;   // the forest's factor launch carries the forward sweep of its fronts (fused, one right-hand side)
};

// f(std::integral_constant<int, KIND>{}) for the handle's kind: the factorisation instances (never CS3_LU_T).
template <class F>
auto with_kind(int kind, F &&f)
{
    return (kind == CS3_LU) ? f(std::integral_constant<int, CS3_LU>{}) : f(std::integral_constant<int, CS3_CHOLESKY>{});
}

// How an LU pivot is accepted, as the factor launchers take it: a multiplier larger than inv_tol = 1 / tol rejects its
// column, and (static pivot perturbation, delta > 0) a pivot with |p| < delta is replaced by +delta before its reciprocal
// is formed; count [batch] takes the number of replaced pivots of every matrix.
struct PivotCtl {
    double inv_tol = HUGE_VAL, delta = 0.0;
    int *count = nullptr;
    bool operator==(const PivotCtl &o) const { return inv_tol == o.inv_tol && delta == o.delta; }
    bool operator!=(const PivotCtl &o) const { return !(*this == o); }
};
// The same as a kernel argument (by value), and as a template argument of every factor kernel: PivotRule<false> is the
// kernels' old `double inv_tol` and compiles to the instructions they had before the perturbation existed -- a handle
// with delta = 0 (and every Cholesky handle) runs those instances; PivotRule<true> exists for LU only.
template <bool ON> struct PivotRule;
template <> struct PivotRule<false> {
    static constexpr bool on = false;
    double inv_tol;
};
template <> struct PivotRule<true> {
    static constexpr bool on = true;
    double inv_tol, delta;
    int *count;
};
// f(rule) with the rule's type picked by delta.
template <int KIND, class F>
auto with_rule(const PivotCtl &pc, F &&f)
{
    if constexpr (KIND == CS3_LU) {
        if (pc.delta > 0.0) return f(PivotRule<true>{pc.inv_tol, pc.delta, pc.count});
    }
    return f(PivotRule<false>{pc.inv_tol});
}

// What the assembly of a front reads, as a kernel argument (by value).
struct AsmLists {
    const int *fa_tgt, *fa_src;   // entries of A: target in the front (image index / pool offset), entry of Ax
    const int *ch_tab;            // children: update rows, row map (first entry in rel_idx), block offset, leading dimension
    const int *rel_idx;
};

// The interleaved block as a kernel argument (by value).
struct IlView {
    double *base;                 // DeviceFactor::pool_il
    long long len;                // DeviceFactor::il_len (0: no interleaved region)
};

// Side streams and events used to run the independent launches of one tree level
// as parallel branches (of the captured graph, or of real streams in eager mode).
struct ForkJoin {
    static constexpr int NSIDE = 3;
    hipStream_t side[NSIDE] = {nullptr, nullptr, nullptr};
    hipStream_t aux = nullptr;             // carries the forward sweep next to the factorisation
    std::vector<hipEvent_t> events;
    size_t next = 0;
    hipError_t init();
    void destroy();
    hipError_t event(hipEvent_t *e);       // next event of the pool (grows on demand)
    void rewind() { next = 0; }
};

// ---- the launch schedule (schedule.cpp plans it, kernels.hip issues it) ---------------------------------------------
// Sizes of the kernels in kernels.hip that the schedule depends on.
constexpr int BIG_NB = 32;                 // big fronts: pivots per block-step launch
constexpr int SOLVE_BW = 64;               // the triangles of the block sweeps
constexpr int BIG_CW = 2 * SOLVE_BW;       // big-front sweeps, few right-hand sides: columns per chunk launch ...
constexpr int BIG_CW4 = 4 * SOLVE_BW;      //   ... of a front with more than BIG_CW pivots
constexpr int BIG_SR4 = 32;                // rows of a workgroup's slice (16 threads per row, 16 columns each)
constexpr int BIG_KT = 8;                  // right-hand sides per workgroup of the multi-vector chunk step
constexpr int GC = 64;                     // GEMM sweeps: pivots per chunk
constexpr int RHS_LANES_MIN = 16;          // from this many right-hand sides on, SK_SMALL fronts run lane = right-hand side
                                           //   and the fronts of order > 64 sweep as GEMMs
// pivots per block step: 16 keeps the kernel within 128 registers, i.e. two workgroups per CU (its phases are serial and
// latency-bound: 512 matrices took 809 us with one workgroup per CU, in two rounds; the 32-pivot form of round 2a is gone)
constexpr int WG_NB = 16;
constexpr int PROMOTE_MAX = 16;            // (8 .. 200 measured identical on config 3: only the top three levels hold such a group)

// A plan = the launches, event records and stream waits of one factorisation, sweep or factorisation with forward sweep,
// in the order they are issued.  Stream slot 0 is the caller's stream, 1 .. NSIDE are ForkJoin::side, SLOT_AUX is
// ForkJoin::aux; events are numbered from 0 in the order of their first record.
enum StepKind : int {
    STEP_FRONT_GROUP = 0,         // one call of launch_front_group (every class that is a single launch)
    STEP_BIG_GATHER, STEP_BIG_BLOCK /* arg: block */, STEP_SCHUR_TAKE,
    STEP_SWEEP_FWD, STEP_SWEEP_BWD,                   // one call of launch_solve_group
    STEP_FWD_BIG_PRE, STEP_FWD_BIG_CHUNK /* arg: chunk */, STEP_BWD_BIG_PRE, STEP_BWD_BIG_CHUNK /* arg: chunk */,
    STEP_RECORD, STEP_WAIT                            // event on / stream behind: slot, event
};
constexpr int SLOT_AUX = 4;
struct PlanStep {
    int kind, slot;
    LaunchGroup g;                // launches: the group (after factor_groups / sweep_groups)
    int arg, event;               // -1 where there is none
};
using LaunchPlan = std::vector<PlanStep>;

// What the schedule depends on, and nothing else.
struct ScheduleInput {
    const std::vector<LaunchGroup> *fgroups = nullptr;   // Symbolic::groups
    const std::vector<LaunchGroup> *sgroups = nullptr;   // Symbolic::sgroups, or sgroups1 when the sweeps follow the forest schedule
    int kind = CS3_LU, nrhs = 0;
    long long batch = 1;
    bool forest = false, forest_sweeps = false;          // a bottom forest exists; the sweeps follow its schedule (sgroups1)
    bool fwd_in_factor = false;                          // SweepCall::fwd_in_factor
};
LaunchPlan plan_factor_levels(const ScheduleInput &in);
LaunchPlan plan_solve_levels(const ScheduleInput &in, bool forward);
LaunchPlan plan_factor_with_forward(const ScheduleInput &in);

// Sweeps over a group of wide big fronts: a preparation launch, then one launch per chunk of columns.
struct BigSweepPlan {
    bool wide, multi;       // several 64-blocks per launch (latency-bound); BIG_KT right-hand sides per workgroup
    bool no_init;           // the backward sweep's first chunk launch reads X itself (k_bwd_big_step4, xmode)
    int cw, nchunk, slices;
    unsigned by, by_multi;
};
BigSweepPlan big_sweep_plan(long long batch, const LaunchGroup &g, int nrhs);
int wg_panel_ld(const LaunchGroup &g);
size_t wg_lds_bytes(int kind, const LaunchGroup &g);
bool gemm_sweeps_on();            // CS3_NO_GEMM_SWEEPS=1: many right-hand sides sweep the fronts of order > 64 by substitution

hipError_t prepare_kernels();
hipError_t launch_poison_lds(hipStream_t st);     // diagnostics: NaN patterns into every CU's LDS
hipError_t launch_diag_inverses(const DeviceFactor &D, hipStream_t st);
bool permutation_can_fuse(const DeviceFactor &D, int nrhs);   // once after a factorisation, before a many-RHS sweep
bool big_group_in_one_workgroup(int kind, long long batch, const LaunchGroup &g);
hipError_t launch_factor_levels(const DeviceFactor &D, const SweepCall &call, const std::vector<LaunchGroup> &groups,
                                const PivotCtl &pc, hipStream_t st, ForkJoin &fj);
// sweeps over call.groups
hipError_t launch_solve_levels(const DeviceFactor &D, const SweepCall &call, double *X, int nrhs, bool forward, hipStream_t st,
                               ForkJoin &fj);
// Factorisation with the forward sweep partly hidden behind it: the sweep of the finished levels
// runs on fj.aux beside the factorisation of the tail of the tree (one fork, one join).
hipError_t launch_factor_with_forward(const DeviceFactor &D, const SweepCall &call, const std::vector<LaunchGroup> &fgroups,
                                      const PivotCtl &pc, double *X, int nrhs, hipStream_t st, ForkJoin &fj);
// status word, big-front zeros, copy of the caller's values and (x_src != null) the permuted right-hand sides, one launch
hipError_t launch_prologue(const DeviceFactor &D, const double *ax_src, const double *x_src, int nrhs, hipStream_t st);
// forest.hip: the bottom forest = one launch, one workgroup per task
hipError_t prepare_forest_kernels();
hipError_t set_withhold_handover(int on);          // diagnostics: producers of the LDS hand-overs keep their counters back
hipError_t set_withhold_handover_forest(int on);   //   (the copy of the flag in forest.hip)
hipError_t launch_sub_factor(const DeviceFactor &D, const SweepCall &call, const PivotCtl &pc, hipStream_t st);
hipError_t launch_sub_sweep(const DeviceFactor &D, double *X, bool forward, hipStream_t st);
hipError_t launch_permute(const DeviceFactor &D, const double *src, double *dst, int nrhs, bool scatter,
                          hipStream_t st);
hipError_t launch_extract(const double *vals, const double *vals_il, long long il_len, const long long *map, double *out,
                          long long count, hipStream_t st);
hipError_t launch_tri_level(const int *rows, int nrows, const int *Rp, const int *Rj, const long long *Rmap,
                            const long long *diag, const double *Gx, double *X, int nrhs, hipStream_t st);
hipError_t launch_stack_4_by_4(int an, int bn, int am, int bm, const int *Ap, const int *Ai, const double *Ax,
                               const int *Bp, const int *Bi, const double *Bx, const int *Cp, const int *Ci,
                               const double *Cx, const int *Dp, const int *Di, const double *Dx,
                               int *Pp, int *Pi, double *Px, int *map, hipStream_t st);
hipError_t launch_restack_values(long long nnz, const int *map, long long na, long long nb, long long nc, const double *Ax,
                                 const double *Bx, const double *Cx, const double *Dx, double *Px, hipStream_t st);
hipError_t launch_residual(const int *Rp, const int *Rj, const int *Rmap, const double *Ax, const double *X, const double *B,
                           double *R, long long n, int nrhs, long long nnz_a, long long batch, hipStream_t st);
hipError_t launch_axpy_max(double *X, const double *D, long long total, unsigned long long *maxbits, hipStream_t st);
hipError_t launch_matvec_rows(const int *Rp, const int *Rj, const double *Rx, const double *X, double *Y,
                              long long m, int nrhs, hipStream_t st);

// schur.hip: the assembled Schur front of every matrix goes to D.schur (row-major; Cholesky: mirrored to the full
// symmetric matrix), the identity takes its place in the pool
hipError_t launch_schur_take(const DeviceFactor &D, hipStream_t st);

// estimate.hip: condition estimates (LAPACK dlacn2, one state machine per matrix of a batch) and log-determinants.
// The state of one matrix: step = what the next solve's result is for (1..5: dlacn2's J1..J5; J1, J3, J5 consume
// x = A^-1 b, J2 and J4 x = A^-T b), 0 = DONE; j = the current column, iter = dlacn2's iteration count; sbuf = which half
// of the sign buffer S [2][batch][n] (int8) holds the current sign vector s.
struct EstState {
    double est, anorm;            // the estimate of ||A^-1||_1 so far, ||A||_1
    int step, j, iter, sbuf;
};
// The reductions over a vector of n entries run on a FIXED partition (chunks of EST_CHUNK entries, one workgroup each) and
// a second stage that combines the chunks in index order: the same sums on every run, whatever the batch.
constexpr long long EST_CHUNK = 2048;
inline long long est_chunks(long long n) { return n > 0 ? (n + EST_CHUNK - 1) / EST_CHUNK : 1; }
constexpr long long EST_NORM_COLS = 256;       // ||A||_1: columns per workgroup (a max: any partition gives the same value)
inline long long norm_chunks(long long n) { return n > 0 ? (n + EST_NORM_COLS - 1) / EST_NORM_COLS : 1; }
struct EstPart {                  // one chunk: sum |x_i|, max |x_i| and its first index, flags (1: non-finite, 2: a sign changed)
    double sum, max;
    int idx, flags;
};
// ||A_b||_1 over the column view (Cp, Cmap: entry of Ax) and the initial states; parts [batch][norm_chunks(n)]
hipError_t launch_est_start(const int *Cp, const int *Cmap, const double *Ax, long long n, long long nnz_a, long long batch,
                            EstPart *parts, EstState *state, hipStream_t st);
// kmask: bit 0 = this slot solves with A^-1, bit 1 = with A^-T (a Cholesky slot serves both)
hipError_t launch_est_prepare(const EstState *state, const signed char *S, double *X, long long n, long long batch, int kmask,
                              unsigned *cnt, hipStream_t st);
hipError_t launch_est_consume(EstState *state, signed char *S, const double *X, long long n, long long batch, int kmask,
                              EstPart *parts, unsigned *cnt, hipStream_t st);
hipError_t launch_est_finalize(const EstState *state, long long batch, double *cond, double *inv_norm, hipStream_t st);
// diag[n]: virtual pool offset of every pivot's diagonal
hipError_t launch_slogdet(const DeviceFactor &D, const long long *diag, double *sign, double *logabs, hipStream_t st);

// matching.hip: a matched handle (cs3_analyze_matched) factorises B = P (Dr A Dc); its callers speak in terms of A.
struct MatchView {                // device arrays of the matching
    const double *dr, *dc;        // [n] row and column scalings
    const int *rq;                // [n] rowperm[q[k]]: the row of A behind pivot row k (D.q is the other row map)
    const int *erow, *ecol;       // [nnz_a] row and column of every entry of A
};
// dst [batch][nnz] = (dr[row] * src) * dc[col], entry by entry (src may be dst)
hipError_t launch_match_values(const MatchView &M, const double *src, double *dst, long long nnz, long long batch, hipStream_t st);
// k_permute_rows with a scaling: gather dst[k, :] = scale[map[k]] src[map[k], :], scatter dst[map[k], :] = scale[map[k]] src[k, :]
hipError_t launch_match_rows(const double *src, double *dst, const int *map, const double *scale, long long n, int nrhs,
                             long long batch, bool scatter, hipStream_t st);
// sign[b] *= parity (unless 0), logabs[b] += shift
hipError_t launch_match_slogdet(double *sign, double *logabs, long long batch, double parity, double shift, hipStream_t st);

// updates.hip: many low-rank-modified systems (A + dA_c) x = b on the held factors (cs3_updates_*).
constexpr int UPD_MAX_RANK = 16;               // distinct rows / columns of one case
constexpr int UPD_MAX_TILE = 1024;             // columns of A^-1 solved for at a time (the width the many-RHS path is tuned at)
constexpr int UPD_MAX_TILE_CASES = 1024;       // cases of one tile: lanes of one k_upd_apply workgroup
struct UpdCase {                  // one case as the kernels read it
    int r, s;                     // distinct rows / columns
    int col[UPD_MAX_RANK];        // its columns C_c, ascending (rows of Z and of x0 to gather)
    unsigned short zcol[UPD_MAX_RANK];    // where its rows R_c, ascending, sit among the columns of its tile of Z
};
struct UpdTables {                // device arrays of one plan
    const UpdCase *cases;         // [ncases]
    const int *cp;                // [ncases + 1] triplets of each case
    const unsigned char *tpos;    // [cp[ncases]] entry of D_c (16 x 16, row-major) each triplet adds to
    double *y;                    // [ncases][16] S_c^-1 D_c x0[C_c], zero-padded
    int *flag;                    // [ncases] 1: singular, its column of X is NaN
};
hipError_t prepare_updates_kernels();
// Z [n, t] = the unit vectors e_{unit_row[j]} (a negative row: a zero column)
hipError_t launch_upd_units(double *Z, long long n, int t, const int *unit_row, hipStream_t st);
// the cases c0 .. c0 + nc - 1 of one tile: y, rpiv, flag from the solved tile Z [n, t] and x0
hipError_t launch_upd_capacitance(const UpdTables &T, const double *cx, const double *Z, int t, const double *x0, int c0, int nc,
                                  double sing_tol, double *rpiv, hipStream_t st);
// columns c0 .. c0 + nc - 1 of X [n, ldx]; rmax = the largest rank among them
hipError_t launch_upd_apply(const UpdTables &T, const double *Z, int t, const double *x0, long long n, int c0, int nc, int rmax,
                            long long ldx, double *X, hipStream_t st);

// sens.hip: sparse right-hand sides, Y = C op(A)^-1 B on the held factors (cs3_sens_*).
constexpr int SENS_MAX_TILE = 1024;            // solved-for columns per tile (the width ensure_rhs_capacity and updates.hip use)
constexpr int SENS_PAD_WIDTH = 16;             // a narrower last tile is padded to this width (the GEMM sweeps start there)
constexpr int SENS_SCATTER_ROWS = 32;          // rows of the tile per k_sens_scatter workgroup
constexpr int SENS_SCATTER_THREADS = 256;      //   ... and its threads (a thread owns columns j, j + 256, ...)
constexpr int SENS_COMBINE_COLS = 32;          // columns of the other operand per k_sens_combine workgroup
constexpr int SENS_COMBINE_LANES = 64;         //   ... and its tile columns
constexpr int SENS_TBLOCK = 32;                // block edge of the transposing store: contiguous doubles per row of Y
struct SensOperand {              // a sparse operand by columns on the device; p == null: the identity (i, x unused)
    const int *p, *i;
    const double *x;
};
// T [n, w] = columns c0 .. c0 + t - 1 of `op`, zero columns behind them
hipError_t launch_sens_scatter(double *T, long long n, int w, const SensOperand &op, long long c0, int t, hipStream_t st);
// out[g, j] = sum over the entries (i, v) of column g < ng of `op` of v T[i, j], j < t; stored at Y[g * ldy + c0 + j], or
// (transposed) at Y[(c0 + j) * ldy + g]
hipError_t launch_sens_combine(const double *T, int w, int t, const SensOperand &op, long long ng, long long c0, long long ldy,
                               bool transposed, double *Y, hipStream_t st);

// selinv.hip / selinv.cpp: selected inversion, A^-1 on the pattern of L + U from the held factors (cs3_selinv_*).
// Every front gets a dense r x r column-major block Zfront of a second pool (zpool) holding Z = (Q' A Q)^-1 on its
// structure; fronts run parents first, a front gathers its update block from its parent's Zfront.
constexpr int SELINV_WAVE_R = 32;              // fronts up to this order: one wave each, four per workgroup
constexpr int SELINV_LDS_R = 136;              // ... up to this order: one workgroup each, the r x r image in LDS
constexpr int SELINV_TILE = 16;                // edge of an MFMA output tile (one wave computes one)
constexpr int SELINV_DIAG = 64;                // big fronts: pivots per chunk of the triangular solves
constexpr int SELINV_SLICE = 16;               // big fronts: vectors (rows of X, columns of Y and of the identity) per workgroup
enum SelinvClass : int { SELINV_WAVE = 0, SELINV_LDS = 1, SELINV_BIG = 2 };
struct SelFront {                 // one front as the kernels read it, in top-down schedule order
    long long lpan, upan;         // pool offsets of the panels
    long long z, zpar;            // zpool offsets of its Zfront and of its parent's
    long long wk;                 // big fronts: offset of X (c x w, ld c) in the work buffer, Y (w x c, ld w) behind it
    long long rel;                // first entry of its row map in rel_idx
    int r, w, rpar;               // order, pivots, the parent's order
    int u_sk, u_sj;
    int pad;
};
struct SelinvGroup {              // the fronts of one level and class: one launch (big fronts: three)
    int cls, first, count, max_r;
    int launch;                   // index of its first launch
    unsigned grid_prep, grid_cross, grid_pivot;      // big fronts: workgroups per front of the three launches
};
struct SelinvPlan {
    std::vector<SelFront> fronts;
    std::vector<i32> front_sn;                // supernode of every entry of `fronts`
    std::vector<i32> front_launch;            // index of the (first) launch that computes it
    std::vector<SelinvGroup> groups;
    std::vector<i64> z_off;                   // per supernode: zpool offset of its Zfront
    i64 zpool_doubles = 0, work_doubles = 0;
    i64 nsmall = 0, nbig = 0, nlaunches = 0;
};
void build_selinv_plan(const Symbolic &S, SelinvPlan &P);
// zpool offset of Z(k, l), k and l in pivot order; -1 when (k, l) is outside the pattern of L + U
i64 selinv_position(const Symbolic &S, const SelinvPlan &P, i64 k, i64 l);
hipError_t prepare_selinv_kernels();
struct SelinvView {               // device arrays of one call
    const double *pool;           // DeviceFactor::pool_pm
    long long pool_stride;
    double *zpool, *work;
    long long z_stride, work_stride;
    const SelFront *fronts;
    const int *rel_idx;
    long long batch;
};
hipError_t launch_selinv_group(int kind, const SelinvView &V, const SelinvGroup &g, hipStream_t st);
// out [batch][count] = zpool[b][map[e]]
hipError_t launch_selinv_gather(const double *zpool, long long z_stride, const long long *map, double *out, long long count,
                                long long batch, hipStream_t st);

// cplxselinv.hip: Z = A^-1 of a complex matrix out of the zpool of the handle on its real-equivalent form
// (cs3_cplx_selinv_*).  Per matrix Z(i, j) = (ZR(2i, 2j), ZR(2i + 1, 2j)) * s_j with the complex plan's rotation s.
constexpr int CSELINV_BLOCK = 256;             // threads per workgroup, one complex number per lane
constexpr int CSELINV_GRID_CAP = 2048;         // workgroups: grid-stride beyond
struct CselinvMaps {              // device tables of the handle, pairs stored side by side (one 16-byte or 8-byte load)
    const long long *entry;       // [nnz][2] zpool offsets of ZR(2i, 2j), ZR(2i + 1, 2j) for entry e = (i, j) of the complex matrix
    const long long *entry_t;     // [nnz][2] ... of ZR(2j, 2i), ZR(2j + 1, 2i)
    const long long *diag;        // [n][2]   ... of ZR(2i, 2i), ZR(2i + 1, 2i)
    const int *ij;                // [nnz][2] (i, j)
};
// out [batch][nnz] complex: Z(i, j), or with trans Z(j, i); s [batch][n] complex
hipError_t launch_cselinv_entries(const double *zpool, long long z_stride, const CselinvMaps &M, bool trans, const double *s,
                                  long long n, long long nnz, long long batch, double *out, hipStream_t st);
// out [batch][n] complex: Z(i, i)
hipError_t launch_cselinv_diag(const double *zpool, long long z_stride, const CselinvMaps &M, const double *s, long long n,
                               long long batch, double *out, hipStream_t st);
// out [batch][nnz] complex: ((Z(i, i) + Z(j, j)) - Z(i, j)) - Z(j, i)
hipError_t launch_cselinv_thevenin(const double *zpool, long long z_stride, const CselinvMaps &M, const double *s, long long n,
                                   long long nnz, long long batch, double *out, hipStream_t st);

// quadform.hip: bilinear forms t_i = c_i' A^-1 b_i on the zpool that cs3_selinv_dev left (cs3_quad_*), and the normalised
// residuals of a state estimate on top of them (cs3_quad_normres*).
constexpr int QUAD_BLOCK = 256;                // threads per workgroup of all three kernels (four waves)
constexpr int QUAD_LANE_TERMS = 32;            // rows with at most this many terms: one lane each
constexpr int QUAD_WAVE_TERMS = 1024;          // ... up to this many: one wave each, four per workgroup; beyond: one workgroup each
constexpr int QUAD_CHUNK = 8;                  // lane class: positions loaded together before their entries of Z
struct QuadRow {                  // one row as k_quad_forms reads it, in class order (lane rows, wave rows, workgroup rows)
    long long term0;              // its first term in the position table
    int c0, nc, b0, nb;           // its entries of C and of B in the value arrays (term u: entry u / nb of C, u % nb of B)
    int row;                      // the caller's row index
    int pad;
};
struct QuadShape {                // rows per class and the first workgroup of the wave and workgroup classes
    long long n_lane, n_wave, n_wg;
    unsigned blk_wave, blk_wg, blocks;
};
// t [batch][m]: t[b][row] = sum over the row's terms u of (cx[c0 + u / nb] * zpool[pos[term0 + u]]) * bx[b0 + u % nb]
hipError_t launch_quad_forms(const double *zpool, long long z_stride, const QuadRow *rows, const long long *pos, const QuadShape &G,
                             const double *cx, long long cx_stride, const double *bx, long long bx_stride, long long m,
                             long long batch, double *t, hipStream_t st);
// omega, rn [batch][m] (either may be null), summary [batch][4] = (max rn, its row, sum w r^2, critical rows) from t, w, r
// [batch][m]; parts [batch][ceil(m / QUAD_BLOCK)][4] is the workspace between the two launches
hipError_t launch_quad_normres(const double *t, const double *w, const double *r, double crit_tol, long long m, long long batch,
                               double *omega, double *rn, double *parts, double *summary, hipStream_t st);

// cplxsens.hip: the same around a handle on the real-equivalent form of a complex matrix (cs3_cplx_sens_*), and the
// complex Schur complement read out of the real one (cs3_cplx_schur_get*).  The tiling constants are those above; a
// complex row is a pair of real rows, so a scatter workgroup owns half as many.
constexpr int CSENS_SCATTER_ROWS = SENS_SCATTER_ROWS / 2;      // complex rows (pairs of real rows) per k_csens_scatter workgroup
constexpr int CSENS_BLOCK_LD = SENS_COMBINE_LANES + 1;         // LDS row of the transposing store, in complex numbers
struct CsensOperand {             // SensOperand with interleaved complex values (16-byte aligned)
    const int *p, *i;
    const double *x;
};
struct CsensGlue {                // what a tile goes through around the solve: pack / unpack of cs3_cplx_op `inner`, a conjugation
    int inner;                    //   of the solved-for values before the pack and of the solution after the unpack
    int conj;
    const double *s;              // the plan's rotation s [n] complex, as it stands in stream order
};
// T [2n, w] real = pack_inner of columns c0 .. c0 + t - 1 of `op` (n: the complex order), zero columns behind them
hipError_t launch_csens_scatter(double *T, long long n, int w, const CsensOperand &op, long long c0, int t, const CsensGlue &g,
                                hipStream_t st);
// out[g, j] = sum over the entries (i, v) of column g < ng of `op` of v * unpack_inner(T[2i, j], T[2i + 1, j]), j < t; stored
// at Y[g * ldy + c0 + j], or (transposed) at Y[(c0 + j) * ldy + g], Y complex
hipError_t launch_csens_combine(const double *T, int w, int t, const CsensOperand &op, long long ng, long long c0, long long ldy,
                                bool transposed, const CsensGlue &g, double *Y, hipStream_t st);
// S [batch][ns, ns] complex from SR [batch][2 ns, 2 ns] real: S[i, j] = (SR[2i, 2j], SR[2i + 1, 2j])
hipError_t launch_cplx_schur_gather(const double *SR, long long batch, long long ns, double *S, hipStream_t st);

// cplxupd.hip: many low-rank-modified COMPLEX systems (A + dA_c) v = i around a handle on the real-equivalent form
// (cs3_cplx_updates_*).  Plan, cases and tiles are those of updates.hip with n = the complex order (UpdCase, UpdTables;
// y is [ncases][16] complex here); a complex row is a pair of real rows of the tile Z [2n, t].
constexpr int CUPD_UNIT_ROWS = 8;              // complex rows (pairs of real rows) per k_cupd_units workgroup
constexpr int CUPD_UNIT_THREADS = 256;         //   ... and its threads (a thread owns columns j, j + 256, ...)
constexpr int CUPD_APPLY_STAGE = 4;            // complex rows of Z in LDS at a time: 2 x 4 x 1024 x 8 B = 64 KB at the full width
constexpr int CUPD_APPLY_ROWS = 64;            // complex rows per k_cupd_apply workgroup
constexpr int CUPD_APPLY_NT_MIN = 1024;        // threads of the smallest k_cupd_apply workgroup
hipError_t prepare_cupd_kernels();
// Z [2n, t]: column j = pack_N(e_{unit_row[j]}) with the rotation s [n] complex (a negative row: a zero column)
hipError_t launch_cupd_units(double *Z, long long n, int t, const int *unit_row, const double *s, hipStream_t st);
// the cases c0 .. c0 + nc - 1 of one tile: y, rpiv, flag from the solved tile Z [2n, t] and x0 [n] complex; cz interleaved
hipError_t launch_cupd_capacitance(const UpdTables &T, const double *cz, const double *Z, int t, const double *x0, int c0, int nc,
                                   double sing_tol, double *rpiv, hipStream_t st);
// columns c0 .. c0 + nc - 1 of X [n, ldx] complex; rmax = the largest rank among them
hipError_t launch_cupd_apply(const UpdTables &T, const double *Z, int t, const double *x0, long long n, int c0, int nc, int rmax,
                             long long ldx, double *X, hipStream_t st);

// krylov.hip: the vector layer of restarted GMRES on the held factors (cs3_gmres*), for batch * k systems in lock-step.
// Every vector is [batch][n, k] row-major; system s = b * k + t is column t of matrix b.  Reductions over the rows run on
// a FIXED partition (chunks of KRY_CHUNK rows) and the chunks are summed in index order by whoever consumes them: the
// same bits on every run, whatever the grid.
constexpr int KRY_MAX_RESTART = 32;
constexpr long long KRY_CHUNK = 1024;
constexpr int KRY_RHS_TILE = 64;
inline long long kry_chunks(long long n) { return n > 0 ? (n + KRY_CHUNK - 1) / KRY_CHUNK : 1; }
enum KryStatus : int { KRY_RUN = 0, KRY_DONE = 1, KRY_BAD = 2 };      // still iterating / finished / non-finite: frozen for good
struct KrySys {                   // one system
    double bnorm, relres;         // ||b||, the last TRUE ||b - A x|| / ||b|| (NaN: bad)
    double est;                   // |g_{j+1}| / ||b|| of the recurrence when the system last froze or its cycle ended
    double inv;                   // 1 / h_{j+1,j} for the next basis vector, 0: frozen
    int status, active, part;     // KryStatus; advancing in this cycle; took part in this cycle (gets the cycle's update)
    int iters, ncols;             // Krylov iterations so far; columns of this cycle's Hessenberg matrix
};
struct KryWork {                  // device arrays of one call (owned by the handle)
    double *V, *W, *Z;            // (restart + 1) basis vectors, w, and the vector that goes through the solves
    KrySys *sys;                  // [nsys]
    double *R, *cs, *sn, *g, *y;  // per system: R [restart][restart] (column j at j * restart), rotations, g [restart + 1], y
    double *parts;                // [2][nsys][restart][chunks] partial dots of the two Gram-Schmidt passes
    double *hsum;                 // [2][nsys][restart] ... summed over the chunks (by the update that consumes them)
    double *nparts;               // [2][nsys][chunks] partial squared norms (second half: of B, at the start)
    unsigned *cnt;                // [restart + 2] systems still active: after the start, after iteration j at [1 + j]
    long long n, k, batch, chunks;
    int restart;
};
// r = W on entry.  The norms, the state of every system for the coming cycle (first: ||b|| too, zero right-hand sides
// zero their column of X), v0 = r / ||r|| into V[0] and Z, cnt[0] = active systems.
hipError_t launch_kry_start(const KryWork &K, const double *B, double *X, bool first, double rtol, int max_iters, hipStream_t st);
// Iteration j on w = W: both Gram-Schmidt passes against V[0 .. j], the Hessenberg column with its rotations, the
// decision per system, v_{j+1} into V[j + 1] and Z, cnt[1 + j] = systems still active.
hipError_t launch_kry_step(const KryWork &K, int j, double rtol, int max_iters, hipStream_t st);
// y from R y = g, u = sum over the cycle's `cols` columns of y_i v_i into Z (zero for a system that took no part)
hipError_t launch_kry_combine(const KryWork &K, int cols, hipStream_t st);
// diagnostics: which = 0 the multi-dot, 1 the first update, 2 the second update with the norm, of iteration j alone
hipError_t launch_kry_probe(const KryWork &K, int which, int j, hipStream_t st);
// X += Z for the systems that took part in the cycle; every other column keeps its bits
hipError_t launch_kry_axpy(const KryWork &K, double *X, hipStream_t st);

// refine_xp.hip: extra-precise refinement (cs3_refine_xp*), batch * k systems in lock-step with the layouts of krylov.hip.
constexpr int XP_BLOCK = 256;                  // threads per workgroup of every kernel of the family
constexpr long long XP_GRID_CAP = 4096;        // workgroups (per matrix) of the residual and update kernels: grid-stride beyond
constexpr long long XP_MAXIMA_GRID_CAP = 1024; // workgroups over the rows of k_xp_maxima (per matrix and column tile): each ends in one atomic per column
constexpr int XP_MAX_ITERS_DEFAULT = 10;
constexpr double XP_EPS = 0x1p-52, XP_STALL_RATIO = 0.5;
enum XpFlag : int { XP_RUNNING = 0, XP_CONVERGED = 1, XP_STALLED = 2, XP_NONFINITE = 3 };
struct XpSys {                    // one system
    unsigned long long nd_bits, nx_bits;      // max |dx_i|, max |x_i| of this pass as bit patterns (zeroed by the control kernel)
    double nd_prev, rate;         // the last applied max |dx_i|; the largest nd / nd_prev so far
    int iters, flag;              // corrections applied; XpFlag
    int apply, stopped;           // this pass's correction goes into x; no longer iterating
};
// R = B - op(A) (X + XT) in doubled precision, rounded once; S = |B| + |op(A)| |X| (XT, S may be null).  ratio: R takes
// |r_i| / s_i instead (0 / 0 = 0), the closing pass's input to launch_xp_maxima.
hipError_t launch_residual_xp(const int *Rp, const int *Rj, const int *Rmap, const double *Ax, const double *B, const double *X,
                              const double *XT, double *R, double *S, long long n, int nrhs, long long nnz_a, long long batch,
                              bool ratio, hipStream_t st);
// per system: nd_bits = max over its column of |D|, nx_bits = of |X| (atomicMax on the bit patterns, onto what is there)
hipError_t launch_xp_maxima(const double *D, const double *X, XpSys *sys, long long n, int nrhs, long long batch, hipStream_t st);
// the decision of one pass per system; *active += the systems that go on
hipError_t launch_xp_control(XpSys *sys, long long nsys, unsigned *active, hipStream_t st);
// (x, xt) += dx in doubled precision for the systems whose apply is set; every other column keeps its bits
hipError_t launch_xp_update(double *X, double *XT, const double *D, const XpSys *sys, long long n, int nrhs, long long batch,
                            hipStream_t st);

}  // namespace cs3
