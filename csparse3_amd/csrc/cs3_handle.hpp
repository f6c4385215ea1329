// The handle and the plans made for it, as the host layer sees them: api.cpp (handles, graphs, factor and solve) and
// apps.cpp (the applications on held factors) share this and nothing else.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <map>
#include <tuple>
#include <vector>

#include "cs3_device.hpp"
#include "cs3_hipmem.hpp"

// Captured graphs, one cache per handle, keyed by what a capture bakes in: (operation, trans, nrhs, the caller's X when
// its address is inside the graph, else null).
//   - GRAPH_FACTOR: one graph (trans false, nrhs 0), dropped when inv_tol or the perturbation delta changes.
//   - GRAPH_SOLVE per (trans, nrhs): unbounded.  With fused permutations (X baked in) per (trans, nrhs, X): at most 8 per
//     trans -- the 9th clears that class (callers that rotate buffers).
//   - GRAPH_FUSED (factor + overlapped forward + backward) per nrhs: unbounded.  The same with the closing permutation
//     inside the graph (no eager launch behind it: 5 us) per (nrhs, X): at most 4, and only from the third call in a row
//     with the same X (fused_last_x / fused_same_x).  A change of inv_tol or delta drops every fused-step graph.
//   - ensure_rhs_capacity drops every solve and fused-step graph (the buffers they read move).
//   - GRAPH_SCHUR_FWD / GRAPH_SCHUR_BWD (the half-solves of a Schur handle) per nrhs: unbounded, X never baked in.
// A graph that may still be running on another stream is destroyed only after a hipDeviceSynchronize.
enum GraphOp { GRAPH_FACTOR, GRAPH_SOLVE, GRAPH_FUSED, GRAPH_SCHUR_FWD, GRAPH_SCHUR_BWD };
using GraphKey = std::tuple<int, bool, int, const void *>;     // (GraphOp, trans, nrhs, X)

namespace cs3 {

// What every plan made for a handle is (cs3_updates_plan, cs3_sens_plan and their complex forms): it sits in its handle's
// `plans` until one of the two is freed.  Plans and handle may be freed in either order: freeing the handle drops the
// device copies of its plans and clears their `h`, and such a plan can only be freed (plan_free in apps.cpp).
struct HeldPlan {
    cs3_handle h = nullptr;                   // null once the handle has been freed
    bool on_device = false;                   // the tables are in HBM (uploaded by the first solve)
    virtual ~HeldPlan() = default;
    void drop_device() { reset_memory(); on_device = false; }
protected:
    virtual void reset_memory() = 0;          // frees every device block of the plan
};

}  // namespace cs3

struct cs3_handle_s {
    cs3::Symbolic S;
    cs3::DeviceFactor D;
    long long batch = 1;
    bool on_device = false, factored = false;
    bool factor_ran = false;          // a numeric factorisation was enqueued on this handle (its counters mean something)
    bool use_graph = true;
    hipStream_t cap_stream = nullptr;
    cs3::ForkJoin fj;
    std::map<GraphKey, hipGraphExec_t> graphs;
    cs3::PivotCtl factor_ctl{0.0, 0.0, nullptr}, fused_ctl{0.0, 0.0, nullptr};     // what the factor / fused-step graphs were captured with
    double perturb_delta = 0.0;       // cs3_set_pivot_perturbation: LU pivots with |p| < delta become +delta (0: off)
    const void *fused_last_x = nullptr;
    int fused_same_x = 0;
    long long fail_col = -1;
    bool inverses_valid = false;      // inverted diagonal blocks (many-RHS GEMM sweeps) match the current factors
    // selected inversion (cs3_selinv_*): the plan and the extraction maps, built from S on first use (ensure_selinv_plan);
    // selinv_valid: mem.selinv.z holds Z of the current factors (every factor entry point clears it)
    struct Selinv {
        bool planned = false;
        cs3::SelinvPlan plan;
        std::vector<cs3::i64> entry, entry_t, diag;    // zpool offsets: A^-1(Ai[p], j), A^-1(j, Ai[p]) per entry of A; A^-1(i, i)
        // a handle on the real form of a complex matrix (ensure_cselinv_plan): the same in pairs (real part, imaginary
        // part) per entry and per row of the COMPLEX matrix, and (row, column) of every complex entry
        bool cplanned = false;
        std::vector<cs3::i64> centry, centry_t, cdiag;
        std::vector<cs3::i32> cij;
    } selinv;
    bool selinv_valid = false;
    std::vector<cs3::i32> Ap_host, Ai_host;
    // A matched handle (cs3_analyze_matched): S analyses B = P (Dr A Dc), Ap_host / Ai_host keep the pattern of A.
    struct Matching {
        bool on = false;
        std::vector<cs3::i32> rowperm;        // row of A matched to column j = row j of B
        std::vector<double> dr, dc;
        double t_match = 0.0;                 // host seconds of the matching
        double parity = 1.0, log_shift = 0.0; // det A = parity det B exp(log_shift): sign of rowperm, -(sum log dr + sum log dc)
    } match;
    std::vector<cs3::HeldPlan *> plans;       // the plans made for this handle, of every kind
    cs3::KryWork kry_work{};                  // the work arrays of the last cs3_gmres* call (views of mem.kry)
    // Every HBM block of the handle, one group per feature that builds it; release_device drops them all at once.  A
    // new feature declares its DevBuf in a group here and allocates it in its ensure_*: nothing else has to know.
    struct Memory {
        template <class T> using DevBuf = cs3::DevBuf<T>;
        // ensure_device: the arrays behind D's pointers (allocated together, die together) ...
        std::vector<DevBuf<unsigned char>> factor;
        // ... but for the sweep buffers D.cv, D.xp, D.bigv, D.gv, which grow with nrhs (ensure_rhs_capacity)
        DevBuf<double> cv, xp, bigv, gv;
        // ensure_row_view / ensure_col_view (residuals, refinement): the analysed pattern by rows, the same by columns
        // (transposed products), the residual R [batch][n][k] (grows), the bits of max |dx|
        struct { DevBuf<int> rp, rj, rmap, cp, ci, cmap; DevBuf<double> res; DevBuf<unsigned long long> maxbits; } view;
        // ensure_krylov (krylov.hip, cs3_gmres*): (restart + 1) basis vectors, w and the vector that goes through the
        // solves, all [batch][n, k]; per system its state, R, the rotations, g, y; the partial sums of the reductions and
        // their sums; the counters of active systems.  All grow with k and restart.
        struct {
            DevBuf<double> v, w, z, small, parts;
            DevBuf<cs3::KrySys> sys;
            DevBuf<unsigned> cnt;
        } kry;
        // ensure_refine_xp (refine_xp.hip, cs3_refine_xp*): the tail of the iterate [batch][n, k], one state per system,
        // the counter of active systems.  Grow with k.  (The residual / correction vector is view.res.)
        struct { DevBuf<double> tail; DevBuf<cs3::XpSys> sys; DevBuf<unsigned> cnt; } xpr;
        // ensure_estimator (estimate.hip): X [batch][n] (stable address: the solves on it replay the cached graphs), the
        // sign vectors [2][batch][n], one state per matrix, the chunks of the partial reductions, the two "wants" counters
        struct { DevBuf<double> x; DevBuf<signed char> s; DevBuf<cs3::EstState> state; DevBuf<cs3::EstPart> parts; DevBuf<unsigned> cnt; } est;
        // the host forms of condest / slogdet stage through these: values of A, results [2][batch]
        struct { DevBuf<double> ax, out; } host;
        DevBuf<cs3::i64> diag;        // ensure_diag_map (log-determinants): virtual pool offset of every pivot's diagonal
        // cs3_get_factors: where the entries of L and U sit in the pool, and their values gathered
        struct { DevBuf<cs3::i64> lmap, umap; DevBuf<double> lx, ux; } exp;
        // ensure_updates (updates.hip, cplxupd.hip): the tile of A^-1 columns Z [n][widest tile so far] of the REAL plans
        // (grows; the complex ones keep theirs in sens.t) and x0 [n] of both (stable addresses: the solves on them replay
        // the cached graphs)
        struct { DevBuf<double> z, x0; } upd;
        // ensure_sens (sens.hip, cplxsens.hip): the tile of right-hand sides T [n][widest solve width so far] (grows; a
        // stable address: the solves on it replay the cached graphs)
        struct { DevBuf<double> t; } sens;
        // ensure_match (matching.hip): the scalings, the row of A behind every pivot row, row and column of every entry
        struct { DevBuf<double> dr, dc; DevBuf<int> rq, erow, ecol; } match;
        // ensure_device on a Schur handle (schur.hip): the held Schur complements S [batch][ns, ns]
        DevBuf<double> schur;
        // ensure_selinv (selinv.hip): zpool [batch][zpool_doubles], X and Y of the big fronts [batch][work_doubles], the
        // fronts in top-down order, the extraction maps (those on the CSC factors: cs3_selinv_factors), the host forms' results
        struct { DevBuf<double> z, work, out; DevBuf<cs3::SelFront> fronts; DevBuf<cs3::i64> entry, entry_t, diag, lmap, umap; } selinv;
        // ensure_cselinv (cplxselinv.hip, a handle on the real form of a complex matrix): the same maps in pairs per entry
        // and per row of the COMPLEX matrix ([.][2], CselinvMaps), row and column of every complex entry
        struct { DevBuf<cs3::i64> entry, entry_t, diag; DevBuf<cs3::i32> ij; } cselinv;
    } mem;
    // diagnostics (cs3_debug_alloc_counters): device allocations / graph instantiations and host synchronisations made by the
    // solves and the paths on top of them
    long long dbg_allocs = 0, dbg_syncs = 0;
};

// One list of sparse modifications dA_c of a handle's matrix, pattern only (cs3_updates_plan, cs3_cplx_updates_plan).
// Cases are grouped into TILES: consecutive cases whose union of touched rows fits the tile width; a tile is one many-RHS
// solve.  A complex plan (p set) is one for a handle on the real form of a complex matrix: n is the COMPLEX order, the
// handle's is 2 n; mem.y holds 16 complex numbers per case, mem.cx the host form's interleaved values.
struct cs3_updates_s : cs3::HeldPlan {
    const cs3_cplx_s *p = nullptr;            // the complex plan it was made with (compared, never followed); null: a real plan
    cs3::i64 n = 0, ncases = 0, ntrip = 0, nrows_unique = 0, max_rank = 0;
    int tile_cap = cs3::UPD_MAX_TILE;
    std::vector<cs3::UpdCase> cases;
    std::vector<cs3::i32> cp;
    std::vector<unsigned char> tpos;
    struct Tile {
        int c0, nc;                           // its cases
        int t, t_solve;                       // touched rows, and the width it is solved at (t rounded up; zero columns behind t)
        int rmax;                             // largest rank among its cases
        cs3::i64 unit0;                       // its slice of unit_row (t_solve entries)
    };
    std::vector<Tile> tiles;
    std::vector<cs3::i32> unit_row;           // row of the unit entry of every tile column, -1: a zero column
    // device copies (uploaded by the first solve), per-case results, the host form's copy of the triplet values
    struct Memory {
        cs3::DevBuf<cs3::UpdCase> cases;
        cs3::DevBuf<int> cp, unit, flag;
        cs3::DevBuf<unsigned char> tpos;
        cs3::DevBuf<double> y, rpiv, cx;
    } mem;
protected:
    void reset_memory() override { mem = Memory(); }
};
struct cs3_cplx_updates_s : cs3_updates_s {};

// The patterns of B and C' of one Y = C op(A)^-1 B, the side it is evaluated from and its tiles (cs3_sens_plan,
// cs3_cplx_sens_plan).  A complex plan is one for a handle on the real form of a complex matrix: n is the COMPLEX order,
// the handle's is 2 n, and the host form's copies hold interleaved complex numbers.
struct cs3_sens_s : cs3::HeldPlan {
    cs3::i64 n = 0, k = 0, p = 0;
    int side = 1;                             // 1: solve for columns of B, 2: for rows of C
    int op = CS3_CPLX_N;                      // cs3_cplx_op; a real plan: N, or T for `trans`
    bool b_ident = false, c_ident = false;
    int tile_cap = cs3::SENS_MAX_TILE, wmax = 1;
    std::vector<cs3::i32> bp, bi, ctp, cti;   // empty for an identity operand
    struct Tile {
        cs3::i64 c0;                          // first solved-for column
        int t, w;                             // its columns, and the width it is solved at (zero columns behind t)
    };
    std::vector<Tile> tiles;
    // device copies (uploaded by the first solve); the host form's copies of the values and of Y
    struct Memory {
        cs3::DevBuf<int> bp, bi, ctp, cti;
        cs3::DevBuf<double> bx, ctx, y;
    } mem;
    cs3::i64 nnz_b() const { return b_ident ? n : (cs3::i64) bi.size(); }
    cs3::i64 nnz_c() const { return c_ident ? n : (cs3::i64) cti.size(); }
protected:
    void reset_memory() override { mem = Memory(); }
};
struct cs3_cplx_sens_s : cs3_sens_s {};

// The term map of m bilinear forms t_i = c_i' A^-1 b_i on a handle's selected inverse (cs3_quad_plan): per row, in the
// caller's order, its class and its terms' zpool offsets (a-major); the rows again in class order as the kernel reads them.
// The offsets come from the analysis alone, so a plan survives refactorisations.
struct cs3_quad_s : cs3::HeldPlan {
    cs3::i64 m = 0, nnz_c = 0, nnz_b = 0;     // nnz_b == nnz_c and every (b0, nb) == (c0, nc) when B = C
    bool same = false;                        // B = C: one value array
    std::vector<cs3::i32> row_class;          // per row: 0 lane, 1 wave, 2 workgroup
    std::vector<cs3::i64> term_ptr, term_pos; // [m + 1], [term_ptr[m]]
    std::vector<cs3::QuadRow> rows;           // class order; lane rows by ascending term count (stable)
    cs3::QuadShape shape{};
    // device copies (uploaded by the first call) and what the calls stage through: t when the caller wants none and the
    // partials of the normalised residuals (allocated with the tables); the host forms' values, weights, residuals, results
    struct Memory {
        cs3::DevBuf<cs3::QuadRow> rows;
        cs3::DevBuf<cs3::i64> pos;
        cs3::DevBuf<double> t, parts, cx, bx, w, r, out;
    } mem;
protected:
    void reset_memory() override { mem = Memory(); }
};

// What apps.cpp calls of api.cpp.
namespace cs3 {

int guard(cs3_handle h);                      // a null handle: CS3_ERR_ARG
// A Schur handle holds the factors of A with A22 replaced by A22 - S + I: whatever would silently answer for that matrix
// is refused.
int refuse_schur(cs3_handle h, const char *who);
// mode 0: full solve with permutations; 1: lsolve only; 2: usolve only (in pivot order, on X itself).
// trans (LU): A' X = B; the forward sweep solves with U', the backward sweep with L' (mode 1: utsolve, 2: ltsolve).
// On a Cholesky handle A' = A and trans changes nothing.
int run_solve(cs3_handle h, double *x_dev, long long k, int mode, hipStream_t st, bool trans = false);
int ensure_rhs_capacity(cs3_handle h, long long nrhs);

}  // namespace cs3
