// C ABI of the library (include/csparse3_amd.h): handle management, HBM
// residency, hipGraph capture of the level schedules, host <-> device copies.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>

#include "cs3_device.hpp"

using namespace cs3;

namespace {
thread_local std::string g_error;
}

namespace cs3 {
void set_error(const std::string &msg) { g_error = msg; }
}

#define CS3_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_error(std::string(#call) + ": " + hipGetErrorString(e_));               \
            return CS3_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// Captured graphs, one cache per handle, keyed by what a capture bakes in: (operation, trans, nrhs, the caller's X when
// its address is inside the graph, else null).
//   - GRAPH_FACTOR: one graph (trans false, nrhs 0), dropped when inv_tol changes.
//   - GRAPH_SOLVE per (trans, nrhs): unbounded.  With fused permutations (X baked in) per (trans, nrhs, X): at most 8 per
//     trans -- the 9th clears that class (callers that rotate buffers).
//   - GRAPH_FUSED (factor + overlapped forward + backward) per nrhs: unbounded.  The same with the closing permutation
//     inside the graph (no eager launch behind it: 5 us) per (nrhs, X): at most 4, and only from the third call in a row
//     with the same X (fused_last_x / fused_same_x).  A change of inv_tol drops every fused-step graph.
//   - ensure_rhs_capacity drops every solve and fused-step graph (the buffers they read move).
// A graph that may still be running on another stream is destroyed only after a hipDeviceSynchronize.
enum GraphOp { GRAPH_FACTOR, GRAPH_SOLVE, GRAPH_FUSED };
using GraphKey = std::tuple<int, bool, int, const void *>;     // (GraphOp, trans, nrhs, X)

struct cs3_handle_s {
    Symbolic S;
    DeviceFactor D;
    long long batch = 1;
    bool on_device = false, factored = false;
    bool use_graph = true;
    hipStream_t cap_stream = nullptr;
    ForkJoin fj;
    std::map<GraphKey, hipGraphExec_t> graphs;
    double factor_inv_tol = 0.0, fused_inv_tol = 0.0;     // what the factor / fused-step graphs were captured with
    const void *fused_last_x = nullptr;
    int fused_same_x = 0;
    i64 *d_lmap = nullptr, *d_umap = nullptr;
    double *d_lx = nullptr, *d_ux = nullptr;
    long long fail_col = -1;
    bool inverses_valid = false;      // inverted diagonal blocks (many-RHS GEMM sweeps) match the current factors
    // residual / refinement: the analysed pattern in row view (built on first use), a work array, a result word
    std::vector<i32> Ap_host, Ai_host;
    int *d_rp = nullptr, *d_rj = nullptr, *d_rmap = nullptr;
    int *d_cp = nullptr, *d_ci = nullptr, *d_cmap = nullptr;       // the same pattern in column view (transposed products)
    double *d_res = nullptr;
    long long res_cap = 0;
    unsigned long long *d_maxbits = nullptr;
    // condition estimates (estimate.hip), allocated on first use: X [batch][n] (stable address: the solves on it replay the
    // cached graphs), the sign vectors [2][batch][n], one state per matrix, the chunks of the partial reductions, the two
    // "wants" counters; the host forms' buffers; the virtual pool offset of every pivot's diagonal (log-determinants)
    double *d_est_x = nullptr;
    signed char *d_est_s = nullptr;
    EstState *d_est_state = nullptr;
    EstPart *d_est_parts = nullptr;
    unsigned *d_est_cnt = nullptr;
    double *d_est_ax = nullptr, *d_est_out = nullptr;
    i64 *d_diag = nullptr;
    // low-rank-modified solves (updates.hip): the plans made for this handle, the tile of A^-1 columns Z [n][upd_z_cols] and
    // x0 [n] (stable addresses: the solves on them replay the cached graphs), allocated on first use
    std::vector<cs3_updates_s *> plans;
    double *d_upd_z = nullptr, *d_upd_x0 = nullptr;
    long long upd_z_cols = 0;
    // diagnostics (cs3_debug_alloc_counters): device allocations / graph instantiations and host synchronisations made by the
    // solves and the paths on top of them
    long long dbg_allocs = 0, dbg_syncs = 0;
};

// One list of sparse modifications dA_c of a handle's matrix, pattern only (cs3_updates_plan).  Cases are grouped into
// TILES: consecutive cases whose union of touched rows fits the tile width; a tile is one many-RHS solve.
struct cs3_updates_s {
    cs3_handle h = nullptr;                   // null once the handle has been freed: the plan can then only be freed
    i64 n = 0, ncases = 0, ntrip = 0, nrows_unique = 0, max_rank = 0;
    int tile_cap = UPD_MAX_TILE;
    std::vector<UpdCase> cases;
    std::vector<i32> cp;
    std::vector<unsigned char> tpos;
    struct Tile {
        int c0, nc;                           // its cases
        int t, t_solve;                       // touched rows, and the width it is solved at (t rounded up; zero columns behind t)
        int rmax;                             // largest rank among its cases
        i64 unit0;                            // its slice of unit_row (t_solve entries)
    };
    std::vector<Tile> tiles;
    std::vector<i32> unit_row;                // row of the unit entry of every tile column, -1: a zero column
    // device copies (uploaded by the first solve) and per-case results
    UpdCase *d_cases = nullptr;
    int *d_cp = nullptr, *d_unit = nullptr, *d_flag = nullptr;
    unsigned char *d_tpos = nullptr;
    double *d_y = nullptr, *d_rpiv = nullptr, *d_cx = nullptr;
    bool on_device = false;
};

namespace {

template <class T>
int upload(T **dst, const std::vector<T> &src)
{
    size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    CS3_HIP(hipMalloc((void **) dst, bytes));
    if (!src.empty()) CS3_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return CS3_OK;
}

// Destroys the cached graphs whose key satisfies `drop`, after a device synchronisation when there are any (unless the
// caller has just synchronised).
template <class Pred>
int drop_graphs(cs3_handle h, Pred drop, bool synced = false)
{
    bool any = false;
    for (const auto &kv : h->graphs) any = any || drop(kv.first);
    if (!any) return CS3_OK;
    if (!synced) { CS3_HIP(hipDeviceSynchronize()); h->dbg_syncs += 1; }
    for (auto it = h->graphs.begin(); it != h->graphs.end(); ) {
        if (drop(it->first)) { (void) hipGraphExecDestroy(it->second); it = h->graphs.erase(it); }
        else ++it;
    }
    return CS3_OK;
}

bool graph_op_is(const GraphKey &k, int op) { return std::get<0>(k) == op; }

void release_plan_device(cs3_updates_s *u)
{
    void **ptrs[] = {(void **) &u->d_cases, (void **) &u->d_cp, (void **) &u->d_unit, (void **) &u->d_flag, (void **) &u->d_tpos,
                     (void **) &u->d_y, (void **) &u->d_rpiv, (void **) &u->d_cx};
    for (void **p : ptrs) if (*p) { (void) hipFree(*p); *p = nullptr; }
    u->on_device = false;
}

// Frees every HBM allocation of the handle (ensure_device's error path and cs3_free).
void release_device(cs3_handle h)
{
    DeviceFactor &D = h->D;
    for (cs3_updates_s *u : h->plans) release_plan_device(u);
    h->upd_z_cols = 0;
    (void) drop_graphs(h, [](const GraphKey &) { return true; }, true);     // (cs3_free has synchronised)
    if (h->cap_stream) { (void) hipStreamDestroy(h->cap_stream); h->cap_stream = nullptr; }
    h->fj.destroy();
    void **ptrs[] = {(void **) &D.fdesc, (void **) &D.st_idx, (void **) &D.fa_tgt, (void **) &D.fa_src, (void **) &D.ch_tab, (void **) &D.rel_idx,
                     (void **) &D.sdesc, (void **) &D.sdesc1, (void **) &D.sub_tasks, (void **) &D.sub_fronts, (void **) &D.sub_lvl,
                     (void **) &D.sub_rel, (void **) &D.sub_st, (void **) &D.sub_child, (void **) &D.sub_a_tgt, (void **) &D.sub_a_src,
                     (void **) &D.axf, (void **) &D.fasm_src, (void **) &D.fasm_tgt, (void **) &D.flong_src, (void **) &D.rl_pairs,
                     (void **) &D.sl_src,                     (void **) &D.q, (void **) &D.ila_pairs, (void **) &D.inv_tasks, (void **) &D.dinv, (void **) &D.gv,
                     (void **) &D.ax, (void **) &D.pool, (void **) &D.dbuf, (void **) &D.tbuf, (void **) &D.bigv,
                     (void **) &D.cv, (void **) &D.xp, (void **) &D.status, (void **) &h->d_lmap, (void **) &h->d_umap,
                     (void **) &h->d_lx, (void **) &h->d_ux, (void **) &h->d_rp, (void **) &h->d_rj, (void **) &h->d_rmap,
                     (void **) &h->d_cp, (void **) &h->d_ci, (void **) &h->d_cmap, (void **) &h->d_res, (void **) &h->d_maxbits,
                     (void **) &h->d_est_x, (void **) &h->d_est_s, (void **) &h->d_est_state, (void **) &h->d_est_parts, (void **) &h->d_est_cnt,
                     (void **) &h->d_est_ax, (void **) &h->d_est_out, (void **) &h->d_diag, (void **) &h->d_upd_z, (void **) &h->d_upd_x0};
    h->res_cap = 0;
    for (void **p : ptrs) if (*p) { (void) hipFree(*p); *p = nullptr; }
    D.nrhs_cap = 0;
    h->on_device = false;
}

SolveDesc solve_desc_of(const Symbolic &S, i32 s)
{
    SolveDesc f{};
    f.lpan = S.lpan_off[s]; f.upan = S.upan_off[s]; f.cv = S.cv_off[s]; f.st = S.st_ptr[s];
    f.fasm_begin = S.fasm_ptr[s]; f.fasm_count = (int) (S.fasm_ptr[s + 1] - S.fasm_ptr[s]);
    f.bv = S.bv_off[s];
    f.gv = S.gv_off[s]; f.dinv = S.dinv_off[s];
    f.rl_begin = S.rl_ptr[s]; f.rl_count = (int) (S.rl_ptr[s + 1] - S.rl_ptr[s]);
    if (S.sn_class[s] != FC_IL) { f.rl_begin = S.sl_ptr[s]; f.rl_count = S.sl_rounds[s]; }   // not a lane = matrix sweep
    f.c0 = S.sn_ptr[s];
    f.r = (int) (S.st_ptr[s + 1] - S.st_ptr[s]);
    f.w = S.sn_ptr[s + 1] - S.sn_ptr[s];
    f.u_sk = S.u_sk[s]; f.u_sj = S.u_sj[s];
    f.parent = S.sn_parent[s];
    return f;
}

int ensure_device_impl(cs3_handle h);

// Uploads the analysis and allocates the numeric state; a failure half way leaves nothing behind, so a
// retry starts from scratch instead of allocating on top of the leaked buffers.
int ensure_device(cs3_handle h)
{
    if (h->on_device) return CS3_OK;
    const int rc = ensure_device_impl(h);
    if (rc != CS3_OK) release_device(h);
    return rc;
}

int ensure_device_impl(cs3_handle h)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: the numeric path runs on the GPU only (there is no CPU fallback)");
        return CS3_ERR_HIP;
    }
    CS3_HIP(prepare_kernels());
    CS3_HIP(prepare_forest_kernels());
    const Symbolic &S = h->S;
    DeviceFactor &D = h->D;
    D.kind = S.kind; D.n = S.n; D.nnz_a = S.nnzA; D.batch = h->batch;
    D.vals_size = S.vals_size; D.pool_size = S.pool_size; D.cv_size = S.cv_size; D.big_begin = S.big_begin;
    D.bv_size = S.bv_size;
    D.gv_size = S.gv_size; D.dinv_size = S.dinv_size; D.n_inv_tasks = (int) (S.inv_tasks.size() / 2);
    D.inv_tasks_host.assign(S.inv_tasks.begin(), S.inv_tasks.end());
    D.zero_big = false;
    for (const LaunchGroup &g : S.groups)
        if (g.cls == FC_BIG && !big_group_in_one_workgroup(S.kind, h->batch, g)) D.zero_big = true;
    std::vector<FrontDesc> fdesc(S.nsuper);
    i64 dbuf_size = 0;
    for (i32 t = 0; t < S.nsuper; ++t) {
        const i32 s = S.sched[t];
        FrontDesc &f = fdesc[t];
        f.lpan = S.lpan_off[s]; f.upan = S.upan_off[s]; f.cb = S.cb_off[s];
        f.a_begin = S.fa_ptr[s]; f.a_count = (int) (S.fa_ptr[s + 1] - S.fa_ptr[s]);
        f.ch_begin = (int) S.ch_ptr[s]; f.ch_count = (int) (S.ch_ptr[s + 1] - S.ch_ptr[s]);
        if (S.sn_class[s] == FC_IL) { f.a_begin = S.ila_ptr[s]; f.a_count = (int) (S.ila_ptr[s + 1] - S.ila_ptr[s]); }
        f.c0 = S.sn_ptr[s];
        f.r = (int) (S.st_ptr[s + 1] - S.st_ptr[s]);
        f.w = S.sn_ptr[s + 1] - S.sn_ptr[s];
        f.cb_ld = S.cb_ld[s]; f.u_sk = S.u_sk[s]; f.u_sj = S.u_sj[s];
        f.parent = S.sn_parent[s];
        f.dbuf = 0;
        if (S.sn_class[s] == FC_BIG) { f.dbuf = dbuf_size; dbuf_size += (i64) ((f.w + 31) / 32) * 1024; }
    }
    D.dbuf_size = dbuf_size;
    std::vector<SolveDesc> sdesc(S.nsuper);
    for (i32 t = 0; t < S.nsuper; ++t) sdesc[t] = solve_desc_of(S, S.ssched[t]);
    int rc;
    // the bottom forest and the sweep schedule of one right-hand side that goes with it
    D.sub_forest = S.sub_forest;
    D.n_sub_a = (long long) S.sub_a_tgt.size();
    if (!S.sub_forest.empty()) {
        std::vector<SolveDesc> sdesc1(S.nsuper);
        for (i32 t = 0; t < S.nsuper; ++t) sdesc1[t] = solve_desc_of(S, S.ssched1[t]);
        if ((rc = upload(&D.sdesc1, sdesc1))) return rc;
        if ((rc = upload(&D.sub_tasks, S.sub_tasks))) return rc;
        if ((rc = upload(&D.sub_fronts, S.sub_fronts))) return rc;
        if ((rc = upload(&D.sub_lvl, S.sub_lvl))) return rc;
        if ((rc = upload(&D.sub_rel, S.sub_rel))) return rc;
        if ((rc = upload(&D.sub_st, S.sub_st))) return rc;
        if ((rc = upload(&D.sub_child, S.sub_child))) return rc;
        if ((rc = upload(&D.sub_a_tgt, S.sub_a_tgt))) return rc;
        if ((rc = upload(&D.sub_a_src, S.sub_a_src))) return rc;
        CS3_HIP(hipMalloc((void **) &D.axf, std::max<size_t>(1, (size_t) (D.batch * D.n_sub_a)) * sizeof(double)));
    }
    if ((rc = upload(&D.sdesc, sdesc))) return rc;
    if ((rc = upload(&D.fasm_src, S.fasm_src))) return rc;
    if ((rc = upload(&D.fasm_tgt, S.fasm_tgt))) return rc;
    if ((rc = upload(&D.flong_src, S.flong_src))) return rc;
    if ((rc = upload(&D.rl_pairs, S.rl_pairs))) return rc;
    if ((rc = upload(&D.sl_src, S.sl_src))) return rc;
    if ((rc = upload(&D.fdesc, fdesc))) return rc;
    if ((rc = upload(&D.st_idx, S.st_idx))) return rc;
    if ((rc = upload(&D.fa_tgt, S.fa_tgt))) return rc;
    if ((rc = upload(&D.fa_src, S.fa_src))) return rc;
    {
        std::vector<i32> tab(S.ch_tab);
        tab.resize(tab.size() + 4, 0);                          // (16-byte loads of the last entry stay inside the array)
        if ((rc = upload(&D.ch_tab, tab))) return rc;
    }
    if ((rc = upload(&D.rel_idx, S.rel_idx))) return rc;
    if ((rc = upload(&D.q, S.q))) return rc;
    if ((rc = upload(&D.ila_pairs, S.ila_pairs))) return rc;
    if ((rc = upload(&D.inv_tasks, S.inv_tasks))) return rc;
    CS3_HIP(hipMalloc((void **) &D.dinv, std::max<size_t>(1, (size_t) (D.batch * D.dinv_size)) * sizeof(double)));
    D.il_len = S.il_len;
    D.pm_stride = S.pool_size - S.il_len;
    D.ngroups = (D.batch + 63) / 64;
    const size_t il_doubles = (size_t) (D.ngroups * 64 * D.il_len);
    CS3_HIP(hipMalloc((void **) &D.pool, (il_doubles + (size_t) (D.batch * D.pm_stride) + POOL_SLACK) * sizeof(double)));   // slack: see k_fwd_rhs
    D.pool_il = D.pool;
    D.pool_pm = D.pool + il_doubles - D.il_len;            // virtual offsets >= il_len index this pointer directly
    CS3_HIP(hipMalloc((void **) &D.dbuf, std::max<size_t>(1, (size_t) (D.batch * D.dbuf_size)) * sizeof(double)));
    CS3_HIP(hipMalloc((void **) &D.ax, std::max<size_t>(1, (size_t) (D.batch * D.nnz_a)) * sizeof(double)));
    CS3_HIP(hipMalloc((void **) &D.status, 4 * sizeof(int)));    // [0] the status word, [1], [2] unused, [3] a hand-over between waves timed out
    CS3_HIP(hipMemset(D.status, 0, 4 * sizeof(int)));
    CS3_HIP(hipMemset(D.status, 0x7f, sizeof(int)));      // "clean": a handle that only imports factors never runs a prologue
    if (const char *pf = std::getenv("CS3_PROFILE")) {
        if (pf[0] == '1') {
            CS3_HIP(hipMalloc((void **) &D.tbuf, std::max<size_t>(1, (size_t) S.nsuper) * 8 * sizeof(long long)));
            CS3_HIP(hipMemset(D.tbuf, 0, std::max<size_t>(1, (size_t) S.nsuper) * 8 * sizeof(long long)));
        }
    }
    CS3_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    CS3_HIP(h->fj.init());
    const char *ng = std::getenv("CS3_NO_GRAPH");
    h->use_graph = !(ng && ng[0] == '1');
    h->on_device = true;
    return CS3_OK;
}

int ensure_rhs_capacity(cs3_handle h, long long nrhs)
{
    DeviceFactor &D = h->D;
    if (nrhs <= D.nrhs_cap) return CS3_OK;
    CS3_HIP(hipDeviceSynchronize());
    h->dbg_syncs += 1;
    h->dbg_allocs += 4;
    if (int rc = drop_graphs(h, [](const GraphKey &k) { return !graph_op_is(k, GRAPH_FACTOR); }, true)) return rc;
    if (D.cv) (void) hipFree(D.cv);
    if (D.xp) (void) hipFree(D.xp);
    if (D.bigv) (void) hipFree(D.bigv);
    if (D.gv) (void) hipFree(D.gv);
    D.cv = D.xp = D.bigv = D.gv = nullptr;
    D.nrhs_cap = 0;                           // nothing usable until all three are back
    CS3_HIP(hipMalloc((void **) &D.cv, std::max<size_t>(1, (size_t) (D.batch * D.cv_size * nrhs)) * sizeof(double)));
    CS3_HIP(hipMalloc((void **) &D.xp, std::max<size_t>(1, (size_t) (D.batch * D.n * nrhs)) * sizeof(double)));
    CS3_HIP(hipMalloc((void **) &D.bigv, std::max<size_t>(1, (size_t) (D.batch * D.bv_size * nrhs)) * sizeof(double)));
    CS3_HIP(hipMalloc((void **) &D.gv, std::max<size_t>(1, (size_t) (D.batch * D.gv_size * nrhs)) * sizeof(double)));
    D.nrhs_cap = nrhs;
    return CS3_OK;
}

// Capture `body` (kernel launches on h->cap_stream) into an executable graph.
template <class Body>
int capture(cs3_handle h, hipGraphExec_t *exec, Body body)
{
    hipGraph_t graph = nullptr;
    h->dbg_allocs += 1;
    CS3_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    hipError_t e = body(h->cap_stream);
    hipError_t e2 = hipStreamEndCapture(h->cap_stream, &graph);
    if (e != hipSuccess) { if (graph) (void) hipGraphDestroy(graph); CS3_HIP(e); }
    CS3_HIP(e2);
    hipError_t e3 = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void) hipGraphDestroy(graph);
    CS3_HIP(e3);
    return CS3_OK;
}

// Replays the cached graph of `key` on st, capturing `body` (launches on the stream it is given) on cap_stream first when
// the graph is missing; a bounded class that is full is cleared first.  CS3_NO_GRAPH=1: runs `body` on st.
template <class Body>
int replay_or_run(cs3_handle h, const GraphKey &key, hipStream_t st, Body body)
{
    if (!h->use_graph) { CS3_HIP(body(st)); return CS3_OK; }
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        // bounded classes (the cache's policy above): graphs with the caller's X, per operation and trans
        const long bound = !std::get<3>(key) ? 0 : graph_op_is(key, GRAPH_SOLVE) ? 8 : 4;
        auto same_class = [&](const GraphKey &k) {
            return std::get<0>(k) == std::get<0>(key) && std::get<1>(k) == std::get<1>(key) && std::get<3>(k) != nullptr;
        };
        const long count = std::count_if(h->graphs.begin(), h->graphs.end(), [&](const auto &kv) { return same_class(kv.first); });
        if (bound && count >= bound)
            if (int rc = drop_graphs(h, same_class)) return rc;
        hipGraphExec_t exec = nullptr;
        if (int rc = capture(h, &exec, body)) return rc;
        it = h->graphs.emplace(key, exec).first;
    }
    CS3_HIP(hipGraphLaunch(it->second, st));
    return CS3_OK;
}

// The sweeps of one call: launch groups and their descriptors.  One right-hand side on a handle with a bottom forest
// follows the factor schedule (the forest, then the levels above it) with descriptors of its own.  (The forest's sweeps
// have no transposed form: a transposed solve takes the level schedule whatever nrhs is.)
SweepCall select_sweep_schedule(cs3_handle h, int nrhs, bool trans = false)
{
    const bool forest = nrhs == 1 && !trans && !h->S.sub_forest.empty();
    SweepCall c;
    c.groups = forest ? &h->S.sgroups1 : &h->S.sgroups;
    c.sd = forest ? h->D.sdesc1 : h->D.sdesc;
    c.trans = trans;
    return c;
}

int run_factor(cs3_handle h, const double *ax_dev, double tol, hipStream_t st)
{
    const DeviceFactor &D = h->D;
    const double inv_tol = (tol > 0.0) ? 1.0 / tol : HUGE_VAL;
    CS3_HIP(launch_prologue(D, ax_dev, nullptr, 0, st));        // status 0x7f7f7f7f = clean, zeros, values
    if (h->factor_inv_tol != inv_tol) {
        if (int rc = drop_graphs(h, [](const GraphKey &k) { return graph_op_is(k, GRAPH_FACTOR); })) return rc;
        h->factor_inv_tol = inv_tol;
    }
    const SweepCall call;
    int rc = replay_or_run(h, GraphKey(GRAPH_FACTOR, false, 0, nullptr), st, [&](hipStream_t s) {
        return launch_factor_levels(D, call, h->S.groups, inv_tol, s, h->fj);
    });
    if (rc) return rc;
    h->factored = true;
    h->inverses_valid = false;
    return CS3_OK;
}

int read_status(cs3_handle h, hipStream_t st)
{
    int word[4] = {0, 0, 0, 0};
    CS3_HIP(hipMemcpyAsync(word, h->D.status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    if (word[3] != 0) {
        // a wait inside the step was given up: a wave of a shared elimination never saw the multipliers of its partner
        // (eliminate_pair in k_big_step / the shared fronts of the forest).  Whatever was computed behind that point is
        // not to be used.
        CS3_HIP(hipMemsetAsync(h->D.status + 3, 0, sizeof(int), st));
        h->factored = false;
        set_error("a hand-over between the waves of a shared elimination timed out: the factors and solutions of this step are not valid");
        return CS3_ERR_STATE;
    }
    const int col = word[0];
    if (col == 0x7f7f7f7f) { h->fail_col = -1; return CS3_OK; }
    h->fail_col = col;
    h->factored = false;
    if (h->S.kind == CS3_LU) {
        set_error("static diagonal pivot rejected (zero, non-finite or below tol) at pivot column " +
                  std::to_string(col));
        return CS3_ERR_PIVOT;
    }
    set_error("matrix is not positive definite at pivot column " + std::to_string(col));
    return CS3_ERR_NOT_SPD;
}

// mode 0: full solve with permutations; 1: lsolve only; 2: usolve only (in pivot order, on X itself).
// trans (LU): A' X = B; the forward sweep solves with U', the backward sweep with L' (mode 1: utsolve, 2: ltsolve).
// On a Cholesky handle A' = A and trans changes nothing.
int run_solve(cs3_handle h, double *x_dev, long long k, int mode, hipStream_t st, bool trans = false)
{
    if (!h->factored) { set_error("solve before a successful factorisation"); return CS3_ERR_STATE; }
    if (k < 1 || k > INT_MAX) { set_error("solve: bad number of right-hand sides"); return CS3_ERR_ARG; }
    int rc = ensure_rhs_capacity(h, k);
    if (rc) return rc;
    const DeviceFactor &D = h->D;
    const int nrhs = (int) k;
    trans = trans && D.kind == CS3_LU;
    SweepCall call = select_sweep_schedule(h, nrhs, trans);
    if (nrhs >= 16 && D.n_inv_tasks > 0 && !h->inverses_valid) {      // many right-hand sides: GEMM sweeps need the inverted blocks
        CS3_HIP(launch_diag_inverses(D, st));
        h->inverses_valid = true;
    }
    if (mode != 0) {
        CS3_HIP(launch_solve_levels(D, call, x_dev, nrhs, mode == 1, st, h->fj));
        return CS3_OK;
    }
    // fused permutations: the forward sweep reads row q[k] of the caller's X, the backward sweep writes the solution rows
    // back there; X's address is baked into the graph
    const bool fused = permutation_can_fuse(D, nrhs);
    if (fused) call.xm = XMap{x_dev, x_dev, D.q};
    else CS3_HIP(launch_permute(D, x_dev, D.xp, nrhs, false, st));
    rc = replay_or_run(h, GraphKey(GRAPH_SOLVE, trans, nrhs, fused ? x_dev : nullptr), st, [&](hipStream_t s) {
        hipError_t e = launch_solve_levels(D, call, D.xp, nrhs, true, s, h->fj);
        return (e != hipSuccess) ? e : launch_solve_levels(D, call, D.xp, nrhs, false, s, h->fj);
    });
    if (rc) return rc;
    if (!fused) CS3_HIP(launch_permute(D, D.xp, x_dev, nrhs, true, st));
    return CS3_OK;
}

// numeric factorisation and full solve in one graph; the forward sweep runs beside the factorisation
int run_factor_solve(cs3_handle h, const double *ax_dev, const double *b_dev, double *x_dev, long long k, double tol, hipStream_t st)
{
    if (k < 1 || k > INT_MAX) { set_error("factor_solve: bad number of right-hand sides"); return CS3_ERR_ARG; }
    int rc = ensure_rhs_capacity(h, k);
    if (rc) return rc;
    const DeviceFactor &D = h->D;
    const int nrhs = (int) k;
    const double inv_tol = (tol > 0.0) ? 1.0 / tol : HUGE_VAL;
    SweepCall call = select_sweep_schedule(h, nrhs);
    call.fwd_in_factor = nrhs == 1 && !h->S.sub_forest.empty();   // the forest's factor launch carries its forward sweep
    call.inverses_in_sweep = true;                                 // the forward sweep inverts group by group
    CS3_HIP(launch_prologue(D, ax_dev, b_dev, nrhs, st));          // right-hand sides are read from b_dev, the solution goes to x_dev
    if (h->fused_inv_tol != inv_tol) {
        if ((rc = drop_graphs(h, [](const GraphKey &g) { return graph_op_is(g, GRAPH_FUSED); }))) return rc;
        h->fused_inv_tol = inv_tol;
    }
    h->fused_same_x = (x_dev == h->fused_last_x) ? h->fused_same_x + 1 : 0;
    h->fused_last_x = x_dev;
    const bool per_x = h->fused_same_x >= 2;                       // third call in a row with this X: its own graph, permutation included
    rc = replay_or_run(h, GraphKey(GRAPH_FUSED, false, nrhs, per_x ? x_dev : nullptr), st, [&](hipStream_t s) {
        hipError_t e = launch_factor_with_forward(D, call, h->S.groups, inv_tol, D.xp, nrhs, s, h->fj);
        if (e == hipSuccess) e = launch_solve_levels(D, call, D.xp, nrhs, false, s, h->fj);
        if (e == hipSuccess && per_x) e = launch_permute(D, D.xp, x_dev, nrhs, true, s);
        return e;
    });
    if (rc) return rc;
    if (!per_x) CS3_HIP(launch_permute(D, D.xp, x_dev, nrhs, true, st));
    h->factored = true;
    h->inverses_valid = nrhs >= 16;                                // a many-RHS fused call leaves them current
    return CS3_OK;
}

// What analyze() checks before it touches a pattern, for the stand-alone entry points: Ap[0] == 0, Ap monotone,
// 0 <= Ai < n (symmetrized_pattern and the etree walk index arrays of length n by Ai).
int check_pattern(const char *who, int64_t n, const int32_t *Ap, const int32_t *Ai)
{
    if (n < 0 || n >= ((int64_t) 1 << 30) || !Ap) { set_error(std::string(who) + ": bad size or null column pointers"); return CS3_ERR_ARG; }
    if (Ap[0] != 0) { set_error(std::string(who) + ": Ap[0] != 0"); return CS3_ERR_ARG; }
    for (int64_t j = 0; j < n; ++j)
        if (Ap[j + 1] < Ap[j]) { set_error(std::string(who) + ": Ap not monotone"); return CS3_ERR_ARG; }
    const int64_t nnz = n > 0 ? Ap[n] : 0;
    if (nnz > 0 && !Ai) { set_error(std::string(who) + ": null row indices"); return CS3_ERR_ARG; }
    for (int64_t p = 0; p < nnz; ++p)
        if (Ai[p] < 0 || Ai[p] >= n) { set_error(std::string(who) + ": row index out of range"); return CS3_ERR_ARG; }
    return CS3_OK;
}

int check_parent(const char *who, int64_t n, const int32_t *parent)
{
    for (int64_t j = 0; j < n; ++j)
        if (parent[j] < -1 || parent[j] >= n || parent[j] == j) { set_error(std::string(who) + ": parent index out of range"); return CS3_ERR_ARG; }
    return CS3_OK;
}

int guard(cs3_handle h)
{
    if (!h) { set_error("null handle"); return CS3_ERR_ARG; }
    return CS3_OK;
}

}  // namespace

extern "C" {

const char *cs3_last_error(void) { return g_error.c_str(); }

int cs3_version(void) { return 100; }

int cs3_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cs3_amd(int64_t order, int64_t m, int64_t n, const int32_t *Ap, const int32_t *Ai, int32_t *q)
{
    if (m != n || n < 0 || !Ap || !q) { set_error("cs3_amd: square pattern required"); return CS3_ERR_ARG; }
    if (int rc = check_pattern("cs3_amd", n, Ap, Ai)) return rc;
    try {
        if (order == CS3_ORDER_NATURAL) { for (int64_t k = 0; k < n; ++k) q[k] = (int32_t) k; return CS3_OK; }
        if (order != CS3_ORDER_AMD) { set_error("cs3_amd: order must be 0 or 1"); return CS3_ERR_ARG; }
        std::vector<i64> Cp;
        std::vector<i32> Ci;
        symmetrized_pattern(n, Ap, Ai, Cp, Ci);
        std::vector<i32> perm;
        amd_order(n, Cp, Ci, perm);
        std::memcpy(q, perm.data(), (size_t) n * sizeof(int32_t));
    } catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    return CS3_OK;
}

int cs3_etree(int64_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent)
{
    if (n < 0 || !Ap || !parent) { set_error("cs3_etree: null argument"); return CS3_ERR_ARG; }
    if (int rc = check_pattern("cs3_etree", n, Ap, Ai)) return rc;
    try { etree_upper(n, Ap, Ai, parent); }
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    return CS3_OK;
}

int cs3_post(int64_t n, const int32_t *parent, int32_t *post)
{
    if (n < 0 || !parent || !post) { set_error("cs3_post: null argument"); return CS3_ERR_ARG; }
    if (int rc = check_parent("cs3_post", n, parent)) return rc;
    try { tree_postorder(n, parent, post); }
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    return CS3_OK;
}

int cs3_counts(int64_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *parent,
               const int32_t *post, int32_t *colcount)
{
    if (n < 0 || !Ap || !parent || !post || !colcount) { set_error("cs3_counts: null argument"); return CS3_ERR_ARG; }
    if (int rc = check_pattern("cs3_counts", n, Ap, Ai)) return rc;
    if (int rc = check_parent("cs3_counts", n, parent)) return rc;
    for (int64_t k = 0; k < n; ++k)
        if (post[k] < 0 || post[k] >= n) { set_error("cs3_counts: postorder index out of range"); return CS3_ERR_ARG; }
    try { cholesky_counts(n, Ap, Ai, parent, post, colcount); }
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    return CS3_OK;
}

int cs3_analyze(int64_t kind, int64_t order, int64_t n, const int32_t *Ap, const int32_t *Ai,
                const int32_t *q_given, int64_t batch, cs3_handle *out)
{
    if (!out) { set_error("cs3_analyze: null output"); return CS3_ERR_ARG; }
    *out = nullptr;
    if (batch < 1) { set_error("cs3_analyze: batch must be >= 1"); return CS3_ERR_ARG; }
    cs3_handle h = nullptr;
    try {
        h = new cs3_handle_s();
        h->batch = batch;
        analyze((int) kind, (int) order, n, Ap, Ai, q_given, h->S, batch);
        h->Ap_host.assign(Ap, Ap + n + 1);
        h->Ai_host.assign(Ai, Ai + (n > 0 ? Ap[n] : 0));
    } catch (const std::bad_alloc &) {
        delete h; set_error("cs3_analyze: out of memory"); return CS3_ERR_ALLOC;
    } catch (const std::exception &e) {
        delete h; set_error(e.what()); return CS3_ERR_ARG;
    }
    *out = h;
    return CS3_OK;
}

int cs3_free(cs3_handle h)
{
    if (!h) return CS3_OK;
    if (h->on_device) {
        (void) hipDeviceSynchronize();
        release_device(h);
    }
    for (cs3_updates_s *u : h->plans) u->h = nullptr;      // (their device arrays went with release_device)
    delete h;
    return CS3_OK;
}

int cs3_get_info(cs3_handle h, cs3_info *info)
{
    int rc = guard(h); if (rc) return rc;
    if (!info) { set_error("cs3_get_info: null output"); return CS3_ERR_ARG; }
    const Symbolic &S = h->S;
    info->n = S.n; info->nnz_a = S.nnzA;
    info->nnz_l = S.nnz_l;
    info->nnz_u = S.nnz_u;
    info->nsuper = S.nsuper; info->nlevels = S.nlevels;
    info->max_front = S.max_front; info->max_width = S.max_width;
    info->factor_bytes = S.vals_size * (int64_t) sizeof(double);
    info->update_bytes = S.cb_size * (int64_t) sizeof(double);
    info->batch = h->batch;
    info->fail_col = h->fail_col;
    info->flops_factor = S.flops;
    info->t_order_s = S.t_order; info->t_symbolic_s = S.t_symbolic;
    return CS3_OK;
}

int cs3_get_ordering(cs3_handle h, int32_t *q_amd, int32_t *parent, int32_t *post, int32_t *colcount,
                     int32_t *q, int32_t *pinv)
{
    int rc = guard(h); if (rc) return rc;
    const Symbolic &S = h->S;
    const size_t bytes = (size_t) S.n * sizeof(int32_t);
    if (q_amd) std::memcpy(q_amd, S.q_amd.data(), bytes);
    if (parent) std::memcpy(parent, S.parent_amd.data(), bytes);
    if (post) std::memcpy(post, S.post_amd.data(), bytes);
    if (colcount) std::memcpy(colcount, S.count_amd.data(), bytes);
    if (q) std::memcpy(q, S.q.data(), bytes);
    if (pinv) std::memcpy(pinv, S.pinv.data(), bytes);
    return CS3_OK;
}

int cs3_get_supernodes(cs3_handle h, int32_t *sn_ptr, int32_t *sn_parent, int32_t *sn_level)
{
    int rc = guard(h); if (rc) return rc;
    const Symbolic &S = h->S;
    if (sn_ptr) std::memcpy(sn_ptr, S.sn_ptr.data(), (size_t) (S.nsuper + 1) * sizeof(int32_t));
    if (sn_parent) std::memcpy(sn_parent, S.sn_parent.data(), (size_t) S.nsuper * sizeof(int32_t));
    if (sn_level) std::memcpy(sn_level, S.sn_level.data(), (size_t) S.nsuper * sizeof(int32_t));
    return CS3_OK;
}

int cs3_factor_dev(cs3_handle h, const double *Ax_dev, double tol, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!Ax_dev && h->S.nnzA > 0) { set_error("cs3_factor_dev: null values"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    return run_factor(h, Ax_dev, tol, (hipStream_t) stream);
}

int cs3_factor_solve_dev(cs3_handle h, const double *Ax_dev, double tol, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if ((!Ax_dev && h->S.nnzA > 0) || !X_dev) { set_error("cs3_factor_solve_dev: null argument"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    return run_factor_solve(h, Ax_dev, X_dev, X_dev, k, tol, (hipStream_t) stream);
}

int cs3_factor_solve_bx_dev(cs3_handle h, const double *Ax_dev, double tol, const double *B_dev, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if ((!Ax_dev && h->S.nnzA > 0) || !B_dev || !X_dev) { set_error("cs3_factor_solve_bx_dev: null argument"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    return run_factor_solve(h, Ax_dev, B_dev, X_dev, k, tol, (hipStream_t) stream);
}

int cs3_factor_status(cs3_handle h, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!h->on_device) { set_error("cs3_factor_status: nothing factorised yet"); return CS3_ERR_STATE; }
    return read_status(h, (hipStream_t) stream);
}

int cs3_factor(cs3_handle h, const double *Ax, double tol)
{
    int rc = guard(h); if (rc) return rc;
    if (!Ax && h->S.nnzA > 0) { set_error("cs3_factor: null values"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    const size_t count = (size_t) (h->batch * h->S.nnzA);
    if (count) CS3_HIP(hipMemcpy(h->D.ax, Ax, count * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run_factor(h, h->D.ax, tol, nullptr))) return rc;
    return read_status(h, nullptr);
}

int cs3_solve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve(h, X_dev, k, 0, (hipStream_t) stream);
}

int cs3_lsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve(h, X_dev, k, 1, (hipStream_t) stream);
}

int cs3_usolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve(h, X_dev, k, 2, (hipStream_t) stream);
}

// Transposed solves: mode as in run_solve (1: U' \ x, 2: L' \ x).  A Cholesky handle has no U: utsolve is refused,
// ltsolve is L' \ x (its usolve), the full solve is the plain one.
static int run_solve_t(cs3_handle h, double *x_dev, long long k, int mode, hipStream_t st)
{
    if (mode == 1 && h->S.kind != CS3_LU) { set_error("utsolve: a Cholesky factorisation has no U"); return CS3_ERR_ARG; }
    return run_solve(h, x_dev, k, mode, st, true);
}

int cs3_solve_t_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve_t(h, X_dev, k, 0, (hipStream_t) stream);
}

int cs3_utsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve_t(h, X_dev, k, 1, (hipStream_t) stream);
}

int cs3_ltsolve_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_solve_t(h, X_dev, k, 2, (hipStream_t) stream);
}

static int solve_host(cs3_handle h, double *X, int64_t k, int mode, bool trans = false)
{
    int rc = guard(h); if (rc) return rc;
    if (!X) { set_error("solve: null right-hand side"); return CS3_ERR_ARG; }
    if (trans && mode == 1 && h->S.kind != CS3_LU) { set_error("utsolve: a Cholesky factorisation has no U"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("solve before a successful factorisation"); return CS3_ERR_STATE; }
    const size_t bytes = (size_t) (h->batch * h->S.n * k) * sizeof(double);
    double *d_x = nullptr;
    CS3_HIP(hipMalloc((void **) &d_x, std::max<size_t>(bytes, 8)));
    hipError_t e = hipMemcpy(d_x, X, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = trans ? run_solve_t(h, d_x, k, mode, nullptr) : run_solve(h, d_x, k, mode, nullptr);
        if (rc == CS3_OK) e = hipMemcpy(X, d_x, bytes, hipMemcpyDeviceToHost);
    }
    (void) hipFree(d_x);
    if (rc) return rc;
    CS3_HIP(e);
    return CS3_OK;
}

int cs3_solve(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 0); }
int cs3_lsolve(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 1); }
int cs3_usolve(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 2); }
int cs3_solve_t(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 0, true); }
int cs3_utsolve(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 1, true); }
int cs3_ltsolve(cs3_handle h, double *X, int64_t k) { return solve_host(h, X, k, 2, true); }

int cs3_export_factor_dev(cs3_handle h, double *dst_dev, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!h->factored) { set_error("cs3_export_factor_dev: nothing factorised"); return CS3_ERR_STATE; }
    if (!dst_dev) { set_error("cs3_export_factor_dev: null buffer"); return CS3_ERR_ARG; }
    const DeviceFactor &D = h->D;
    if (D.il_len > 0) { set_error("cs3_export_factor_dev: not available for a matrix-interleaved batch (64 or more matrices)"); return CS3_ERR_STATE; }
    if (D.vals_size > 0)
        CS3_HIP(hipMemcpy2DAsync(dst_dev, (size_t) D.vals_size * sizeof(double), D.pool,
                                 (size_t) D.pool_size * sizeof(double), (size_t) D.vals_size * sizeof(double),
                                 (size_t) D.batch, hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_import_factor_dev(cs3_handle h, const double *src_dev, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!src_dev) { set_error("cs3_import_factor_dev: null buffer"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    const DeviceFactor &D = h->D;
    if (D.il_len > 0) { set_error("cs3_import_factor_dev: not available for a matrix-interleaved batch (64 or more matrices)"); return CS3_ERR_STATE; }
    if (D.vals_size > 0)
        CS3_HIP(hipMemcpy2DAsync(D.pool, (size_t) D.pool_size * sizeof(double), src_dev,
                                 (size_t) D.vals_size * sizeof(double), (size_t) D.vals_size * sizeof(double),
                                 (size_t) D.batch, hipMemcpyDeviceToDevice, (hipStream_t) stream));
    h->factored = true;
    h->inverses_valid = false;
    h->fail_col = -1;
    return CS3_OK;
}

int cs3_debug_poison_lds(void *stream)
{
    CS3_HIP(launch_poison_lds((hipStream_t) stream));
    return CS3_OK;
}

int cs3_debug_schedule(cs3_handle h, int32_t *sched, int32_t *front_r, int32_t *front_w)
{
    int rc = guard(h); if (rc) return rc;
    const Symbolic &S = h->S;
    for (i32 t = 0; t < S.nsuper; ++t) {
        const i32 s = S.sched[t];
        if (sched) sched[t] = s;
        if (front_r) front_r[t] = (i32) (S.st_ptr[s + 1] - S.st_ptr[s]);
        if (front_w) front_w[t] = S.sn_ptr[s + 1] - S.sn_ptr[s];
    }
    return CS3_OK;
}

int64_t cs3_debug_forest(cs3_handle h, int32_t *supernode, int32_t *task, int32_t *level, int32_t *tier)
{
    if (guard(h)) return -1;
    const Symbolic &S = h->S;
    for (i32 k = 0; k < (i32) S.sub_tasks.size(); ++k) {
        const SubTask &K = S.sub_tasks[k];
        for (i32 l = 0; l < K.nlevels; ++l)
            for (i32 f = K.front0 + S.sub_lvl[K.lvl0 + 2 * l]; f < K.front0 + S.sub_lvl[K.lvl0 + 2 * l + 2]; ++f) {
                if (supernode) supernode[f] = S.sub_sn[f];
                if (task) task[f] = k;
                if (level) level[f] = l;
                if (tier) tier[f] = 0;
            }
    }
    return (int64_t) S.sub_sn.size();
}

int cs3_debug_withhold_handover(int on)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("cs3_debug_withhold_handover: no HIP device"); return CS3_ERR_HIP; }
    CS3_HIP(hipDeviceSynchronize());
    CS3_HIP(set_withhold_handover(on ? 1 : 0));
    return CS3_OK;
}

int cs3_debug_front_stamps(cs3_handle h, int64_t *out)
{
    int rc = guard(h); if (rc) return rc;
    if (!h->on_device || !h->D.tbuf) { set_error("cs3_debug_front_stamps: run with CS3_PROFILE=1"); return CS3_ERR_STATE; }
    CS3_HIP(hipDeviceSynchronize());
    CS3_HIP(hipMemcpy(out, h->D.tbuf, (size_t) h->S.nsuper * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_get_factors(cs3_handle h, int64_t b, int32_t *Lp, int32_t *Li, double *Lx,
                    int32_t *Up, int32_t *Ui, double *Ux)
{
    int rc = guard(h); if (rc) return rc;
    const Symbolic &S = h->S;
    if (b < 0 || b >= h->batch) { set_error("cs3_get_factors: batch index out of range"); return CS3_ERR_ARG; }
    if (S.kind == CS3_CHOLESKY && (Up || Ui || Ux)) { set_error("cs3_get_factors: Cholesky has no U"); return CS3_ERR_ARG; }
    try { build_csc_factors(h->S); }                           // (first request: the CSC view of the factors is built now)
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    const i64 lnz = S.Lp[S.n];
    if (Lp) std::memcpy(Lp, S.Lp.data(), (size_t) (S.n + 1) * sizeof(int32_t));
    if (Li) std::memcpy(Li, S.Li.data(), (size_t) lnz * sizeof(int32_t));
    const i64 unz = (S.kind == CS3_LU) ? S.Up[S.n] : 0;
    if (Up) std::memcpy(Up, S.Up.data(), (size_t) (S.n + 1) * sizeof(int32_t));
    if (Ui) std::memcpy(Ui, S.Ui.data(), (size_t) unz * sizeof(int32_t));
    if (!Lx && !Ux) return CS3_OK;
    if (!h->factored) { set_error("cs3_get_factors: values requested before a successful factorisation"); return CS3_ERR_STATE; }
    const DeviceFactor &DD = h->D;
    const double *vals = DD.pool_pm + b * DD.pm_stride;                                   // per-matrix part (virtual offsets)
    const double *vals_il = DD.pool_il + (b / 64) * 64 * DD.il_len + (b % 64);          // interleaved part, stride 64
    if (Lx) {
        if (!h->d_lmap) { if ((rc = upload(&h->d_lmap, S.Lmap))) return rc; }
        if (!h->d_lx) CS3_HIP(hipMalloc((void **) &h->d_lx, std::max<size_t>(1, (size_t) lnz) * sizeof(double)));
        CS3_HIP(launch_extract(vals, vals_il, DD.il_len, (const long long *) h->d_lmap, h->d_lx, lnz, nullptr));
        CS3_HIP(hipMemcpy(Lx, h->d_lx, (size_t) lnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (Ux) {
        if (!h->d_umap) { if ((rc = upload(&h->d_umap, S.Umap))) return rc; }
        if (!h->d_ux) CS3_HIP(hipMalloc((void **) &h->d_ux, std::max<size_t>(1, (size_t) unz) * sizeof(double)));
        CS3_HIP(launch_extract(vals, vals_il, DD.il_len, (const long long *) h->d_umap, h->d_ux, unz, nullptr));
        CS3_HIP(hipMemcpy(Ux, h->d_ux, (size_t) unz * sizeof(double), hipMemcpyDeviceToHost));
    }
    return CS3_OK;
}

// trans: x = G' \ x on the same arrays
static int csc_trisolve(int64_t n, const int32_t *Gp, const int32_t *Gi, const double *Gx, double *x,
                        int64_t k, bool lower, bool trans = false)
{
    if (n < 0 || k < 1 || k > INT_MAX || !Gp || !x) { set_error("triangular solve: bad argument"); return CS3_ERR_ARG; }
    if (n == 0) return CS3_OK;
    if (int rc = check_pattern("triangular solve", n, Gp, Gi)) return rc;
    if (!Gx) { set_error("triangular solve: null values"); return CS3_ERR_ARG; }
    TriSchedule T;
    try { tri_schedule(n, Gp, Gi, lower, T, trans); }
    catch (const std::bad_alloc &) { set_error("triangular solve: out of memory"); return CS3_ERR_ALLOC; }
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: triangular solves run on the GPU only"); return CS3_ERR_HIP;
    }
    int *d_rows = nullptr, *d_rp = nullptr, *d_rj = nullptr;
    long long *d_rmap = nullptr, *d_diag = nullptr;
    double *d_gx = nullptr, *d_x = nullptr;
    int rc = CS3_OK;
    auto cleanup = [&]() {
        void *ptrs[] = {d_rows, d_rp, d_rj, d_rmap, d_diag, d_gx, d_x};
        for (void *p : ptrs) if (p) (void) hipFree(p);
    };
    std::vector<long long> rmap(T.Rmap.begin(), T.Rmap.end()), diag(T.diag.begin(), T.diag.end());
    std::vector<double> gx(Gx, Gx + Gp[n]);
    if ((rc = upload(&d_rows, T.level_rows)) || (rc = upload(&d_rp, T.Rp)) || (rc = upload(&d_rj, T.Rj)) ||
        (rc = upload(&d_rmap, rmap)) || (rc = upload(&d_diag, diag)) || (rc = upload(&d_gx, gx))) {
        cleanup(); return rc;
    }
    const size_t xbytes = (size_t) (n * k) * sizeof(double);
    hipError_t e = hipMalloc((void **) &d_x, xbytes);
    if (e == hipSuccess) e = hipMemcpy(d_x, x, xbytes, hipMemcpyHostToDevice);
    for (i32 l = 0; l < T.nlevels && e == hipSuccess; ++l)
        e = launch_tri_level(d_rows + T.level_ptr[l], T.level_ptr[l + 1] - T.level_ptr[l], d_rp, d_rj, d_rmap,
                             d_diag, d_gx, d_x, (int) k, nullptr);
    if (e == hipSuccess) e = hipMemcpy(x, d_x, xbytes, hipMemcpyDeviceToHost);
    cleanup();
    CS3_HIP(e);
    return CS3_OK;
}

int cs3_csc_lsolve(int64_t n, const int32_t *Lp, const int32_t *Li, const double *Lx, double *x, int64_t k)
{
    return csc_trisolve(n, Lp, Li, Lx, x, k, true);
}

int cs3_csc_usolve(int64_t n, const int32_t *Up, const int32_t *Ui, const double *Ux, double *x, int64_t k)
{
    return csc_trisolve(n, Up, Ui, Ux, x, k, false);
}

int cs3_csc_ltsolve(int64_t n, const int32_t *Lp, const int32_t *Li, const double *Lx, double *x, int64_t k)
{
    return csc_trisolve(n, Lp, Li, Lx, x, k, true, true);
}

int cs3_csc_utsolve(int64_t n, const int32_t *Up, const int32_t *Ui, const double *Ux, double *x, int64_t k)
{
    return csc_trisolve(n, Up, Ui, Ux, x, k, false, true);
}

int cs3_csc_matvec(int64_t m, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                   const double *X, double *Y, int64_t k)
{
    if (m < 0 || n < 0 || k < 1 || k > INT_MAX || !Ap || !X || !Y) { set_error("cs3_csc_matvec: bad argument"); return CS3_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: cs3_csc_matvec runs on the GPU only"); return CS3_ERR_HIP;
    }
    const i64 nnz = Ap[n];
    // row view with ascending columns: the summation order of the column scatter loop
    std::vector<int> Rp(m + 1, 0), Rj(nnz);
    std::vector<double> Rx(nnz);
    for (i64 p = 0; p < nnz; ++p) {
        if (Ai[p] < 0 || Ai[p] >= m) { set_error("cs3_csc_matvec: row index out of range"); return CS3_ERR_ARG; }
        ++Rp[Ai[p] + 1];
    }
    for (i64 i = 0; i < m; ++i) Rp[i + 1] += Rp[i];
    {
        std::vector<int> fill(Rp.begin(), Rp.end() - 1);
        for (i64 j = 0; j < n; ++j)
            for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) { int q = fill[Ai[p]]++; Rj[q] = (int) j; Rx[q] = Ax[p]; }
    }
    int *d_rp = nullptr, *d_rj = nullptr;
    double *d_rx = nullptr, *d_x = nullptr, *d_y = nullptr;
    auto cleanup = [&]() {
        void *ptrs[] = {d_rp, d_rj, d_rx, d_x, d_y};
        for (void *p : ptrs) if (p) (void) hipFree(p);
    };
    int rc;
    if ((rc = upload(&d_rp, Rp)) || (rc = upload(&d_rj, Rj)) || (rc = upload(&d_rx, Rx))) { cleanup(); return rc; }
    hipError_t e = hipMalloc((void **) &d_x, std::max<size_t>(8, (size_t) (n * k) * sizeof(double)));
    if (e == hipSuccess) e = hipMalloc((void **) &d_y, std::max<size_t>(8, (size_t) (m * k) * sizeof(double)));
    if (e == hipSuccess) e = hipMemcpy(d_x, X, (size_t) (n * k) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_matvec_rows(d_rp, d_rj, d_rx, d_x, d_y, m, (int) k, nullptr);
    if (e == hipSuccess) e = hipMemcpy(Y, d_y, (size_t) (m * k) * sizeof(double), hipMemcpyDeviceToHost);
    cleanup();
    CS3_HIP(e);
    return CS3_OK;
}

int cs3_csc_stack_4_by_4(int64_t am, int64_t an, const int32_t *Ai, const int32_t *Ap, const double *Ax,
                         int64_t bm, int64_t bn, const int32_t *Bi, const int32_t *Bp, const double *Bx,
                         int64_t cm, int64_t cn, const int32_t *Ci, const int32_t *Cp, const double *Cx,
                         int64_t dm, int64_t dn, const int32_t *Di, const int32_t *Dp, const double *Dx,
                         int32_t *Pi, int32_t *Pp, double *Px)
{
    // the reference asserts these (csc_numba.py:679-682)
    if (am != bm || cm != dm || an != cn || bn != dn) { set_error("cs3_csc_stack_4_by_4: incompatible block shapes"); return CS3_ERR_ARG; }
    if (!Ap || !Bp || !Cp || !Dp || !Pp) { set_error("cs3_csc_stack_4_by_4: null argument"); return CS3_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: cs3_csc_stack_4_by_4 runs on the GPU only"); return CS3_ERR_HIP;
    }
    const i64 nnz = (i64) Ap[an] + Bp[bn] + Cp[cn] + Dp[dn];
    struct Blk { const int32_t *p, *i; const double *x; i64 n; int *dp = nullptr, *di = nullptr; double *dx = nullptr; };
    Blk blk[4] = {{Ap, Ai, Ax, an}, {Bp, Bi, Bx, bn}, {Cp, Ci, Cx, cn}, {Dp, Di, Dx, dn}};
    int *d_pp = nullptr, *d_pi = nullptr; double *d_px = nullptr;
    auto cleanup = [&]() {
        for (Blk &b : blk) { if (b.dp) (void) hipFree(b.dp); if (b.di) (void) hipFree(b.di); if (b.dx) (void) hipFree(b.dx); }
        if (d_pp) (void) hipFree(d_pp); if (d_pi) (void) hipFree(d_pi); if (d_px) (void) hipFree(d_px);
    };
    hipError_t e = hipSuccess;
    for (Blk &b : blk) {
        const size_t bn_ = (size_t) b.p[b.n];
        if (e == hipSuccess) e = hipMalloc((void **) &b.dp, (size_t) (b.n + 1) * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void **) &b.di, std::max<size_t>(1, bn_) * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void **) &b.dx, std::max<size_t>(1, bn_) * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(b.dp, b.p, (size_t) (b.n + 1) * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && bn_) e = hipMemcpy(b.di, b.i, bn_ * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && bn_) e = hipMemcpy(b.dx, b.x, bn_ * sizeof(double), hipMemcpyHostToDevice);
    }
    const i64 ncol = an + bn;
    if (e == hipSuccess) e = hipMalloc((void **) &d_pp, (size_t) (ncol + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **) &d_pi, std::max<size_t>(1, (size_t) nnz) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **) &d_px, std::max<size_t>(1, (size_t) nnz) * sizeof(double));
    if (e == hipSuccess) e = hipMemset(d_pp, 0, (size_t) (ncol + 1) * sizeof(int));
    if (e == hipSuccess)
        e = launch_stack_4_by_4((int) an, (int) bn, (int) am, (int) bm, blk[0].dp, blk[0].di, blk[0].dx, blk[1].dp, blk[1].di,
                                blk[1].dx, blk[2].dp, blk[2].di, blk[2].dx, blk[3].dp, blk[3].di, blk[3].dx, d_pp, d_pi, d_px,
                                nullptr, nullptr);
    if (e == hipSuccess) e = hipMemcpy(Pp, d_pp, (size_t) (ncol + 1) * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && nnz) e = hipMemcpy(Pi, d_pi, (size_t) nnz * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && nnz) e = hipMemcpy(Px, d_px, (size_t) nnz * sizeof(double), hipMemcpyDeviceToHost);
    cleanup();
    CS3_HIP(e);
    return CS3_OK;
}

// ---- residual and iterative refinement on resident data ---------------------------------
static int ensure_row_view(cs3_handle h, long long k)
{
    int rc = ensure_device(h);
    if (rc) return rc;
    const Symbolic &S = h->S;
    if (!h->d_rp) {
        const i64 n = S.n, nnz = S.nnzA;
        std::vector<int> Rp(n + 1, 0), Rj(nnz), Rmap(nnz);
        const i32 *Ap = h->Ap_host.data(), *Ai = h->Ai_host.data();
        for (i64 p = 0; p < nnz; ++p) ++Rp[Ai[p] + 1];
        for (i64 i = 0; i < n; ++i) Rp[i + 1] += Rp[i];
        std::vector<int> fill(Rp.begin(), Rp.end() - 1);
        for (i64 j = 0; j < n; ++j)                      // ascending column inside every row: csc_mat_vec_ff's summation order
            for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) { const int q = fill[Ai[p]]++; Rj[q] = (int) j; Rmap[q] = (int) p; }
        if ((rc = upload(&h->d_rp, Rp)) || (rc = upload(&h->d_rj, Rj)) || (rc = upload(&h->d_rmap, Rmap))) return rc;
        CS3_HIP(hipMalloc((void **) &h->d_maxbits, sizeof(unsigned long long)));
    }
    const long long need = h->batch * S.n * k;
    if (need > h->res_cap) {
        CS3_HIP(hipDeviceSynchronize());
        if (h->d_res) (void) hipFree(h->d_res);
        h->d_res = nullptr; h->res_cap = 0;
        CS3_HIP(hipMalloc((void **) &h->d_res, std::max<size_t>(8, (size_t) need * sizeof(double))));
        h->res_cap = need;
    }
    return CS3_OK;
}

// The analysed pattern in column view for the transposed products: row j of A' = column j of A, in storage order
static int ensure_col_view(cs3_handle h, long long k)
{
    int rc = ensure_row_view(h, k);
    if (rc) return rc;
    if (!h->d_cp) {
        std::vector<int> Cmap(h->S.nnzA);
        for (i64 p = 0; p < h->S.nnzA; ++p) Cmap[p] = (int) p;
        if ((rc = upload(&h->d_cp, h->Ap_host)) || (rc = upload(&h->d_ci, h->Ai_host)) || (rc = upload(&h->d_cmap, Cmap))) return rc;
    }
    return CS3_OK;
}

// R = B - A X (B null: Y = A X) on resident data; trans: with A', through the column view.  The products of a row are
// summed in csc_mat_vec_ff's order (bit-exact with cs3_csc_matvec).
static int product(const char *who, cs3_handle h, const double *Ax_dev, const double *B_dev, bool with_b, const double *X_dev,
                   double *R_dev, int64_t k, void *stream, bool trans)
{
    int rc = guard(h); if (rc) return rc;
    if (!Ax_dev || (with_b && !B_dev) || !X_dev || !R_dev || k < 1 || k > INT_MAX) { set_error(std::string(who) + ": bad argument"); return CS3_ERR_ARG; }
    if ((rc = trans ? ensure_col_view(h, 0) : ensure_row_view(h, 0))) return rc;
    const int *vp = trans ? h->d_cp : h->d_rp, *vj = trans ? h->d_ci : h->d_rj, *vmap = trans ? h->d_cmap : h->d_rmap;
    CS3_HIP(launch_residual(vp, vj, vmap, Ax_dev, X_dev, B_dev, R_dev, h->S.n, (int) k, h->S.nnzA, h->batch, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_residual_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, double *R_dev, int64_t k, void *stream)
{
    return product("cs3_residual_dev", h, Ax_dev, B_dev, true, X_dev, R_dev, k, stream, false);
}

int cs3_matvec_dev(cs3_handle h, const double *Ax_dev, const double *X_dev, double *Y_dev, int64_t k, void *stream)
{
    return product("cs3_matvec_dev", h, Ax_dev, nullptr, false, X_dev, Y_dev, k, stream, false);
}

int cs3_residual_t_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, double *R_dev, int64_t k, void *stream)
{
    return product("cs3_residual_t_dev", h, Ax_dev, B_dev, true, X_dev, R_dev, k, stream, true);
}

int cs3_matvec_t_dev(cs3_handle h, const double *Ax_dev, const double *X_dev, double *Y_dev, int64_t k, void *stream)
{
    return product("cs3_matvec_t_dev", h, Ax_dev, nullptr, false, X_dev, Y_dev, k, stream, true);
}

static int refine(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t steps,
                  double *last_correction, void *stream, bool trans)
{
    const char *who = trans ? "cs3_refine_t_dev" : "cs3_refine_dev";
    int rc = guard(h); if (rc) return rc;
    if (!Ax_dev || !B_dev || !X_dev || k < 1 || k > INT_MAX || steps < 0) { set_error(std::string(who) + ": bad argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": refinement needs a factorisation"); return CS3_ERR_STATE; }
    if ((rc = trans ? ensure_col_view(h, k) : ensure_row_view(h, k))) return rc;
    hipStream_t st = (hipStream_t) stream;
    const long long total = h->batch * h->S.n * k;
    const int *vp = trans ? h->d_cp : h->d_rp, *vj = trans ? h->d_ci : h->d_rj, *vmap = trans ? h->d_cmap : h->d_rmap;
    for (int64_t s = 0; s < steps; ++s) {
        CS3_HIP(launch_residual(vp, vj, vmap, Ax_dev, X_dev, B_dev, h->d_res, h->S.n, (int) k, h->S.nnzA, h->batch, st));
        if ((rc = run_solve(h, h->d_res, k, 0, st, trans))) return rc;    // d = A \ r (A' \ r) with the factors at hand
        const bool want = last_correction && s + 1 == steps;
        if (want) CS3_HIP(hipMemsetAsync(h->d_maxbits, 0, sizeof(unsigned long long), st));
        CS3_HIP(launch_axpy_max(X_dev, h->d_res, total, want ? h->d_maxbits : nullptr, st));      // x += d
        if (want) {
            unsigned long long bits = 0;
            CS3_HIP(hipMemcpyAsync(&bits, h->d_maxbits, sizeof(bits), hipMemcpyDeviceToHost, st));
            CS3_HIP(hipStreamSynchronize(st));
            std::memcpy(last_correction, &bits, sizeof(double));
        }
    }
    if (steps == 0 && last_correction) *last_correction = 0.0;
    return CS3_OK;
}

int cs3_refine_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t steps,
                   double *last_correction, void *stream)
{
    return refine(h, Ax_dev, B_dev, X_dev, k, steps, last_correction, stream, false);
}

int cs3_refine_t_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t steps,
                     double *last_correction, void *stream)
{
    return refine(h, Ax_dev, B_dev, X_dev, k, steps, last_correction, stream, true);
}

// ---- condition estimates and log-determinants from the held factors --------------------------------------------------
static int ensure_estimator(cs3_handle h)
{
    int rc = ensure_col_view(h, 0);
    if (rc) return rc;
    const size_t bn = std::max<size_t>(1, (size_t) (h->batch * h->S.n));
    if (!h->d_est_x) CS3_HIP(hipMalloc((void **) &h->d_est_x, bn * sizeof(double)));
    if (!h->d_est_s) CS3_HIP(hipMalloc((void **) &h->d_est_s, 2 * bn));
    if (!h->d_est_state) CS3_HIP(hipMalloc((void **) &h->d_est_state, (size_t) h->batch * sizeof(EstState)));
    const long long nparts = std::max(est_chunks(h->S.n), norm_chunks(h->S.n));
    if (!h->d_est_parts) CS3_HIP(hipMalloc((void **) &h->d_est_parts, (size_t) (h->batch * nparts) * sizeof(EstPart)));
    if (!h->d_est_cnt) CS3_HIP(hipMalloc((void **) &h->d_est_cnt, 2 * sizeof(unsigned)));
    return CS3_OK;
}

// dlacn2 for every matrix of the batch in SLOTS (estimate.hip): prepare(kind), the handle's own solve of that kind on the
// work buffer (k = 1, run_solve mode 0: the cached graphs), consume(kind).  adaptive (cs3_condest): after every slot the
// two counters come back (8 bytes and a sync) and only a wanted kind runs, alternating when both are wanted -- one matrix
// gets exactly dlacn2's call sequence.  Otherwise (cs3_condest_dev) the fixed sequence F T F T F T F T F T F: enough for
// every path (J1, J2, four J3/J4 pairs, J5; a matrix that leaves J3 for J5 waits one slot at most), no synchronisation.
// A Cholesky slot serves both kinds (A' = A).  Both drivers give the same bits: a solve of the batch computes every matrix
// on its own, an idle matrix gets zeros and keeps its state.
static int condest_run(cs3_handle h, const double *Ax_dev, double *cond_dev, double *inv_dev, hipStream_t st, bool adaptive)
{
    int rc = ensure_estimator(h);
    if (rc) return rc;
    const i64 n = h->S.n, batch = h->batch;
    const bool chol = h->S.kind == CS3_CHOLESKY;
    CS3_HIP(launch_est_start(h->d_cp, h->d_cmap, Ax_dev, n, h->S.nnzA, batch, h->d_est_parts, h->d_est_state, st));
    constexpr int FIXED_SLOTS = 11;
    unsigned want[2] = {1u, 0u};                             // before the first slot: J1 wants A^-1
    int last = 1;
    // (adaptive: a wanted kind runs at most one slot late, so 2 * 11 slots bound every matrix's 11 steps)
    for (int slot = 0; slot < (adaptive ? 2 * FIXED_SLOTS : FIXED_SLOTS); ++slot) {
        int kind = slot & 1;                                 // 0: x = A^-1 b (F), 1: x = A^-T b (T)
        if (adaptive) {
            if (slot > 0) {
                CS3_HIP(hipMemcpyAsync(want, h->d_est_cnt, sizeof(want), hipMemcpyDeviceToHost, st));
                CS3_HIP(hipStreamSynchronize(st));
            }
            if (!want[0] && !want[1]) break;
            kind = (want[0] && want[1]) ? 1 - last : (want[0] ? 0 : 1);
        }
        if (chol) kind = 0;
        const int kmask = chol ? 3 : 1 << kind;
        CS3_HIP(launch_est_prepare(h->d_est_state, h->d_est_s, h->d_est_x, n, batch, kmask, h->d_est_cnt, st));
        if ((rc = run_solve(h, h->d_est_x, 1, 0, st, kind == 1))) return rc;
        CS3_HIP(launch_est_consume(h->d_est_state, h->d_est_s, h->d_est_x, n, batch, kmask, h->d_est_parts, h->d_est_cnt, st));
        last = kind;
    }
    CS3_HIP(launch_est_finalize(h->d_est_state, batch, cond_dev, inv_dev, st));
    return CS3_OK;
}

static int condest_check(const char *who, cs3_handle h, const double *Ax, const double *cond)
{
    int rc = guard(h); if (rc) return rc;
    if (!Ax || !cond) { set_error(std::string(who) + ": null argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": no successful factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

int cs3_condest_dev(cs3_handle h, const double *Ax_dev, double *cond_dev, double *inv_norm_dev, void *stream)
{
    int rc = condest_check("cs3_condest_dev", h, Ax_dev, cond_dev);
    if (rc) return rc;
    hipStream_t st = (hipStream_t) stream;
    if (h->S.n == 0) {
        CS3_HIP(hipMemsetAsync(cond_dev, 0, (size_t) h->batch * sizeof(double), st));
        if (inv_norm_dev) CS3_HIP(hipMemsetAsync(inv_norm_dev, 0, (size_t) h->batch * sizeof(double), st));
        return CS3_OK;
    }
    return condest_run(h, Ax_dev, cond_dev, inv_norm_dev, st, false);
}

// The host forms stage through buffers the handle keeps (allocated on first use), on the null stream.
static int ensure_host_out(cs3_handle h)
{
    if (!h->d_est_out) CS3_HIP(hipMalloc((void **) &h->d_est_out, (size_t) (2 * h->batch) * sizeof(double)));
    return CS3_OK;
}

int cs3_condest(cs3_handle h, const double *Ax, double *cond, double *inv_norm)
{
    int rc = condest_check("cs3_condest", h, Ax, cond);
    if (rc) return rc;
    const long long batch = h->batch;
    if (h->S.n == 0) {
        for (long long b = 0; b < batch; ++b) { cond[b] = 0.0; if (inv_norm) inv_norm[b] = 0.0; }
        return CS3_OK;
    }
    if ((rc = ensure_host_out(h))) return rc;
    const size_t ax_bytes = (size_t) (batch * h->S.nnzA) * sizeof(double);
    if (!h->d_est_ax) CS3_HIP(hipMalloc((void **) &h->d_est_ax, std::max<size_t>(ax_bytes, 8)));
    if (ax_bytes) CS3_HIP(hipMemcpy(h->d_est_ax, Ax, ax_bytes, hipMemcpyHostToDevice));
    if ((rc = condest_run(h, h->d_est_ax, h->d_est_out, h->d_est_out + batch, nullptr, true))) return rc;
    std::vector<double> out((size_t) (2 * batch));
    CS3_HIP(hipMemcpy(out.data(), h->d_est_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(cond, out.data(), (size_t) batch * sizeof(double));
    if (inv_norm) std::memcpy(inv_norm, out.data() + batch, (size_t) batch * sizeof(double));
    return CS3_OK;
}

// sign and log|det| from the diagonal of the held factors: pivot j's diagonal sits at virtual pool offset
// lpan_off[s] + jj (r + 1), s = col2sn[j], jj = j - sn_ptr[s], r = the front order (build_csc_factors' rule); the map is
// built once per handle, without the CSC view of the factors.
static int ensure_diag_map(cs3_handle h)
{
    if (h->d_diag) return CS3_OK;
    const Symbolic &S = h->S;
    std::vector<i64> diag((size_t) S.n);
    for (i64 j = 0; j < S.n; ++j) {
        const i32 s = S.col2sn[j];
        diag[j] = S.lpan_off[s] + (j - S.sn_ptr[s]) * (S.st_ptr[s + 1] - S.st_ptr[s] + 1);
    }
    return upload(&h->d_diag, diag);
}

int cs3_slogdet_dev(cs3_handle h, double *sign_dev, double *logabs_dev, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!sign_dev || !logabs_dev) { set_error("cs3_slogdet_dev: null argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_slogdet_dev: no successful factorisation"); return CS3_ERR_STATE; }
    if ((rc = ensure_diag_map(h))) return rc;
    CS3_HIP(launch_slogdet(h->D, (const long long *) h->d_diag, sign_dev, logabs_dev, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_slogdet(cs3_handle h, double *sign, double *logabs)
{
    int rc = guard(h); if (rc) return rc;
    if (!sign || !logabs) { set_error("cs3_slogdet: null argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_slogdet: no successful factorisation"); return CS3_ERR_STATE; }
    if ((rc = ensure_host_out(h))) return rc;
    const long long batch = h->batch;
    if ((rc = cs3_slogdet_dev(h, h->d_est_out, h->d_est_out + batch, nullptr))) return rc;
    std::vector<double> out((size_t) (2 * batch));
    CS3_HIP(hipMemcpy(out.data(), h->d_est_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(sign, out.data(), (size_t) batch * sizeof(double));
    std::memcpy(logabs, out.data() + batch, (size_t) batch * sizeof(double));
    return CS3_OK;
}

// ---- many low-rank-modified systems (A + dA_c) x = b on the held factors (updates.hip) ---------------------------------
// Plan: per case its distinct rows R_c and columns C_c (ascending) and the entry of D_c every triplet adds to; the cases
// in their order cut into tiles (a case joins the current tile unless the union of touched rows would pass the tile
// width, or the tile already has UPD_MAX_TILE_CASES cases); per tile the touched rows in order of first use = the columns
// of its Z.  A row that cases of two tiles touch is a column of both.
static int updates_build(cs3_updates_s &u, int64_t n, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj)
{
    u.n = n; u.ncases = ncases; u.ntrip = cp[ncases];
    u.cp.assign(cp, cp + ncases + 1);
    u.cases.assign((size_t) ncases, UpdCase());
    u.tpos.assign((size_t) u.ntrip, 0);
    std::vector<i32> rows, cols;
    std::vector<char> seen((size_t) n, 0);
    for (int64_t c = 0; c < ncases; ++c) {
        rows.assign(ci + cp[c], ci + cp[c + 1]);
        cols.assign(cj + cp[c], cj + cp[c + 1]);
        std::sort(rows.begin(), rows.end()); rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        std::sort(cols.begin(), cols.end()); cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        if (rows.size() > (size_t) UPD_MAX_RANK || cols.size() > (size_t) UPD_MAX_RANK) {
            set_error("cs3_updates_plan: case " + std::to_string(c) + " touches " + std::to_string(rows.size()) + " rows and " +
                      std::to_string(cols.size()) + " columns (at most 16 of each)");
            return CS3_ERR_ARG;
        }
        UpdCase &uc = u.cases[(size_t) c];
        std::memset(&uc, 0, sizeof(uc));
        uc.r = (int) rows.size(); uc.s = (int) cols.size();
        for (size_t a = 0; a < cols.size(); ++a) uc.col[a] = cols[a];
        for (int p = cp[c]; p < cp[c + 1]; ++p) {
            const int ri = (int) (std::lower_bound(rows.begin(), rows.end(), ci[p]) - rows.begin());
            const int cc = (int) (std::lower_bound(cols.begin(), cols.end(), cj[p]) - cols.begin());
            u.tpos[(size_t) p] = (unsigned char) (ri * UPD_MAX_RANK + cc);
        }
        u.max_rank = std::max<i64>(u.max_rank, std::max(uc.r, uc.s));
        for (i32 r : rows) if (!seen[(size_t) r]) { seen[(size_t) r] = 1; u.nrows_unique += 1; }
    }
    int tile = UPD_MAX_TILE;
    if (const char *e = std::getenv("CS3_UPD_TILE")) tile = (int) std::min<long long>(UPD_MAX_TILE, std::max<long long>(1, std::atoll(e)));
    u.tile_cap = std::max<int>(tile, (int) u.max_rank);           // every case fits a tile of its own
    std::vector<i32> pos((size_t) n, -1);                          // column of a row in the current tile
    std::vector<i32> cur;                                          // the current tile's rows
    cs3_updates_s::Tile t{0, 0, 0, 0, 0, 0};
    auto close_tile = [&]() {
        t.t = (int) cur.size();
        t.t_solve = std::min(u.tile_cap, (t.t + 63) / 64 * 64);   // few distinct widths: one captured graph per width
        t.unit0 = (i64) u.unit_row.size();
        u.unit_row.insert(u.unit_row.end(), cur.begin(), cur.end());
        u.unit_row.insert(u.unit_row.end(), (size_t) (t.t_solve - t.t), -1);
        u.tiles.push_back(t);
        for (i32 r : cur) pos[(size_t) r] = -1;
        cur.clear();
    };
    for (int64_t c = 0; c < ncases; ++c) {
        rows.assign(ci + cp[c], ci + cp[c + 1]);
        std::sort(rows.begin(), rows.end()); rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        int fresh = 0;
        for (i32 r : rows) fresh += pos[(size_t) r] < 0;
        if (t.nc > 0 && ((int) cur.size() + fresh > u.tile_cap || t.nc == UPD_MAX_TILE_CASES)) {
            close_tile();
            t = cs3_updates_s::Tile{(int) c, 0, 0, 0, 0, 0};
        }
        UpdCase &uc = u.cases[(size_t) c];
        for (size_t k = 0; k < rows.size(); ++k) {
            i32 &p = pos[(size_t) rows[k]];
            if (p < 0) { p = (i32) cur.size(); cur.push_back(rows[k]); }
            uc.zcol[k] = (unsigned short) p;
        }
        t.nc += 1;
        t.rmax = std::max(t.rmax, uc.r);
    }
    close_tile();
    return CS3_OK;
}

int cs3_updates_plan(cs3_handle h, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj, cs3_updates *out)
{
    int rc = guard(h); if (rc) return rc;
    if (!out) { set_error("cs3_updates_plan: null output"); return CS3_ERR_ARG; }
    *out = nullptr;
    if (!cp) { set_error("cs3_updates_plan: null case pointers"); return CS3_ERR_ARG; }
    if (ncases < 1 || ncases > INT_MAX / 2) { set_error("cs3_updates_plan: ncases must be >= 1"); return CS3_ERR_ARG; }
    if (cp[0] != 0) { set_error("cs3_updates_plan: cp[0] != 0"); return CS3_ERR_ARG; }
    for (int64_t c = 0; c < ncases; ++c)
        if (cp[c + 1] < cp[c]) { set_error("cs3_updates_plan: cp not monotone at case " + std::to_string(c)); return CS3_ERR_ARG; }
    if (cp[ncases] > 0 && (!ci || !cj)) { set_error("cs3_updates_plan: null index arrays"); return CS3_ERR_ARG; }
    const int64_t n = h->S.n;
    for (int64_t c = 0; c < ncases; ++c)
        for (int p = cp[c]; p < cp[c + 1]; ++p)
            if (ci[p] < 0 || ci[p] >= n || cj[p] < 0 || cj[p] >= n) {
                set_error("cs3_updates_plan: index out of range in case " + std::to_string(c));
                return CS3_ERR_ARG;
            }
    cs3_updates_s *u = nullptr;
    try {
        u = new cs3_updates_s();
        if ((rc = updates_build(*u, n, ncases, cp, ci, cj))) { delete u; return rc; }
        if (h->batch > 1) {
            delete u;
            set_error("cs3_updates_plan: handles with batch > 1 are not supported");
            return CS3_ERR_ARG;
        }
        h->plans.push_back(u);
    } catch (const std::bad_alloc &) {
        delete u; set_error("cs3_updates_plan: out of memory"); return CS3_ERR_ALLOC;
    }
    u->h = h;
    *out = u;
    return CS3_OK;
}

int cs3_updates_free(cs3_updates u)
{
    if (!u) return CS3_OK;
    if (u->h) {
        if (u->on_device) { (void) hipDeviceSynchronize(); release_plan_device(u); }
        auto &pl = u->h->plans;
        pl.erase(std::remove(pl.begin(), pl.end(), u), pl.end());
    }
    delete u;
    return CS3_OK;
}

int cs3_updates_info(cs3_updates u, int64_t *ncases, int64_t *nrows_unique, int64_t *max_rank, int64_t *ntiles)
{
    if (!u) { set_error("cs3_updates_info: null plan"); return CS3_ERR_ARG; }
    if (ncases) *ncases = u->ncases;
    if (nrows_unique) *nrows_unique = u->nrows_unique;
    if (max_rank) *max_rank = u->max_rank;
    if (ntiles) *ntiles = (int64_t) u->tiles.size();
    return CS3_OK;
}

int64_t cs3_debug_updates_tiles(cs3_updates u, int32_t *first_case, int32_t *ncases, int32_t *nrows, int32_t *width)
{
    if (!u) { set_error("cs3_debug_updates_tiles: null plan"); return CS3_ERR_ARG; }
    for (size_t k = 0; k < u->tiles.size(); ++k) {
        const auto &t = u->tiles[k];
        if (first_case) first_case[k] = t.c0;
        if (ncases) ncases[k] = t.nc;
        if (nrows) nrows[k] = t.t;
        if (width) width[k] = t.t_solve;
    }
    return (int64_t) u->tiles.size();
}

int cs3_debug_alloc_counters(cs3_handle h, int64_t *allocs, int64_t *syncs)
{
    int rc = guard(h); if (rc) return rc;
    if (allocs) *allocs = h->dbg_allocs;
    if (syncs) *syncs = h->dbg_syncs;
    return CS3_OK;
}

static int updates_check(const char *who, cs3_handle h, cs3_updates u, const double *cx, const double *b, const double *X)
{
    int rc = guard(h); if (rc) return rc;
    if (!u) { set_error(std::string(who) + ": null plan"); return CS3_ERR_ARG; }
    if (!b || !X || (u->ntrip > 0 && !cx)) { set_error(std::string(who) + ": null argument"); return CS3_ERR_ARG; }
    if (u->h != h) { set_error(std::string(who) + ": the plan was made for another handle"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": no successful factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

// Tables of the plan in HBM, the handle's Z and x0, room for the widest tile in the sweep buffers: everything a call
// needs, so that later calls neither allocate nor synchronise.
static int ensure_updates(cs3_handle h, cs3_updates_s *u)
{
    int wmax = 1;
    for (const auto &t : u->tiles) wmax = std::max(wmax, t.t_solve);
    if (!u->on_device) {
        static bool prepared = false;
        if (!prepared) { CS3_HIP(prepare_updates_kernels()); prepared = true; }
        int rc;
        if ((rc = upload(&u->d_cases, u->cases))) return rc;
        if ((rc = upload(&u->d_cp, u->cp))) return rc;
        if ((rc = upload(&u->d_tpos, u->tpos))) return rc;
        if ((rc = upload(&u->d_unit, u->unit_row))) return rc;
        CS3_HIP(hipMalloc((void **) &u->d_y, (size_t) u->ncases * UPD_MAX_RANK * sizeof(double)));
        CS3_HIP(hipMalloc((void **) &u->d_flag, (size_t) u->ncases * sizeof(int)));
        CS3_HIP(hipMalloc((void **) &u->d_rpiv, (size_t) u->ncases * sizeof(double)));
        h->dbg_allocs += 7;
        u->on_device = true;
    }
    const size_t n1 = std::max<size_t>(1, (size_t) h->S.n);
    if (!h->d_upd_x0) { CS3_HIP(hipMalloc((void **) &h->d_upd_x0, n1 * sizeof(double))); h->dbg_allocs += 1; }
    if (h->upd_z_cols < wmax) {
        if (h->d_upd_z) {                                  // a wider plan than any before: the old tile may still be in use
            CS3_HIP(hipDeviceSynchronize());
            h->dbg_syncs += 1;
            (void) hipFree(h->d_upd_z);
            h->d_upd_z = nullptr; h->upd_z_cols = 0;
        }
        CS3_HIP(hipMalloc((void **) &h->d_upd_z, n1 * (size_t) wmax * sizeof(double)));
        h->dbg_allocs += 1;
        h->upd_z_cols = wmax;
    }
    return ensure_rhs_capacity(h, wmax);
}

static int updates_run(cs3_handle h, cs3_updates_s *u, const double *cx_dev, const double *b_dev, double sing_tol, double *X_dev,
                       double *rpiv_dev, hipStream_t st)
{
    int rc = ensure_updates(h, u);
    if (rc) return rc;
    const i64 n = h->S.n;
    const UpdTables T{u->d_cases, u->d_cp, u->d_tpos, u->d_y, u->d_flag};
    double *rpiv = rpiv_dev ? rpiv_dev : u->d_rpiv;
    if (n > 0) {
        CS3_HIP(hipMemcpyAsync(h->d_upd_x0, b_dev, (size_t) n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if ((rc = run_solve(h, h->d_upd_x0, 1, 0, st))) return rc;
    }
    for (const auto &t : u->tiles) {
        if (n > 0 && t.t > 0) {
            CS3_HIP(launch_upd_units(h->d_upd_z, n, t.t_solve, u->d_unit + t.unit0, st));
            if ((rc = run_solve(h, h->d_upd_z, t.t_solve, 0, st))) return rc;
        }
        CS3_HIP(launch_upd_capacitance(T, cx_dev, h->d_upd_z, t.t_solve, h->d_upd_x0, t.c0, t.nc, sing_tol, rpiv, st));
        CS3_HIP(launch_upd_apply(T, h->d_upd_z, t.t_solve, h->d_upd_x0, n, t.c0, t.nc, t.rmax, u->ncases, X_dev, st));
    }
    return CS3_OK;
}

int cs3_updates_solve_dev(cs3_handle h, cs3_updates u, const double *cx_dev, const double *b_dev, double sing_tol, double *X_dev,
                          double *rpiv_dev, void *stream)
{
    int rc = updates_check("cs3_updates_solve_dev", h, u, cx_dev, b_dev, X_dev);
    if (rc) return rc;
    return updates_run(h, u, cx_dev, b_dev, sing_tol, X_dev, rpiv_dev, (hipStream_t) stream);
}

int cs3_updates_solve(cs3_handle h, cs3_updates u, const double *cx, const double *b, double sing_tol, double *X, double *rpiv)
{
    int rc = updates_check("cs3_updates_solve", h, u, cx, b, X);
    if (rc) return rc;
    const size_t n = (size_t) h->S.n, nc = (size_t) u->ncases, nt = (size_t) u->ntrip;
    if (!u->d_cx) CS3_HIP(hipMalloc((void **) &u->d_cx, std::max<size_t>(nt, 1) * sizeof(double)));
    double *d_b = nullptr, *d_x = nullptr;                 // [n] and [n, ncases], for this call
    CS3_HIP(hipMalloc((void **) &d_b, std::max<size_t>(n * (nc + 1), 1) * sizeof(double)));
    d_x = d_b + n;
    hipError_t e = nt ? hipMemcpy(u->d_cx, cx, nt * sizeof(double), hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess && n) e = hipMemcpy(d_b, b, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = updates_run(h, u, u->d_cx, d_b, sing_tol, d_x, nullptr, nullptr);
        if (rc == CS3_OK && n) e = hipMemcpy(X, d_x, n * nc * sizeof(double), hipMemcpyDeviceToHost);
        if (rc == CS3_OK && e == hipSuccess && rpiv) e = hipMemcpy(rpiv, u->d_rpiv, nc * sizeof(double), hipMemcpyDeviceToHost);
        if (rc == CS3_OK && e == hipSuccess) e = hipDeviceSynchronize();
    }
    (void) hipFree(d_b);
    if (rc) return rc;
    CS3_HIP(e);
    return CS3_OK;
}

// The same on data that already lives in HBM: nothing crosses PCIe and nothing synchronises.  The caller knows the
// blocks' entry counts (it allocated them) and passes them, so no column pointer has to come back to the host.
int cs3_csc_stack_4_by_4_dev(int64_t am, int64_t an, int64_t nnz_a, const int32_t *Ai, const int32_t *Ap, const double *Ax,
                             int64_t bm, int64_t bn, int64_t nnz_b, const int32_t *Bi, const int32_t *Bp, const double *Bx,
                             int64_t cm, int64_t cn, int64_t nnz_c, const int32_t *Ci, const int32_t *Cp, const double *Cx,
                             int64_t dm, int64_t dn, int64_t nnz_d, const int32_t *Di, const int32_t *Dp, const double *Dx,
                             int32_t *Pi, int32_t *Pp, double *Px, int32_t *map, void *stream)
{
    if (am != bm || cm != dm || an != cn || bn != dn) { set_error("cs3_csc_stack_4_by_4_dev: incompatible block shapes"); return CS3_ERR_ARG; }
    if (!Ap || !Bp || !Cp || !Dp || !Pp) { set_error("cs3_csc_stack_4_by_4_dev: null argument"); return CS3_ERR_ARG; }
    const int64_t nnz = nnz_a + nnz_b + nnz_c + nnz_d;
    if (nnz_a < 0 || nnz_b < 0 || nnz_c < 0 || nnz_d < 0 || nnz > INT_MAX || an + bn > INT_MAX) { set_error("cs3_csc_stack_4_by_4_dev: bad sizes"); return CS3_ERR_ARG; }
    if (nnz > 0 && (!Pi || !Px)) { set_error("cs3_csc_stack_4_by_4_dev: null output"); return CS3_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: cs3_csc_stack_4_by_4_dev runs on the GPU only"); return CS3_ERR_HIP;
    }
    CS3_HIP(launch_stack_4_by_4((int) an, (int) bn, (int) am, (int) bm, Ap, Ai, Ax, Bp, Bi, Bx, Cp, Ci, Cx, Dp, Di, Dx, Pp, Pi, Px,
                                map, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_restack_values_dev(int64_t nnz, const int32_t *map, int64_t nnz_a, int64_t nnz_b, int64_t nnz_c,
                           const double *Ax, const double *Bx, const double *Cx, const double *Dx, double *Px, void *stream)
{
    if (nnz < 0 || nnz_a < 0 || nnz_b < 0 || nnz_c < 0 || (nnz > 0 && (!map || !Px))) { set_error("cs3_restack_values_dev: bad argument"); return CS3_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: cs3_restack_values_dev runs on the GPU only"); return CS3_ERR_HIP;
    }
    CS3_HIP(launch_restack_values(nnz, map, nnz_a, nnz_b, nnz_c, Ax, Bx, Cx, Dx, Px, (hipStream_t) stream));
    return CS3_OK;
}

}  // extern "C"
