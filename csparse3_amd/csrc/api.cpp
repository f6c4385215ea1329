// C ABI of the library (include/csparse3_amd.h): handle management, HBM
// residency, hipGraph capture of the level schedules, host <-> device copies.
// (The applications on a factorised handle -- updates, sparse right-hand sides, selected inversion -- are in apps.cpp.)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "cs3_cplx.hpp"
#include "cs3_handle.hpp"

using namespace cs3;

namespace {
thread_local std::string g_error;
}

namespace cs3 {
void set_error(const std::string &msg) { g_error = msg; }
}

namespace {

// One array of the DeviceFactor: the block joins h->mem.factor, *field points at it.
template <class T>
int factor_alloc(cs3_handle h, T **field, size_t count)
{
    DevBuf<unsigned char> b;
    CS3_HIP(b.alloc(count * sizeof(T)));
    *field = reinterpret_cast<T *>(b.get());
    h->mem.factor.push_back(std::move(b));
    return CS3_OK;
}

template <class T>
int factor_upload(cs3_handle h, T **field, const std::vector<T> &src)
{
    if (int rc = factor_alloc(h, field, src.size())) return rc;
    if (!src.empty()) CS3_HIP(hipMemcpy(*field, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
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

// Frees every HBM allocation of the handle (ensure_device's error path and cs3_free).
void release_device(cs3_handle h)
{
    for (HeldPlan *u : h->plans) u->drop_device();
    (void) drop_graphs(h, [](const GraphKey &) { return true; }, true);     // (cs3_free has synchronised)
    if (h->cap_stream) { (void) hipStreamDestroy(h->cap_stream); h->cap_stream = nullptr; }
    h->fj.destroy();
    h->mem = cs3_handle_s::Memory();
    h->kry_work = KryWork();
    h->selinv_valid = false;
    h->D = DeviceFactor();                  // (no pointer of it outlives its block; nrhs_cap = 0)
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
int ensure_match(cs3_handle h);

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
    if (!device_visible()) {
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
        if (S.sn_class[s] == FC_BIG && f.r >= (1 << 22)) {     // (launch_big_block refuses it too: this message survives)
            set_error("a front of order " + std::to_string(f.r) + " is beyond k_big_step's 32-bit tile offsets (order < 2^22)");
            return CS3_ERR_ARG;
        }
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
        if ((rc = factor_upload(h, &D.sdesc1, sdesc1))) return rc;
        if ((rc = factor_upload(h, &D.sub_tasks, S.sub_tasks))) return rc;
        if ((rc = factor_upload(h, &D.sub_fronts, S.sub_fronts))) return rc;
        if ((rc = factor_upload(h, &D.sub_lvl, S.sub_lvl))) return rc;
        if ((rc = factor_upload(h, &D.sub_rel, S.sub_rel))) return rc;
        if ((rc = factor_upload(h, &D.sub_st, S.sub_st))) return rc;
        if ((rc = factor_upload(h, &D.sub_child, S.sub_child))) return rc;
        if ((rc = factor_upload(h, &D.sub_a_tgt, S.sub_a_tgt))) return rc;
        if ((rc = factor_upload(h, &D.sub_a_src, S.sub_a_src))) return rc;
        if ((rc = factor_alloc(h, &D.axf, (size_t) (D.batch * D.n_sub_a)))) return rc;
    }
    if ((rc = factor_upload(h, &D.sdesc, sdesc))) return rc;
    if ((rc = factor_upload(h, &D.fasm_src, S.fasm_src))) return rc;
    if ((rc = factor_upload(h, &D.fasm_tgt, S.fasm_tgt))) return rc;
    if ((rc = factor_upload(h, &D.flong_src, S.flong_src))) return rc;
    if ((rc = factor_upload(h, &D.rl_pairs, S.rl_pairs))) return rc;
    if ((rc = factor_upload(h, &D.sl_src, S.sl_src))) return rc;
    if ((rc = factor_upload(h, &D.fdesc, fdesc))) return rc;
    if ((rc = factor_upload(h, &D.st_idx, S.st_idx))) return rc;
    if ((rc = factor_upload(h, &D.fa_tgt, S.fa_tgt))) return rc;
    if ((rc = factor_upload(h, &D.fa_src, S.fa_src))) return rc;
    {
        std::vector<i32> tab(S.ch_tab);
        tab.resize(tab.size() + 4, 0);                          // (16-byte loads of the last entry stay inside the array)
        if ((rc = factor_upload(h, &D.ch_tab, tab))) return rc;
    }
    if ((rc = factor_upload(h, &D.rel_idx, S.rel_idx))) return rc;
    if ((rc = factor_upload(h, &D.q, S.q))) return rc;
    if ((rc = factor_upload(h, &D.ila_pairs, S.ila_pairs))) return rc;
    if ((rc = factor_upload(h, &D.inv_tasks, S.inv_tasks))) return rc;
    if ((rc = factor_alloc(h, &D.dinv, (size_t) (D.batch * D.dinv_size)))) return rc;
    D.il_len = S.il_len;
    D.pm_stride = S.pool_size - S.il_len;
    D.ngroups = (D.batch + 63) / 64;
    const size_t il_doubles = (size_t) (D.ngroups * 64 * D.il_len);
    if ((rc = factor_alloc(h, &D.pool, il_doubles + (size_t) (D.batch * D.pm_stride) + POOL_SLACK))) return rc;   // slack: see k_fwd_rhs
    D.pool_il = D.pool;
    D.pool_pm = D.pool + il_doubles - D.il_len;            // virtual offsets >= il_len index this pointer directly
    if ((rc = factor_alloc(h, &D.dbuf, (size_t) (D.batch * D.dbuf_size)))) return rc;
    if ((rc = factor_alloc(h, &D.ax, (size_t) (D.batch * D.nnz_a)))) return rc;
    // [0] the status word, [1], [2] unused, [3] a hand-over between waves timed out, [4 + b] perturbed pivots of matrix b
    if ((rc = factor_alloc(h, &D.status, 4 + (size_t) D.batch))) return rc;
    CS3_HIP(hipMemset(D.status, 0, (4 + (size_t) D.batch) * sizeof(int)));
    CS3_HIP(hipMemset(D.status, 0x7f, sizeof(int)));      // "clean": a handle that only imports factors never runs a prologue
    if (const char *pf = std::getenv("CS3_PROFILE")) {
        if (pf[0] == '1' || pf[0] == '2') {
            D.tbuf_diag = pf[0] == '2';
            const size_t stamps = std::max<size_t>(1, (size_t) S.nsuper) * 8;
            if ((rc = factor_alloc(h, &D.tbuf, stamps))) return rc;
            CS3_HIP(hipMemset(D.tbuf, 0, stamps * sizeof(long long)));
        }
    }
    if (h->match.on)
        if ((rc = ensure_match(h))) return rc;
    if (S.schur_sn >= 0) {
        // the Schur front's buffer is rewritten (with the identity) by every factorisation: the prologue zeroes it whatever
        // the other big fronts do
        const i64 ns = (i64) S.schur_idx.size();
        D.zero_big = true;
        D.schur_ns = (int) ns;
        D.schur_lpan = S.lpan_off[S.schur_sn];
        CS3_HIP(h->mem.schur.alloc((size_t) (D.batch * ns * ns)));
        D.schur = h->mem.schur.get();
    }
    CS3_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    CS3_HIP(h->fj.init());
    const char *ng = std::getenv("CS3_NO_GRAPH");
    h->use_graph = !(ng && ng[0] == '1');
    h->on_device = true;
    return CS3_OK;
}

}  // namespace

int cs3::ensure_rhs_capacity(cs3_handle h, long long nrhs)
{
    DeviceFactor &D = h->D;
    if (nrhs <= D.nrhs_cap) return CS3_OK;
    CS3_HIP(hipDeviceSynchronize());
    h->dbg_syncs += 1;
    h->dbg_allocs += 4;
    if (int rc = drop_graphs(h, [](const GraphKey &k) { return !graph_op_is(k, GRAPH_FACTOR); }, true)) return rc;
    auto &M = h->mem;
    M.cv.reset(); M.xp.reset(); M.bigv.reset(); M.gv.reset();
    D.cv = D.xp = D.bigv = D.gv = nullptr;
    D.nrhs_cap = 0;                           // nothing usable until all four are back
    CS3_HIP(M.cv.alloc((size_t) (D.batch * D.cv_size * nrhs)));
    CS3_HIP(M.xp.alloc((size_t) (D.batch * D.n * nrhs)));
    CS3_HIP(M.bigv.alloc((size_t) (D.batch * D.bv_size * nrhs)));
    CS3_HIP(M.gv.alloc((size_t) (D.batch * D.gv_size * nrhs)));
    D.cv = M.cv.get(); D.xp = M.xp.get(); D.bigv = M.bigv.get(); D.gv = M.gv.get();
    D.nrhs_cap = nrhs;
    return CS3_OK;
}

namespace {

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

// Device arrays of a matched handle, uploaded once (they die with release_device).
int ensure_match(cs3_handle h)
{
    auto &M = h->mem.match;
    if (M.dr.get()) return CS3_OK;
    const i64 n = h->S.n, nnz = h->S.nnzA;
    std::vector<int> rq((size_t) n), ecol((size_t) nnz);
    for (i64 k = 0; k < n; ++k) rq[k] = h->match.rowperm[h->S.q[k]];
    for (i64 j = 0; j < n; ++j)
        for (i64 p = h->Ap_host[j]; p < h->Ap_host[j + 1]; ++p) ecol[p] = (int) j;
    CS3_HIP(M.dr.upload(h->match.dr)); CS3_HIP(M.dc.upload(h->match.dc));
    CS3_HIP(M.rq.upload(rq)); CS3_HIP(M.erow.upload(h->Ai_host)); CS3_HIP(M.ecol.upload(ecol));
    return CS3_OK;
}

MatchView match_view(cs3_handle h)
{
    const auto &M = h->mem.match;
    return MatchView{M.dr.get(), M.dc.get(), M.rq.get(), M.erow.get(), M.ecol.get()};
}

// The row permutations of a full solve on a matched handle, scalings folded in (A x = b: x = Dc B^-1 (Dr P b);
// A' x = b: x = P' Dr B^-T (Dc b)).  into_pivot_order: the caller's rows into D.xp; else D.xp back to the caller's rows.
hipError_t launch_match_permute(cs3_handle h, const double *src, double *dst, int nrhs, bool into_pivot_order, bool trans, hipStream_t st)
{
    const DeviceFactor &D = h->D;
    const MatchView M = match_view(h);
    const bool rows_of_a = into_pivot_order != trans;          // this side runs over the rows of A (rq, dr), the other over its columns (q, dc)
    return launch_match_rows(src, dst, rows_of_a ? M.rq : D.q, rows_of_a ? M.dr : M.dc, D.n, nrhs, D.batch, !into_pivot_order, st);
}

}  // namespace

// A Schur handle holds the factors of A with A22 replaced by A22 - S + I: whatever would silently answer for that matrix
// is refused.
int cs3::refuse_schur(cs3_handle h, const char *who)
{
    if (h->S.schur_sn < 0) return CS3_OK;
    set_error(std::string(who) + ": not available on a Schur handle (cs3_analyze_schur) -- its factors are those of A with A22 replaced "
              "by A22 - S + I, not of A; use cs3_schur_get / cs3_schur_fwd / cs3_schur_bwd");
    return CS3_ERR_ARG;
}

namespace {

// One half-solve of a Schur handle: the caller's X (rows of A) into D.xp, one direction of the unchanged sweeps, back.
// Forward: the Schur rows end up as b2 - A21 A11^-1 b1, the interior rows half-solved.  Backward, entered with x2 in the
// Schur rows: x1 = U11^-1 (y1 - U12 x2).  The sweeps are replayed from a graph per (direction, nrhs).
int run_schur_sweep(cs3_handle h, const char *who, double *x_dev, long long k, bool forward, hipStream_t st);

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

// The pivot rule of one factorisation: the caller's tol and the handle's perturbation.
PivotCtl pivot_ctl(cs3_handle h, double tol)
{
    return PivotCtl{(tol > 0.0) ? 1.0 / tol : HUGE_VAL, h->perturb_delta, h->D.status + 4};
}

int run_factor(cs3_handle h, const double *ax_dev, double tol, hipStream_t st)
{
    const DeviceFactor &D = h->D;
    const PivotCtl pc = pivot_ctl(h, tol);
    if (h->match.on) {                                          // the values of B straight into the library's copy
        CS3_HIP(launch_match_values(match_view(h), ax_dev, D.ax, D.nnz_a, D.batch, st));
        ax_dev = D.ax;
    }
    CS3_HIP(launch_prologue(D, ax_dev, nullptr, 0, st));        // status 0x7f7f7f7f = clean, zeros, values
    if (h->factor_ctl != pc) {
        if (int rc = drop_graphs(h, [](const GraphKey &k) { return graph_op_is(k, GRAPH_FACTOR); })) return rc;
        h->factor_ctl = pc;
    }
    const SweepCall call;
    int rc = replay_or_run(h, GraphKey(GRAPH_FACTOR, false, 0, nullptr), st, [&](hipStream_t s) {
        return launch_factor_levels(D, call, h->S.groups, pc, s, h->fj);
    });
    if (rc) return rc;
    h->factored = true;
    h->factor_ran = true;
    h->inverses_valid = false;
    h->selinv_valid = false;
    return CS3_OK;
}

int read_status(cs3_handle h, hipStream_t st)
{
    int word[4] = {0, 0, 0, 0};
    CS3_HIP(hipMemcpyAsync(word, h->D.status, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    if (word[3] != 0) {
        // a wait inside the step was given up: a wave of a shared elimination never saw the multipliers of its partner
        // (eliminate_parts in k_big_step / the shared fronts of the forest).  Whatever was computed behind that point is
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

}  // namespace

// mode 0: full solve with permutations; 1: lsolve only; 2: usolve only (in pivot order, on X itself).
// trans (LU): A' X = B; the forward sweep solves with U', the backward sweep with L' (mode 1: utsolve, 2: ltsolve).
// On a Cholesky handle A' = A and trans changes nothing.
int cs3::run_solve(cs3_handle h, double *x_dev, long long k, int mode, hipStream_t st, bool trans)
{
    if (int rc = refuse_schur(h, "solves and one-sided sweeps")) return rc;
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
    const bool matched = h->match.on;                          // (the scalings are not folded into the XMap sweeps)
    const bool fused = !matched && permutation_can_fuse(D, nrhs);
    if (fused) call.xm = XMap{x_dev, x_dev, D.q};
    else if (matched) CS3_HIP(launch_match_permute(h, x_dev, D.xp, nrhs, true, trans, st));
    else CS3_HIP(launch_permute(D, x_dev, D.xp, nrhs, false, st));
    rc = replay_or_run(h, GraphKey(GRAPH_SOLVE, trans, nrhs, fused ? x_dev : nullptr), st, [&](hipStream_t s) {
        hipError_t e = launch_solve_levels(D, call, D.xp, nrhs, true, s, h->fj);
        return (e != hipSuccess) ? e : launch_solve_levels(D, call, D.xp, nrhs, false, s, h->fj);
    });
    if (rc) return rc;
    if (matched) CS3_HIP(launch_match_permute(h, D.xp, x_dev, nrhs, false, trans, st));
    else if (!fused) CS3_HIP(launch_permute(D, D.xp, x_dev, nrhs, true, st));
    return CS3_OK;
}

namespace {

int run_schur_sweep(cs3_handle h, const char *who, double *x_dev, long long k, bool forward, hipStream_t st)
{
    if (h->S.schur_sn < 0) { set_error(std::string(who) + ": the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (!x_dev) { set_error(std::string(who) + ": null right-hand side"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": called before a successful factorisation"); return CS3_ERR_STATE; }
    if (k < 1 || k > INT_MAX) { set_error(std::string(who) + ": bad number of right-hand sides"); return CS3_ERR_ARG; }
    int rc = ensure_rhs_capacity(h, k);
    if (rc) return rc;
    const DeviceFactor &D = h->D;
    const int nrhs = (int) k;
    const SweepCall call = select_sweep_schedule(h, nrhs);
    if (nrhs >= 16 && D.n_inv_tasks > 0 && !h->inverses_valid) {
        CS3_HIP(launch_diag_inverses(D, st));
        h->inverses_valid = true;
    }
    CS3_HIP(launch_permute(D, x_dev, D.xp, nrhs, false, st));
    rc = replay_or_run(h, GraphKey(forward ? GRAPH_SCHUR_FWD : GRAPH_SCHUR_BWD, false, nrhs, nullptr), st, [&](hipStream_t s) {
        return launch_solve_levels(D, call, D.xp, nrhs, forward, s, h->fj);
    });
    if (rc) return rc;
    CS3_HIP(launch_permute(D, D.xp, x_dev, nrhs, true, st));
    return CS3_OK;
}

// numeric factorisation and full solve in one graph; the forward sweep runs beside the factorisation
int run_factor_solve(cs3_handle h, const double *ax_dev, const double *b_dev, double *x_dev, long long k, double tol, hipStream_t st)
{
    if (k < 1 || k > INT_MAX) { set_error("factor_solve: bad number of right-hand sides"); return CS3_ERR_ARG; }
    int rc = refuse_schur(h, "cs3_factor_solve(_bx)_dev");
    if (rc) return rc;
    if ((rc = ensure_rhs_capacity(h, k))) return rc;
    const DeviceFactor &D = h->D;
    const int nrhs = (int) k;
    const PivotCtl pc = pivot_ctl(h, tol);
    SweepCall call = select_sweep_schedule(h, nrhs);
    call.fwd_in_factor = nrhs == 1 && !h->S.sub_forest.empty();   // the forest's factor launch carries its forward sweep
    call.inverses_in_sweep = true;                                 // the forward sweep inverts group by group
    const bool matched = h->match.on;
    if (matched) {                                                 // scaled values, then the scaled right-hand sides into D.xp
        CS3_HIP(launch_match_values(match_view(h), ax_dev, D.ax, D.nnz_a, D.batch, st));
        CS3_HIP(launch_prologue(D, D.ax, nullptr, nrhs, st));
        CS3_HIP(launch_match_permute(h, b_dev, D.xp, nrhs, true, false, st));
    } else {
        CS3_HIP(launch_prologue(D, ax_dev, b_dev, nrhs, st));      // right-hand sides are read from b_dev, the solution goes to x_dev
    }
    if (h->fused_ctl != pc) {
        if ((rc = drop_graphs(h, [](const GraphKey &g) { return graph_op_is(g, GRAPH_FUSED); }))) return rc;
        h->fused_ctl = pc;
    }
    h->fused_same_x = (x_dev == h->fused_last_x) ? h->fused_same_x + 1 : 0;
    h->fused_last_x = x_dev;
    const bool per_x = h->fused_same_x >= 2;                       // third call in a row with this X: its own graph, permutation included
    rc = replay_or_run(h, GraphKey(GRAPH_FUSED, false, nrhs, per_x ? x_dev : nullptr), st, [&](hipStream_t s) {
        hipError_t e = launch_factor_with_forward(D, call, h->S.groups, pc, D.xp, nrhs, s, h->fj);
        if (e == hipSuccess) e = launch_solve_levels(D, call, D.xp, nrhs, false, s, h->fj);
        if (e == hipSuccess && per_x)
            e = matched ? launch_match_permute(h, D.xp, x_dev, nrhs, false, false, s) : launch_permute(D, D.xp, x_dev, nrhs, true, s);
        return e;
    });
    if (rc) return rc;
    if (!per_x) CS3_HIP(matched ? launch_match_permute(h, D.xp, x_dev, nrhs, false, false, st) : launch_permute(D, D.xp, x_dev, nrhs, true, st));
    h->factored = true;
    h->factor_ran = true;
    h->inverses_valid = nrhs >= 16;                                // a many-RHS fused call leaves them current
    h->selinv_valid = false;
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

}  // namespace

int cs3::guard(cs3_handle h)
{
    if (!h) { set_error("null handle"); return CS3_ERR_ARG; }
    return CS3_OK;
}

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

// The checks of cs3_match_scale and the matching itself; `matched` columns on CS3_ERR_PIVOT.
static int matching_of(const char *who, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                       int32_t *rowperm, double *dr, double *dc)
{
    if (!rowperm || !dr || !dc) { set_error(std::string(who) + ": null output"); return CS3_ERR_ARG; }
    if (int rc = check_pattern(who, n, Ap, Ai)) return rc;
    const int64_t nnz = n > 0 ? Ap[n] : 0;
    if (nnz > 0 && !Ax) { set_error(std::string(who) + ": null values"); return CS3_ERR_ARG; }
    for (int64_t p = 0; p < nnz; ++p)
        if (!std::isfinite(Ax[p])) { set_error(std::string(who) + ": non-finite value at entry " + std::to_string(p)); return CS3_ERR_ARG; }
    int64_t matched = 0;
    try { matched = match_scale(n, Ap, Ai, Ax, rowperm, dr, dc); }
    catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    if (matched < n) {
        set_error(std::string(who) + ": structurally singular, only " + std::to_string(matched) + " of " + std::to_string(n) +
                  " columns can be matched to distinct rows (stored zeros count as absent)");
        return CS3_ERR_PIVOT;
    }
    return CS3_OK;
}

int cs3_match_scale(int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, int32_t *rowperm, double *dr, double *dc)
{
    return matching_of("cs3_match_scale", n, Ap, Ai, Ax, rowperm, dr, dc);
}

int cs3_analyze_matched(int64_t order, int64_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                        const int32_t *q_given, int64_t batch, cs3_handle *out)
{
    if (!out) { set_error("cs3_analyze_matched: null output"); return CS3_ERR_ARG; }
    *out = nullptr;
    if (batch < 1) { set_error("cs3_analyze_matched: batch must be >= 1"); return CS3_ERR_ARG; }
    if (n < 0 || !Ap) { set_error("cs3_analyze_matched: bad size or null column pointers"); return CS3_ERR_ARG; }
    cs3_handle h = nullptr;
    try {
        h = new cs3_handle_s();
        h->batch = batch;
        auto &M = h->match;
        M.rowperm.resize((size_t) n); M.dr.resize((size_t) n); M.dc.resize((size_t) n);
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = matching_of("cs3_analyze_matched", n, Ap, Ai, Ax, M.rowperm.data(), M.dr.data(), M.dc.data())) { delete h; return rc; }
        M.t_match = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        M.on = true;
        const int64_t nnz = n > 0 ? Ap[n] : 0;
        std::vector<i32> rowinv((size_t) n), Bi((size_t) nnz);
        for (int64_t j = 0; j < n; ++j) rowinv[M.rowperm[j]] = (i32) j;
        for (int64_t p = 0; p < nnz; ++p) Bi[p] = rowinv[Ai[p]];
        // det A = parity det B / (prod dr prod dc): the two scalars of cs3_slogdet, summed in index order
        std::vector<char> seen((size_t) n, 0);
        for (int64_t j = 0; j < n; ++j) {
            if (seen[j]) continue;
            int64_t len = 0;
            for (int64_t k = j; !seen[k]; k = M.rowperm[k]) { seen[k] = 1; ++len; }
            if (len % 2 == 0) M.parity = -M.parity;
        }
        double sum = 0.0;
        for (int64_t j = 0; j < n; ++j) sum += std::log(M.dr[j]);
        for (int64_t j = 0; j < n; ++j) sum += std::log(M.dc[j]);
        M.log_shift = -sum;
        analyze(CS3_LU, (int) order, n, Ap, Bi.data(), q_given, h->S, batch);
        h->Ap_host.assign(Ap, Ap + n + 1);
        h->Ai_host.assign(Ai, Ai + nnz);
    } catch (const std::bad_alloc &) {
        delete h; set_error("cs3_analyze_matched: out of memory"); return CS3_ERR_ALLOC;
    } catch (const std::exception &e) {
        delete h; set_error(e.what()); return CS3_ERR_ARG;
    }
    *out = h;
    return CS3_OK;
}

int cs3_get_matching(cs3_handle h, int32_t *rowperm, double *dr, double *dc, double *t_match_s)
{
    int rc = guard(h); if (rc) return rc;
    if (!h->match.on) { set_error("cs3_get_matching: the handle was not analysed with a matching (cs3_analyze_matched)"); return CS3_ERR_STATE; }
    const size_t n = (size_t) h->S.n;
    if (rowperm) std::memcpy(rowperm, h->match.rowperm.data(), n * sizeof(int32_t));
    if (dr) std::memcpy(dr, h->match.dr.data(), n * sizeof(double));
    if (dc) std::memcpy(dc, h->match.dc.data(), n * sizeof(double));
    if (t_match_s) *t_match_s = h->match.t_match;
    return CS3_OK;
}

int cs3_analyze_schur(int64_t kind, int64_t order, int64_t n, const int32_t *Ap, const int32_t *Ai,
                      const int32_t *q_given, int64_t batch, int64_t ns, const int32_t *schur_idx, cs3_handle *out)
{
    if (!out) { set_error("cs3_analyze_schur: null output"); return CS3_ERR_ARG; }
    *out = nullptr;
    if (batch < 1) { set_error("cs3_analyze_schur: batch must be >= 1"); return CS3_ERR_ARG; }
    cs3_handle h = nullptr;
    try {
        h = new cs3_handle_s();
        h->batch = batch;
        const SchurSet schur{schur_idx, ns};
        analyze((int) kind, (int) order, n, Ap, Ai, q_given, h->S, batch, &schur);
        h->Ap_host.assign(Ap, Ap + n + 1);
        h->Ai_host.assign(Ai, Ai + (n > 0 ? Ap[n] : 0));
    } catch (const std::bad_alloc &) {
        delete h; set_error("cs3_analyze_schur: out of memory"); return CS3_ERR_ALLOC;
    } catch (const std::exception &e) {
        delete h; set_error(e.what()); return CS3_ERR_ARG;
    }
    *out = h;
    return CS3_OK;
}

int cs3_schur_info(cs3_handle h, int64_t *ns, int32_t *schur_idx)
{
    int rc = guard(h); if (rc) return rc;
    if (h->S.schur_sn < 0) { set_error("cs3_schur_info: the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (ns) *ns = (int64_t) h->S.schur_idx.size();
    if (schur_idx) std::memcpy(schur_idx, h->S.schur_idx.data(), h->S.schur_idx.size() * sizeof(int32_t));
    return CS3_OK;
}

int cs3_schur_get_dev(cs3_handle h, double *S_dev, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (h->S.schur_sn < 0) { set_error("cs3_schur_get_dev: the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (!S_dev) { set_error("cs3_schur_get_dev: null buffer"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_schur_get_dev: called before a successful factorisation"); return CS3_ERR_STATE; }
    CS3_HIP(hipMemcpyAsync(S_dev, h->D.schur, h->mem.schur.count() * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_schur_get(cs3_handle h, double *S)
{
    int rc = guard(h); if (rc) return rc;
    if (h->S.schur_sn < 0) { set_error("cs3_schur_get: the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (!S) { set_error("cs3_schur_get: null buffer"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_schur_get: called before a successful factorisation"); return CS3_ERR_STATE; }
    CS3_HIP(hipMemcpy(S, h->D.schur, h->mem.schur.count() * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_schur_fwd_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_schur_sweep(h, "cs3_schur_fwd_dev", X_dev, k, true, (hipStream_t) stream);
}

int cs3_schur_bwd_dev(cs3_handle h, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    return run_schur_sweep(h, "cs3_schur_bwd_dev", X_dev, k, false, (hipStream_t) stream);
}

// The host forms: X staged in HBM for the call, the same kernels on the null stream, the same bits.
static int schur_sweep_host(cs3_handle h, const char *who, double *X, int64_t k, bool forward)
{
    int rc = guard(h); if (rc) return rc;
    if (h->S.schur_sn < 0) { set_error(std::string(who) + ": the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (!X) { set_error(std::string(who) + ": null right-hand side"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": called before a successful factorisation"); return CS3_ERR_STATE; }
    if (k < 1 || k > INT_MAX) { set_error(std::string(who) + ": bad number of right-hand sides"); return CS3_ERR_ARG; }
    const size_t count = (size_t) (h->batch * h->S.n * k);
    DevBuf<double> x;
    CS3_HIP(x.alloc(count));
    CS3_HIP(hipMemcpy(x.get(), X, count * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = run_schur_sweep(h, who, x.get(), k, forward, nullptr))) return rc;
    CS3_HIP(hipMemcpy(X, x.get(), count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_schur_fwd(cs3_handle h, double *X, int64_t k) { return schur_sweep_host(h, "cs3_schur_fwd", X, k, true); }
int cs3_schur_bwd(cs3_handle h, double *X, int64_t k) { return schur_sweep_host(h, "cs3_schur_bwd", X, k, false); }

int cs3_free(cs3_handle h)
{
    if (!h) return CS3_OK;
    if (h->on_device) {
        (void) hipDeviceSynchronize();
        release_device(h);
    }
    for (HeldPlan *u : h->plans) u->h = nullptr;            // (their device arrays went with release_device)
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
    if ((rc = refuse_schur(h, "cs3_factor_solve_dev"))) return rc;
    if ((!Ax_dev && h->S.nnzA > 0) || !X_dev) { set_error("cs3_factor_solve_dev: null argument"); return CS3_ERR_ARG; }
    if ((rc = ensure_device(h))) return rc;
    return run_factor_solve(h, Ax_dev, X_dev, X_dev, k, tol, (hipStream_t) stream);
}

int cs3_factor_solve_bx_dev(cs3_handle h, const double *Ax_dev, double tol, const double *B_dev, double *X_dev, int64_t k, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, "cs3_factor_solve_bx_dev"))) return rc;
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

int cs3_set_pivot_perturbation(cs3_handle h, double delta)
{
    int rc = guard(h); if (rc) return rc;
    if (!(delta >= 0.0) || !std::isfinite(delta)) { set_error("cs3_set_pivot_perturbation: delta must be finite and >= 0"); return CS3_ERR_ARG; }
    if (h->S.kind != CS3_LU) { set_error("cs3_set_pivot_perturbation: LU handles only"); return CS3_ERR_ARG; }
    h->perturb_delta = delta;         // (the next factorisation sees the change and drops the graphs captured with the old one)
    return CS3_OK;
}

int cs3_get_perturbed(cs3_handle h, int64_t *count, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!count) { set_error("cs3_get_perturbed: null argument"); return CS3_ERR_ARG; }
    if (!h->on_device || !h->factor_ran) { set_error("cs3_get_perturbed: nothing factorised yet"); return CS3_ERR_STATE; }
    std::vector<int> word((size_t) h->batch);
    hipStream_t st = (hipStream_t) stream;
    CS3_HIP(hipMemcpyAsync(word.data(), h->D.status + 4, word.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    for (size_t b = 0; b < word.size(); ++b) count[b] = word[b];
    return CS3_OK;
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
    if ((rc = refuse_schur(h, "solves and one-sided sweeps"))) return rc;
    if (!X) { set_error("solve: null right-hand side"); return CS3_ERR_ARG; }
    if (trans && mode == 1 && h->S.kind != CS3_LU) { set_error("utsolve: a Cholesky factorisation has no U"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("solve before a successful factorisation"); return CS3_ERR_STATE; }
    const size_t count = (size_t) (h->batch * h->S.n * k);
    DevBuf<double> x;
    CS3_HIP(x.alloc(count));
    CS3_HIP(hipMemcpy(x.get(), X, count * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = trans ? run_solve_t(h, x.get(), k, mode, nullptr) : run_solve(h, x.get(), k, mode, nullptr))) return rc;
    CS3_HIP(hipMemcpy(X, x.get(), count * sizeof(double), hipMemcpyDeviceToHost));
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
    if ((rc = refuse_schur(h, "cs3_export_factor_dev"))) return rc;
    if (h->match.on) { set_error("cs3_export_factor_dev: not available for a matched handle"); return CS3_ERR_ARG; }
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
    if ((rc = refuse_schur(h, "cs3_import_factor_dev"))) return rc;
    if (h->match.on) { set_error("cs3_import_factor_dev: not available for a matched handle"); return CS3_ERR_ARG; }
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
    h->selinv_valid = false;
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

int64_t cs3_debug_launch_plan(cs3_handle h, int32_t op, int64_t nrhs, int32_t trans, int32_t *rows, int64_t cap)
{
    if (guard(h)) return -1;
    if (op < 0 || op > 5 || (op != 0 && (nrhs < 1 || nrhs > INT_MAX))) { set_error("cs3_debug_launch_plan: bad operation or number of right-hand sides"); return -1; }
    const Symbolic &S = h->S;
    const SweepCall call = select_sweep_schedule(h, (int) nrhs, (op == 1 || op == 2) && trans && S.kind == CS3_LU);
    ScheduleInput in;
    in.fgroups = &S.groups; in.sgroups = call.groups;
    in.kind = S.kind; in.nrhs = (op == 0) ? 0 : (int) nrhs; in.batch = h->batch;
    in.forest = !S.sub_forest.empty();
    in.forest_sweeps = call.groups == &S.sgroups1;
    in.fwd_in_factor = op == 3 && nrhs == 1 && in.forest;       // (run_factor_solve)
    LaunchPlan plan = (op == 0) ? plan_factor_levels(in) : (op == 3) ? plan_factor_with_forward(in) : plan_solve_levels(in, op == 1 || op == 4);
    if (op == 3) {
        const LaunchPlan back = plan_solve_levels(in, false);
        plan.insert(plan.end(), back.begin(), back.end());
    }
    for (size_t i = 0; rows && i < plan.size() && (int64_t) i < cap; ++i) {
        const PlanStep &s = plan[i];
        const int32_t row[10] = {s.kind, s.slot, s.g.first, s.g.count, s.g.cls, s.g.level, s.g.max_r, s.g.max_w, s.arg, s.event};
        std::copy(row, row + 10, rows + 10 * i);
    }
    return (int64_t) plan.size();
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
    if (!device_visible()) { set_error("cs3_debug_withhold_handover: no HIP device"); return CS3_ERR_HIP; }
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
    if ((rc = refuse_schur(h, "cs3_get_factors"))) return rc;
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
    auto &E = h->mem.exp;
    if (Lx) {
        if (!E.lmap.get()) CS3_HIP(E.lmap.upload(S.Lmap));
        CS3_HIP(E.lx.reserve((size_t) lnz));
        CS3_HIP(launch_extract(vals, vals_il, DD.il_len, (const long long *) E.lmap.get(), E.lx.get(), lnz, nullptr));
        CS3_HIP(hipMemcpy(Lx, E.lx.get(), (size_t) lnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (Ux) {
        if (!E.umap.get()) CS3_HIP(E.umap.upload(S.Umap));
        CS3_HIP(E.ux.reserve((size_t) unz));
        CS3_HIP(launch_extract(vals, vals_il, DD.il_len, (const long long *) E.umap.get(), E.ux.get(), unz, nullptr));
        CS3_HIP(hipMemcpy(Ux, E.ux.get(), (size_t) unz * sizeof(double), hipMemcpyDeviceToHost));
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
    if (!device_visible()) { set_error("no HIP device visible: triangular solves run on the GPU only"); return CS3_ERR_HIP; }
    DevBuf<int> d_rows, d_rp, d_rj;
    DevBuf<long long> d_rmap, d_diag;
    DevBuf<double> d_gx, d_x;
    std::vector<long long> rmap(T.Rmap.begin(), T.Rmap.end()), diag(T.diag.begin(), T.diag.end());
    CS3_HIP(d_rows.upload(T.level_rows)); CS3_HIP(d_rp.upload(T.Rp)); CS3_HIP(d_rj.upload(T.Rj));
    CS3_HIP(d_rmap.upload(rmap)); CS3_HIP(d_diag.upload(diag)); CS3_HIP(d_gx.upload(Gx, (size_t) Gp[n]));
    CS3_HIP(d_x.upload(x, (size_t) (n * k)));
    for (i32 l = 0; l < T.nlevels; ++l)
        CS3_HIP(launch_tri_level(d_rows.get() + T.level_ptr[l], T.level_ptr[l + 1] - T.level_ptr[l], d_rp.get(), d_rj.get(),
                                 d_rmap.get(), d_diag.get(), d_gx.get(), d_x.get(), (int) k, nullptr));
    CS3_HIP(hipMemcpy(x, d_x.get(), (size_t) (n * k) * sizeof(double), hipMemcpyDeviceToHost));
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
    if (no_device("cs3_csc_matvec")) return CS3_ERR_HIP;
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
    DevBuf<int> d_rp, d_rj;
    DevBuf<double> d_rx, d_x, d_y;
    CS3_HIP(d_rp.upload(Rp)); CS3_HIP(d_rj.upload(Rj)); CS3_HIP(d_rx.upload(Rx));
    CS3_HIP(d_x.alloc((size_t) (n * k)));
    CS3_HIP(d_y.alloc((size_t) (m * k)));
    CS3_HIP(hipMemcpy(d_x.get(), X, (size_t) (n * k) * sizeof(double), hipMemcpyHostToDevice));
    CS3_HIP(launch_matvec_rows(d_rp.get(), d_rj.get(), d_rx.get(), d_x.get(), d_y.get(), m, (int) k, nullptr));
    CS3_HIP(hipMemcpy(Y, d_y.get(), (size_t) (m * k) * sizeof(double), hipMemcpyDeviceToHost));
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
    if (no_device("cs3_csc_stack_4_by_4")) return CS3_ERR_HIP;
    const i64 nnz = (i64) Ap[an] + Bp[bn] + Cp[cn] + Dp[dn];
    struct Blk { const int32_t *p, *i; const double *x; i64 n; DevBuf<int> dp, di; DevBuf<double> dx; };
    Blk blk[4] = {{Ap, Ai, Ax, an}, {Bp, Bi, Bx, bn}, {Cp, Ci, Cx, cn}, {Dp, Di, Dx, dn}};
    for (Blk &b : blk) {
        const size_t bn_ = (size_t) b.p[b.n];
        CS3_HIP(b.dp.alloc((size_t) (b.n + 1)));
        CS3_HIP(b.di.alloc(bn_));
        CS3_HIP(b.dx.alloc(bn_));
        CS3_HIP(hipMemcpy(b.dp.get(), b.p, (size_t) (b.n + 1) * sizeof(int), hipMemcpyHostToDevice));
        if (bn_) CS3_HIP(hipMemcpy(b.di.get(), b.i, bn_ * sizeof(int), hipMemcpyHostToDevice));
        if (bn_) CS3_HIP(hipMemcpy(b.dx.get(), b.x, bn_ * sizeof(double), hipMemcpyHostToDevice));
    }
    const i64 ncol = an + bn;
    DevBuf<int> d_pp, d_pi;
    DevBuf<double> d_px;
    CS3_HIP(d_pp.alloc((size_t) (ncol + 1)));
    CS3_HIP(d_pi.alloc((size_t) nnz));
    CS3_HIP(d_px.alloc((size_t) nnz));
    CS3_HIP(hipMemset(d_pp.get(), 0, (size_t) (ncol + 1) * sizeof(int)));
    CS3_HIP(launch_stack_4_by_4((int) an, (int) bn, (int) am, (int) bm, blk[0].dp.get(), blk[0].di.get(), blk[0].dx.get(),
                                blk[1].dp.get(), blk[1].di.get(), blk[1].dx.get(), blk[2].dp.get(), blk[2].di.get(), blk[2].dx.get(),
                                blk[3].dp.get(), blk[3].di.get(), blk[3].dx.get(), d_pp.get(), d_pi.get(), d_px.get(), nullptr, nullptr));
    CS3_HIP(hipMemcpy(Pp, d_pp.get(), (size_t) (ncol + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (nnz) CS3_HIP(hipMemcpy(Pi, d_pi.get(), (size_t) nnz * sizeof(int), hipMemcpyDeviceToHost));
    if (nnz) CS3_HIP(hipMemcpy(Px, d_px.get(), (size_t) nnz * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- residual and iterative refinement on resident data ---------------------------------
static int ensure_row_view(cs3_handle h, long long k)
{
    int rc = ensure_device(h);
    if (rc) return rc;
    const Symbolic &S = h->S;
    auto &V = h->mem.view;
    if (!V.rp.get()) {
        const i64 n = S.n, nnz = S.nnzA;
        std::vector<int> Rp(n + 1, 0), Rj(nnz), Rmap(nnz);
        const i32 *Ap = h->Ap_host.data(), *Ai = h->Ai_host.data();
        for (i64 p = 0; p < nnz; ++p) ++Rp[Ai[p] + 1];
        for (i64 i = 0; i < n; ++i) Rp[i + 1] += Rp[i];
        std::vector<int> fill(Rp.begin(), Rp.end() - 1);
        for (i64 j = 0; j < n; ++j)                      // ascending column inside every row: csc_mat_vec_ff's summation order
            for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) { const int q = fill[Ai[p]]++; Rj[q] = (int) j; Rmap[q] = (int) p; }
        CS3_HIP(V.rp.upload(Rp)); CS3_HIP(V.rj.upload(Rj)); CS3_HIP(V.rmap.upload(Rmap));
        CS3_HIP(V.maxbits.alloc(1));
    }
    const size_t need = (size_t) (h->batch * S.n * k);
    if (need > V.res.count()) {
        CS3_HIP(hipDeviceSynchronize());              // (the old block may still be in use)
        CS3_HIP(V.res.alloc(need));
    }
    return CS3_OK;
}

// The analysed pattern in column view for the transposed products: row j of A' = column j of A, in storage order
static int ensure_col_view(cs3_handle h, long long k)
{
    int rc = ensure_row_view(h, k);
    if (rc) return rc;
    auto &V = h->mem.view;
    if (!V.cp.get()) {
        std::vector<int> Cmap(h->S.nnzA);
        for (i64 p = 0; p < h->S.nnzA; ++p) Cmap[p] = (int) p;
        CS3_HIP(V.cp.upload(h->Ap_host)); CS3_HIP(V.ci.upload(h->Ai_host)); CS3_HIP(V.cmap.upload(Cmap));
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
    const auto &V = h->mem.view;
    const int *vp = (trans ? V.cp : V.rp).get(), *vj = (trans ? V.ci : V.rj).get(), *vmap = (trans ? V.cmap : V.rmap).get();
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
                  double *last_correction, void *stream, bool trans, const char *who = nullptr)
{
    if (!who) who = trans ? "cs3_refine_t_dev" : "cs3_refine_dev";
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, who))) return rc;
    if (!Ax_dev || !B_dev || !X_dev || k < 1 || k > INT_MAX || steps < 0) { set_error(std::string(who) + ": bad argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": refinement needs a factorisation"); return CS3_ERR_STATE; }
    if ((rc = trans ? ensure_col_view(h, k) : ensure_row_view(h, k))) return rc;
    hipStream_t st = (hipStream_t) stream;
    const long long total = h->batch * h->S.n * k;
    const auto &V = h->mem.view;
    const int *vp = (trans ? V.cp : V.rp).get(), *vj = (trans ? V.ci : V.rj).get(), *vmap = (trans ? V.cmap : V.rmap).get();
    for (int64_t s = 0; s < steps; ++s) {
        CS3_HIP(launch_residual(vp, vj, vmap, Ax_dev, X_dev, B_dev, V.res.get(), h->S.n, (int) k, h->S.nnzA, h->batch, st));
        if ((rc = run_solve(h, V.res.get(), k, 0, st, trans))) return rc;    // d = A \ r (A' \ r) with the factors at hand
        const bool want = last_correction && s + 1 == steps;
        if (want) CS3_HIP(hipMemsetAsync(V.maxbits.get(), 0, sizeof(unsigned long long), st));
        CS3_HIP(launch_axpy_max(X_dev, V.res.get(), total, want ? V.maxbits.get() : nullptr, st));      // x += d
        if (want) {
            unsigned long long bits = 0;
            CS3_HIP(hipMemcpyAsync(&bits, V.maxbits.get(), sizeof(bits), hipMemcpyDeviceToHost, st));
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

// The host-array form: values, right-hand sides and the iterate are staged in HBM (the values through the buffer the
// other host forms use), the steps are cs3_refine_dev's on the null stream -- the same kernels, the same bits.
int cs3_refine(cs3_handle h, const double *Ax, const double *B, double *X, int64_t k, int64_t steps, double *last_correction)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, "cs3_refine"))) return rc;
    if (!Ax || !B || !X || k < 1 || k > INT_MAX || steps < 0) { set_error("cs3_refine: bad argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_refine: refinement needs a factorisation"); return CS3_ERR_STATE; }
    auto &H = h->mem.host;
    const size_t ax_count = (size_t) (h->batch * h->S.nnzA), x_count = (size_t) (h->batch * h->S.n * k);
    CS3_HIP(H.ax.reserve(ax_count));
    if (ax_count) CS3_HIP(hipMemcpy(H.ax.get(), Ax, ax_count * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<double> b, x;
    CS3_HIP(b.alloc(x_count));
    CS3_HIP(x.alloc(x_count));
    if (x_count) {
        CS3_HIP(hipMemcpy(b.get(), B, x_count * sizeof(double), hipMemcpyHostToDevice));
        CS3_HIP(hipMemcpy(x.get(), X, x_count * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = refine(h, H.ax.get(), b.get(), x.get(), k, steps, last_correction, nullptr, false, "cs3_refine"))) return rc;
    if (x_count) CS3_HIP(hipMemcpy(X, x.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- GMRES refinement on the held factors (krylov.hip) ----------------------------------------------------------------
// Work memory of one call, sized by k and by the restart of THIS call (not by KRY_MAX_RESTART).
static int ensure_krylov(cs3_handle h, long long k, int restart, KryWork &K)
{
    auto &M = h->mem.kry;
    const long long n = h->S.n, batch = h->batch, nsys = batch * k, total = batch * n * k, chunks = kry_chunks(n);
    const size_t need_v = (size_t) (total * (restart + 1)), need_w = (size_t) total;
    // per system: R [restart][restart], cs, sn, y [restart], g [restart + 1], the summed dots [2][restart]
    // = restart^2 + (1 + 1 + 1 + 2) restart + (restart + 1)
    const size_t per_sys = (size_t) restart * restart + 6 * (size_t) restart + 1;
    const size_t need_small = (size_t) nsys * per_sys, need_parts = (size_t) (nsys * chunks) * (2 * (size_t) restart + 2);
    if (need_v > M.v.count() || need_w > M.w.count() || need_small > M.small.count() || need_parts > M.parts.count() ||
        (size_t) nsys > M.sys.count() || !M.cnt.get()) {
        CS3_HIP(hipDeviceSynchronize());              // (the old blocks may still be in use)
        h->dbg_syncs += 1;
        CS3_HIP(M.v.reserve(need_v));
        CS3_HIP(M.w.reserve(need_w));
        CS3_HIP(M.z.reserve(need_w));
        CS3_HIP(M.small.reserve(need_small));
        CS3_HIP(M.parts.reserve(need_parts));
        CS3_HIP(M.sys.reserve((size_t) nsys));
        CS3_HIP(M.cnt.reserve(KRY_MAX_RESTART + 2));
    }
    K.V = M.v.get(); K.W = M.w.get(); K.Z = M.z.get(); K.sys = M.sys.get(); K.cnt = M.cnt.get();
    double *p = M.small.get();
    K.R = p; p += (size_t) nsys * restart * restart;
    K.cs = p; p += (size_t) nsys * restart;
    K.sn = p; p += (size_t) nsys * restart;
    K.y = p; p += (size_t) nsys * restart;
    K.g = p; p += (size_t) nsys * (restart + 1);
    K.hsum = p;
    K.parts = M.parts.get();
    K.nparts = K.parts + (size_t) (nsys * chunks) * 2 * restart;
    K.n = n; K.k = k; K.batch = batch; K.chunks = chunks; K.restart = restart;
    h->kry_work = K;
    return CS3_OK;
}

static int gmres_check(const char *who, cs3_handle h, const double *Ax, const double *B, const double *X, int64_t k,
                       int64_t restart, int64_t max_iters, double rtol)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, who))) return rc;
    if (!Ax || !B || !X || k < 1 || k > INT_MAX || restart < 1 || restart > KRY_MAX_RESTART || max_iters < 0 || max_iters > INT_MAX ||
        !(rtol >= 0.0) || !std::isfinite(rtol)) {
        set_error(std::string(who) + ": bad argument");
        return CS3_ERR_ARG;
    }
    if (!h->factored) { set_error(std::string(who) + ": GMRES needs a factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

// One 4-byte "systems still active" word, read after every iteration: the one host synchronisation of the method.
static int read_active(cs3_handle h, const unsigned *cnt_dev, unsigned *out, hipStream_t st)
{
    CS3_HIP(hipMemcpyAsync(out, cnt_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    h->dbg_syncs += 1;
    return CS3_OK;
}

static int gmres_run(const char *who, cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k,
                     int64_t restart, int64_t max_iters, double rtol, bool trans, int32_t *iters, double *relres, hipStream_t st)
{
    int rc = gmres_check(who, h, Ax_dev, B_dev, X_dev, k, restart, max_iters, rtol);
    if (rc) return rc;
    const long long nsys = h->batch * k;
    if (h->S.n == 0 || nsys == 0) {
        for (long long s = 0; s < nsys; ++s) { if (iters) iters[s] = 0; if (relres) relres[s] = 0.0; }
        return CS3_OK;
    }
    if ((rc = trans ? ensure_col_view(h, 0) : ensure_row_view(h, 0))) return rc;
    KryWork K{};
    if ((rc = ensure_krylov(h, k, (int) restart, K))) return rc;
    const auto &V = h->mem.view;
    const int *vp = (trans ? V.cp : V.rp).get(), *vj = (trans ? V.ci : V.rj).get(), *vmap = (trans ? V.cmap : V.rmap).get();
    const long long n = h->S.n, nnz = h->S.nnzA, batch = h->batch;
    const int m = (int) restart, cap = (int) max_iters;
    // every system does at least one iteration in a cycle it enters, so max_iters + 1 cycles see every system finish
    for (long long cycle = 0; cycle <= (long long) cap; ++cycle) {
        CS3_HIP(launch_residual(vp, vj, vmap, Ax_dev, X_dev, B_dev, K.W, n, (int) k, nnz, batch, st));     // r = b - A x
        CS3_HIP(launch_kry_start(K, B_dev, X_dev, cycle == 0, rtol, cap, st));
        unsigned active = 0;
        if ((rc = read_active(h, K.cnt, &active, st))) return rc;
        if (!active) break;
        int cols = 0;
        while (active && cols < m) {
            if ((rc = run_solve(h, K.Z, k, 0, st, trans))) return rc;                                     // z = M^-1 v_j
            CS3_HIP(launch_residual(vp, vj, vmap, Ax_dev, K.Z, nullptr, K.W, n, (int) k, nnz, batch, st));  // w = A z
            CS3_HIP(launch_kry_step(K, cols, rtol, cap, st));
            if ((rc = read_active(h, K.cnt + 1 + cols, &active, st))) return rc;
            ++cols;
        }
        CS3_HIP(launch_kry_combine(K, cols, st));                                                         // u = V y
        if ((rc = run_solve(h, K.Z, k, 0, st, trans))) return rc;                                         // x += M^-1 u
        CS3_HIP(launch_kry_axpy(K, X_dev, st));
    }
    if (iters || relres) {
        std::vector<KrySys> sys((size_t) nsys);
        CS3_HIP(hipMemcpyAsync(sys.data(), K.sys, sys.size() * sizeof(KrySys), hipMemcpyDeviceToHost, st));
        CS3_HIP(hipStreamSynchronize(st));
        for (long long s = 0; s < nsys; ++s) {
            if (iters) iters[s] = sys[(size_t) s].iters;
            if (relres) relres[s] = sys[(size_t) s].relres;
        }
    }
    return CS3_OK;
}

int cs3_gmres_limits(cs3_gmres_limits_t *out)
{
    if (!out) { set_error("cs3_gmres_limits: null argument"); return CS3_ERR_ARG; }
    out->max_restart = KRY_MAX_RESTART;
    out->chunk_rows = KRY_CHUNK;
    out->rhs_tile = KRY_RHS_TILE;
    return CS3_OK;
}

int cs3_gmres_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, int64_t k, int64_t restart,
                  int64_t max_iters, double rtol, int64_t trans, int32_t *iters, double *relres, void *stream)
{
    return gmres_run("cs3_gmres_dev", h, Ax_dev, B_dev, X_dev, k, restart, max_iters, rtol, trans != 0, iters, relres,
                     (hipStream_t) stream);
}

// The host-array form: staged as cs3_refine stages, then cs3_gmres_dev's steps on the null stream -- the same bits.
int cs3_gmres(cs3_handle h, const double *Ax, const double *B, double *X, int64_t k, int64_t restart, int64_t max_iters,
              double rtol, int64_t trans, int32_t *iters, double *relres)
{
    int rc = gmres_check("cs3_gmres", h, Ax, B, X, k, restart, max_iters, rtol);
    if (rc) return rc;
    auto &H = h->mem.host;
    const size_t ax_count = (size_t) (h->batch * h->S.nnzA), x_count = (size_t) (h->batch * h->S.n * k);
    CS3_HIP(H.ax.reserve(ax_count));
    if (ax_count) CS3_HIP(hipMemcpy(H.ax.get(), Ax, ax_count * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<double> b, x;
    CS3_HIP(b.alloc(x_count));
    CS3_HIP(x.alloc(x_count));
    if (x_count) {
        CS3_HIP(hipMemcpy(b.get(), B, x_count * sizeof(double), hipMemcpyHostToDevice));
        CS3_HIP(hipMemcpy(x.get(), X, x_count * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = gmres_run("cs3_gmres", h, H.ax.get(), b.get(), x.get(), k, restart, max_iters, rtol, trans != 0, iters, relres, nullptr)))
        return rc;
    if (x_count) CS3_HIP(hipMemcpy(X, x.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// diagnostics (tools/bench_gmres.py): one vector kernel of iteration j on the work memory of the last cs3_gmres* call, as
// that call shaped it (which = 0: the multi-dot, 1: the first update, 2: the second update with the norm)
int cs3_debug_gmres_kernel(cs3_handle h, int64_t which, int64_t j, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!h->kry_work.V) { set_error("cs3_debug_gmres_kernel: no cs3_gmres call on this handle yet"); return CS3_ERR_STATE; }
    if (which < 0 || which > 2 || j < 0 || j >= h->kry_work.restart) { set_error("cs3_debug_gmres_kernel: bad argument"); return CS3_ERR_ARG; }
    CS3_HIP(launch_kry_probe(h->kry_work, (int) which, (int) j, (hipStream_t) stream));
    return CS3_OK;
}

// diagnostics: the residual estimate of the recurrence, |g_{j+1}| / ||b||, that every system of the last cs3_gmres* call
// on this handle ended its last cycle with (0 for a system that never iterated); est [count], count = batch * k of that call
int cs3_debug_gmres_estimates(cs3_handle h, double *est, int64_t count)
{
    int rc = guard(h); if (rc) return rc;
    if (!est || count < 0 || (size_t) count > h->mem.kry.sys.count()) { set_error("cs3_debug_gmres_estimates: bad argument"); return CS3_ERR_ARG; }
    std::vector<KrySys> sys((size_t) count);
    if (count) CS3_HIP(hipMemcpy(sys.data(), h->mem.kry.sys.get(), sys.size() * sizeof(KrySys), hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < count; ++s) est[s] = sys[(size_t) s].est;
    return CS3_OK;
}

// diagnostics: the first nvec <= restart + 1 basis vectors as the last cs3_gmres* call on this handle left them, V [nvec]
// [batch][n, k] as stored.  Vector 0 is what the call's closing residual check left (zeros once every system has
// finished); vectors 1 .. belong to the last cycle that iterated, and whatever an earlier cycle left behind it.
int cs3_debug_gmres_basis(cs3_handle h, double *V, int64_t nvec)
{
    int rc = guard(h); if (rc) return rc;
    if (!V || nvec < 0 || nvec > KRY_MAX_RESTART + 1) { set_error("cs3_debug_gmres_basis: bad argument"); return CS3_ERR_ARG; }
    const KryWork &K = h->kry_work;
    if (!K.V) { set_error("cs3_debug_gmres_basis: no cs3_gmres call on this handle yet"); return CS3_ERR_STATE; }
    if (nvec > K.restart + 1) { set_error("cs3_debug_gmres_basis: bad argument"); return CS3_ERR_ARG; }
    const size_t count = (size_t) nvec * (size_t) (K.batch * K.n * K.k);
    if (count) CS3_HIP(hipMemcpy(V, K.V, count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- extra-precise refinement: doubled-precision residuals, berr and ferr (refine_xp.hip) ----------------------------
int cs3_refine_xp_limits(cs3_refine_xp_limits_t *out)
{
    if (!out) { set_error("cs3_refine_xp_limits: null argument"); return CS3_ERR_ARG; }
    out->block = XP_BLOCK;
    out->grid_cap = XP_GRID_CAP;
    out->max_iters_default = XP_MAX_ITERS_DEFAULT;
    out->eps = XP_EPS;
    out->stall_ratio = XP_STALL_RATIO;
    out->maxima_grid_cap = XP_MAXIMA_GRID_CAP;
    return CS3_OK;
}

static int residual_xp_check(const char *who, cs3_handle h, const double *Ax, const double *B, const double *X, const double *R,
                             int64_t k)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, who))) return rc;
    if (!Ax || !B || !X || !R || k < 1 || k > INT_MAX) { set_error(std::string(who) + ": bad argument"); return CS3_ERR_ARG; }
    return CS3_OK;
}

static int residual_xp_run(const char *who, cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev,
                           const double *XT_dev, double *R_dev, double *S_dev, int64_t k, bool trans, hipStream_t st)
{
    int rc = residual_xp_check(who, h, Ax_dev, B_dev, X_dev, R_dev, k);
    if (rc) return rc;
    if ((rc = trans ? ensure_col_view(h, 0) : ensure_row_view(h, 0))) return rc;
    const auto &V = h->mem.view;
    const int *vp = (trans ? V.cp : V.rp).get(), *vj = (trans ? V.ci : V.rj).get(), *vmap = (trans ? V.cmap : V.rmap).get();
    CS3_HIP(launch_residual_xp(vp, vj, vmap, Ax_dev, B_dev, X_dev, XT_dev, R_dev, S_dev, h->S.n, (int) k, h->S.nnzA, h->batch,
                               false, st));
    return CS3_OK;
}

int cs3_residual_xp_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, const double *X_dev, const double *XT_dev,
                        double *R_dev, double *S_dev, int64_t k, int64_t trans, void *stream)
{
    return residual_xp_run("cs3_residual_xp_dev", h, Ax_dev, B_dev, X_dev, XT_dev, R_dev, S_dev, k, trans != 0, (hipStream_t) stream);
}

// The host-array form: staged as cs3_refine stages, the same kernel on the null stream.
int cs3_residual_xp(cs3_handle h, const double *Ax, const double *B, const double *X, const double *XT, double *R, double *S,
                    int64_t k, int64_t trans)
{
    int rc = residual_xp_check("cs3_residual_xp", h, Ax, B, X, R, k);
    if (rc) return rc;
    if ((rc = ensure_device(h))) return rc;
    auto &H = h->mem.host;
    const size_t ax_count = (size_t) (h->batch * h->S.nnzA), x_count = (size_t) (h->batch * h->S.n * k);
    CS3_HIP(H.ax.reserve(ax_count));
    if (ax_count) CS3_HIP(hipMemcpy(H.ax.get(), Ax, ax_count * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<double> b, x, xt, r, s;
    for (DevBuf<double> *buf : {&b, &x, &r}) CS3_HIP(buf->alloc(x_count));
    if (XT) CS3_HIP(xt.alloc(x_count));
    if (S) CS3_HIP(s.alloc(x_count));
    if (x_count) {
        CS3_HIP(hipMemcpy(b.get(), B, x_count * sizeof(double), hipMemcpyHostToDevice));
        CS3_HIP(hipMemcpy(x.get(), X, x_count * sizeof(double), hipMemcpyHostToDevice));
        if (XT) CS3_HIP(hipMemcpy(xt.get(), XT, x_count * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = residual_xp_run("cs3_residual_xp", h, H.ax.get(), b.get(), x.get(), XT ? xt.get() : nullptr, r.get(),
                              S ? s.get() : nullptr, k, trans != 0, nullptr)))
        return rc;
    if (x_count) {
        CS3_HIP(hipMemcpy(R, r.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
        if (S) CS3_HIP(hipMemcpy(S, s.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
    }
    return CS3_OK;
}

// Work memory of one call: the views with the residual vector at this k, the tail, the states, the counter.
static int ensure_refine_xp(cs3_handle h, long long k, bool trans)
{
    const size_t res_before = h->mem.view.res.count();
    int rc = trans ? ensure_col_view(h, k) : ensure_row_view(h, k);
    if (rc) return rc;
    if (h->mem.view.res.count() != res_before) h->dbg_allocs += 1;
    auto &M = h->mem.xpr;
    const size_t total = (size_t) (h->batch * h->S.n * k), nsys = (size_t) (h->batch * k);
    if (total > M.tail.count() || nsys > M.sys.count() || !M.tail.get() || !M.sys.get() || !M.cnt.get()) {
        CS3_HIP(hipDeviceSynchronize());              // (the old blocks may still be in use)
        h->dbg_syncs += 1;
        const double *t0 = M.tail.get(); const XpSys *s0 = M.sys.get(); const unsigned *c0 = M.cnt.get();
        CS3_HIP(M.tail.reserve(total));
        CS3_HIP(M.sys.reserve(nsys));
        CS3_HIP(M.cnt.reserve(1));
        h->dbg_allocs += (M.tail.get() != t0) + (M.sys.get() != s0) + (M.cnt.get() != c0);
    }
    return CS3_OK;
}

static int refine_xp_check(const char *who, cs3_handle h, const double *Ax, const double *B, const double *X, int64_t k,
                           int64_t max_iters)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, who))) return rc;
    if (!Ax || !B || !X || k < 1 || k > INT_MAX || max_iters < 0 || max_iters > INT_MAX) {
        set_error(std::string(who) + ": bad argument");
        return CS3_ERR_ARG;
    }
    if (!h->factored) { set_error(std::string(who) + ": refinement needs a factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

// The forward bound of one system from what the iteration and the closing pass left (the rules of the header, in order).
static double xp_ferr(const XpSys &s, double nxf)
{
    if (s.flag == XP_NONFINITE) return std::nan("");
    if (s.iters == 0) return HUGE_VAL;
    if (s.rate >= 1.0) return HUGE_VAL;
    if (s.nd_prev == 0.0 && nxf == 0.0) return 0.0;
    return std::max(XP_EPS, (s.nd_prev / nxf) / (1.0 - s.rate));
}

static int refine_xp_run(const char *who, cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, double *XT_dev,
                         int64_t k, int64_t max_iters, bool trans, int32_t *iters, int32_t *flag, double *ferr, double *berr,
                         double *rate, hipStream_t st)
{
    int rc = refine_xp_check(who, h, Ax_dev, B_dev, X_dev, k, max_iters);
    if (rc) return rc;
    const long long n = h->S.n, nnz = h->S.nnzA, batch = h->batch, nsys = batch * k;
    if ((rc = ensure_refine_xp(h, k, trans))) return rc;
    const auto &V = h->mem.view;
    auto &M = h->mem.xpr;
    const int *vp = (trans ? V.cp : V.rp).get(), *vj = (trans ? V.ci : V.rj).get(), *vmap = (trans ? V.cmap : V.rmap).get();
    double *res = V.res.get(), *tail = M.tail.get();
    const size_t vec_bytes = (size_t) (batch * n * k) * sizeof(double);
    if (vec_bytes) CS3_HIP(hipMemsetAsync(tail, 0, vec_bytes, st));
    CS3_HIP(hipMemsetAsync(M.sys.get(), 0, (size_t) nsys * sizeof(XpSys), st));       // iterating, no correction yet
    unsigned active = (n > 0 && nsys > 0) ? 1u : 0u;
    for (int64_t s = 0; s < max_iters && active; ++s) {
        CS3_HIP(launch_residual_xp(vp, vj, vmap, Ax_dev, B_dev, X_dev, tail, res, nullptr, n, (int) k, nnz, batch, false, st));
        if ((rc = run_solve(h, res, k, 0, st, trans))) return rc;                      // dx = op(A)^-1 r with the factors at hand
        CS3_HIP(launch_xp_maxima(res, X_dev, M.sys.get(), n, (int) k, batch, st));
        CS3_HIP(hipMemsetAsync(M.cnt.get(), 0, sizeof(unsigned), st));
        CS3_HIP(launch_xp_control(M.sys.get(), nsys, M.cnt.get(), st));
        CS3_HIP(launch_xp_update(X_dev, tail, res, M.sys.get(), n, (int) k, batch, st));
        if ((rc = read_active(h, M.cnt.get(), &active, st))) return rc;
    }
    // the closing pass on x alone: |r_i| / s_i into res, its maxima and those of |x| into the (zeroed) words of the states
    CS3_HIP(launch_residual_xp(vp, vj, vmap, Ax_dev, B_dev, X_dev, nullptr, res, nullptr, n, (int) k, nnz, batch, true, st));
    CS3_HIP(launch_xp_maxima(res, X_dev, M.sys.get(), n, (int) k, batch, st));
    if (XT_dev && vec_bytes) CS3_HIP(hipMemcpyAsync(XT_dev, tail, vec_bytes, hipMemcpyDeviceToDevice, st));
    std::vector<XpSys> sys((size_t) nsys);
    if (nsys) CS3_HIP(hipMemcpyAsync(sys.data(), M.sys.get(), sys.size() * sizeof(XpSys), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    h->dbg_syncs += 1;
    for (long long s = 0; s < nsys; ++s) {
        const XpSys &y = sys[(size_t) s];
        double be, nxf;
        std::memcpy(&be, &y.nd_bits, sizeof(double));
        std::memcpy(&nxf, &y.nx_bits, sizeof(double));
        if (iters) iters[s] = y.iters;
        if (flag) flag[s] = y.flag;
        if (ferr) ferr[s] = xp_ferr(y, nxf);
        if (berr) berr[s] = be;
        if (rate) rate[s] = y.rate;
    }
    return CS3_OK;
}

int cs3_refine_xp_dev(cs3_handle h, const double *Ax_dev, const double *B_dev, double *X_dev, double *XT_dev, int64_t k,
                      int64_t max_iters, int64_t trans, int32_t *iters, int32_t *flag, double *ferr, double *berr, double *rate,
                      void *stream)
{
    return refine_xp_run("cs3_refine_xp_dev", h, Ax_dev, B_dev, X_dev, XT_dev, k, max_iters, trans != 0, iters, flag, ferr, berr,
                         rate, (hipStream_t) stream);
}

// The host-array form: staged as cs3_refine stages, then cs3_refine_xp_dev's steps on the null stream -- the same bits.
int cs3_refine_xp(cs3_handle h, const double *Ax, const double *B, double *X, double *XT, int64_t k, int64_t max_iters,
                  int64_t trans, int32_t *iters, int32_t *flag, double *ferr, double *berr, double *rate)
{
    int rc = refine_xp_check("cs3_refine_xp", h, Ax, B, X, k, max_iters);
    if (rc) return rc;
    auto &H = h->mem.host;
    const size_t ax_count = (size_t) (h->batch * h->S.nnzA), x_count = (size_t) (h->batch * h->S.n * k);
    CS3_HIP(H.ax.reserve(ax_count));
    if (ax_count) CS3_HIP(hipMemcpy(H.ax.get(), Ax, ax_count * sizeof(double), hipMemcpyHostToDevice));
    DevBuf<double> b, x, xt;
    CS3_HIP(b.alloc(x_count));
    CS3_HIP(x.alloc(x_count));
    if (XT) CS3_HIP(xt.alloc(x_count));
    if (x_count) {
        CS3_HIP(hipMemcpy(b.get(), B, x_count * sizeof(double), hipMemcpyHostToDevice));
        CS3_HIP(hipMemcpy(x.get(), X, x_count * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = refine_xp_run("cs3_refine_xp", h, H.ax.get(), b.get(), x.get(), XT ? xt.get() : nullptr, k, max_iters, trans != 0,
                            iters, flag, ferr, berr, rate, nullptr)))
        return rc;
    if (x_count) {
        CS3_HIP(hipMemcpy(X, x.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
        if (XT) CS3_HIP(hipMemcpy(XT, xt.get(), x_count * sizeof(double), hipMemcpyDeviceToHost));
    }
    return CS3_OK;
}

// ---- condition estimates and log-determinants from the held factors --------------------------------------------------
static int ensure_estimator(cs3_handle h)
{
    int rc = ensure_col_view(h, 0);
    if (rc) return rc;
    auto &E = h->mem.est;
    const size_t bn = (size_t) (h->batch * h->S.n);
    const long long nparts = std::max(est_chunks(h->S.n), norm_chunks(h->S.n));
    CS3_HIP(E.x.reserve(bn));
    CS3_HIP(E.s.reserve(2 * bn));
    CS3_HIP(E.state.reserve((size_t) h->batch));
    CS3_HIP(E.parts.reserve((size_t) (h->batch * nparts)));
    CS3_HIP(E.cnt.reserve(2));
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
    const auto &E = h->mem.est;
    CS3_HIP(launch_est_start(h->mem.view.cp.get(), h->mem.view.cmap.get(), Ax_dev, n, h->S.nnzA, batch, E.parts.get(), E.state.get(), st));
    constexpr int FIXED_SLOTS = 11;
    unsigned want[2] = {1u, 0u};                             // before the first slot: J1 wants A^-1
    int last = 1;
    // (adaptive: a wanted kind runs at most one slot late, so 2 * 11 slots bound every matrix's 11 steps)
    for (int slot = 0; slot < (adaptive ? 2 * FIXED_SLOTS : FIXED_SLOTS); ++slot) {
        int kind = slot & 1;                                 // 0: x = A^-1 b (F), 1: x = A^-T b (T)
        if (adaptive) {
            if (slot > 0) {
                CS3_HIP(hipMemcpyAsync(want, E.cnt.get(), sizeof(want), hipMemcpyDeviceToHost, st));
                CS3_HIP(hipStreamSynchronize(st));
            }
            if (!want[0] && !want[1]) break;
            kind = (want[0] && want[1]) ? 1 - last : (want[0] ? 0 : 1);
        }
        if (chol) kind = 0;
        const int kmask = chol ? 3 : 1 << kind;
        CS3_HIP(launch_est_prepare(E.state.get(), E.s.get(), E.x.get(), n, batch, kmask, E.cnt.get(), st));
        if ((rc = run_solve(h, E.x.get(), 1, 0, st, kind == 1))) return rc;
        CS3_HIP(launch_est_consume(E.state.get(), E.s.get(), E.x.get(), n, batch, kmask, E.parts.get(), E.cnt.get(), st));
        last = kind;
    }
    CS3_HIP(launch_est_finalize(E.state.get(), batch, cond_dev, inv_dev, st));
    return CS3_OK;
}

static int condest_check(const char *who, cs3_handle h, const double *Ax, const double *cond)
{
    int rc = guard(h); if (rc) return rc;
    if ((rc = refuse_schur(h, who))) return rc;
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
    CS3_HIP(h->mem.host.out.reserve((size_t) (2 * h->batch)));
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
    auto &H = h->mem.host;
    const size_t ax_count = (size_t) (batch * h->S.nnzA);
    CS3_HIP(H.ax.reserve(ax_count));
    if (ax_count) CS3_HIP(hipMemcpy(H.ax.get(), Ax, ax_count * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = condest_run(h, H.ax.get(), H.out.get(), H.out.get() + batch, nullptr, true))) return rc;
    std::vector<double> out((size_t) (2 * batch));
    CS3_HIP(hipMemcpy(out.data(), H.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(cond, out.data(), (size_t) batch * sizeof(double));
    if (inv_norm) std::memcpy(inv_norm, out.data() + batch, (size_t) batch * sizeof(double));
    return CS3_OK;
}

// sign and log|det| from the diagonal of the held factors: pivot j's diagonal sits at virtual pool offset
// lpan_off[s] + jj (r + 1), s = col2sn[j], jj = j - sn_ptr[s], r = the front order (build_csc_factors' rule); the map is
// built once per handle, without the CSC view of the factors.
static int ensure_diag_map(cs3_handle h)
{
    if (h->mem.diag.get()) return CS3_OK;
    const Symbolic &S = h->S;
    std::vector<i64> diag((size_t) S.n);
    for (i64 j = 0; j < S.n; ++j) {
        const i32 s = S.col2sn[j];
        diag[j] = S.lpan_off[s] + (j - S.sn_ptr[s]) * (S.st_ptr[s + 1] - S.st_ptr[s] + 1);
    }
    CS3_HIP(h->mem.diag.upload(diag));
    return CS3_OK;
}

int cs3_slogdet_dev(cs3_handle h, double *sign_dev, double *logabs_dev, void *stream)
{
    int rc = guard(h); if (rc) return rc;
    if (!sign_dev || !logabs_dev) { set_error("cs3_slogdet_dev: null argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_slogdet_dev: no successful factorisation"); return CS3_ERR_STATE; }
    if ((rc = ensure_diag_map(h))) return rc;
    CS3_HIP(launch_slogdet(h->D, (const long long *) h->mem.diag.get(), sign_dev, logabs_dev, (hipStream_t) stream));
    if (h->match.on)                                               // of A, not of B
        CS3_HIP(launch_match_slogdet(sign_dev, logabs_dev, h->batch, h->match.parity, h->match.log_shift, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_slogdet(cs3_handle h, double *sign, double *logabs)
{
    int rc = guard(h); if (rc) return rc;
    if (!sign || !logabs) { set_error("cs3_slogdet: null argument"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error("cs3_slogdet: no successful factorisation"); return CS3_ERR_STATE; }
    if ((rc = ensure_host_out(h))) return rc;
    const long long batch = h->batch;
    double *d_out = h->mem.host.out.get();
    if ((rc = cs3_slogdet_dev(h, d_out, d_out + batch, nullptr))) return rc;
    std::vector<double> out((size_t) (2 * batch));
    CS3_HIP(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(sign, out.data(), (size_t) batch * sizeof(double));
    std::memcpy(logabs, out.data() + batch, (size_t) batch * sizeof(double));
    return CS3_OK;
}

int64_t cs3_debug_live_device_buffers(void) { return (int64_t) g_live_device_buffers.load(); }

int cs3_debug_alloc_counters(cs3_handle h, int64_t *allocs, int64_t *syncs)
{
    int rc = guard(h); if (rc) return rc;
    if (allocs) *allocs = h->dbg_allocs;
    if (syncs) *syncs = h->dbg_syncs;
    return CS3_OK;
}

// ---- complex Schur handles: the complex S out of the real one (cplxsens.hip) -------------------------------------------
static int cplx_schur_check(const char *who, cs3_cplx p, cs3_handle h, const double *S)
{
    int rc = guard(h); if (rc) return rc;
    if (!p) { set_error(std::string(who) + ": null complex plan"); return CS3_ERR_ARG; }
    if (h->S.schur_sn < 0) { set_error(std::string(who) + ": the handle has no Schur set (cs3_analyze_schur)"); return CS3_ERR_STATE; }
    if (!S) { set_error(std::string(who) + ": null buffer"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(std::string(who) + ": called before a successful factorisation"); return CS3_ERR_STATE; }
    if (p->schur_idx.empty()) { set_error(std::string(who) + ": the plan has no border (cs3_cplx_plan_create_schur)"); return CS3_ERR_STATE; }
    if (h->S.schur_idx.size() != 2 * p->schur_idx.size() || h->batch != p->batch) {
        set_error(std::string(who) + ": the handle's Schur set is not the 2 ns rows of the plan's border (or the batches differ)");
        return CS3_ERR_ARG;
    }
    return CS3_OK;
}

int cs3_cplx_schur_get_dev(cs3_cplx p, cs3_handle h, double *S_dev, void *stream)
{
    const char *who = "cs3_cplx_schur_get_dev";
    int rc = cplx_schur_check(who, p, h, S_dev);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(S_dev) & 15) { set_error(std::string(who) + ": S_dev must be aligned to 16 bytes"); return CS3_ERR_ARG; }
    CS3_HIP(launch_cplx_schur_gather(h->D.schur, h->batch, (long long) p->schur_idx.size(), S_dev, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_cplx_schur_get(cs3_cplx p, cs3_handle h, double *S)
{
    int rc = cplx_schur_check("cs3_cplx_schur_get", p, h, S);
    if (rc) return rc;
    const size_t count = 2 * (size_t) h->batch * p->schur_idx.size() * p->schur_idx.size();
    DevBuf<double> s;
    CS3_HIP(s.alloc(count));
    CS3_HIP(launch_cplx_schur_gather(h->D.schur, h->batch, (long long) p->schur_idx.size(), s.get(), nullptr));
    CS3_HIP(hipMemcpy(S, s.get(), count * sizeof(double), hipMemcpyDeviceToHost));
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
    if (no_device("cs3_csc_stack_4_by_4_dev")) return CS3_ERR_HIP;
    CS3_HIP(launch_stack_4_by_4((int) an, (int) bn, (int) am, (int) bm, Ap, Ai, Ax, Bp, Bi, Bx, Cp, Ci, Cx, Dp, Di, Dx, Pp, Pi, Px,
                                map, (hipStream_t) stream));
    return CS3_OK;
}

int cs3_restack_values_dev(int64_t nnz, const int32_t *map, int64_t nnz_a, int64_t nnz_b, int64_t nnz_c,
                           const double *Ax, const double *Bx, const double *Cx, const double *Dx, double *Px, void *stream)
{
    if (nnz < 0 || nnz_a < 0 || nnz_b < 0 || nnz_c < 0 || (nnz > 0 && (!map || !Px))) { set_error("cs3_restack_values_dev: bad argument"); return CS3_ERR_ARG; }
    if (no_device("cs3_restack_values_dev")) return CS3_ERR_HIP;
    CS3_HIP(launch_restack_values(nnz, map, nnz_a, nnz_b, nnz_c, Ax, Bx, Cx, Dx, Px, (hipStream_t) stream));
    return CS3_OK;
}

}  // extern "C"
