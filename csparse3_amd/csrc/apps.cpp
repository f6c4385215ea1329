// The applications on a factorised handle (include/csparse3_amd.h): low-rank-modified solves (cs3_updates_*), sparse
// right-hand sides (cs3_sens_*), selected inversion (cs3_selinv_*), the complex forms of all three behind a complex plan
// and a handle on its real form, and the bilinear forms on the selected inverse (cs3_quad_*).  Host drivers only: plans, checks, workspace, and the order of the launches; the
// solves themselves are the handle's (run_solve in api.cpp).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "cs3_cplx.hpp"
#include "cs3_handle.hpp"

using namespace cs3;

namespace {

// ---- real and complex plans: what differs, written once ------------------------------------------------------------------
// One call's scalar width: doubles per number, the complex plan (null for a real call, and for a complex call that was
// given none: the checks refuse it), the entry point's name for the messages, and the launches -- the real kernels, or
// behind a complex plan the complex ones, which take its rotation s (the units) or a CsensGlue on top.
struct PlanFlavor {
    int cpl;
    cs3_cplx p;
    const char *who;
    bool complex() const { return cpl == 2; }
    std::string name() const { return who; }
    const double *s() const { return p ? p->d_s.get() : nullptr; }

    hipError_t prepare_updates() const { return p ? prepare_cupd_kernels() : prepare_updates_kernels(); }
    hipError_t upd_units(double *Z, long long n, int t, const int *unit_row, hipStream_t st) const
    {
        return p ? launch_cupd_units(Z, n, t, unit_row, s(), st) : launch_upd_units(Z, n, t, unit_row, st);
    }
    hipError_t upd_capacitance(const UpdTables &T, const double *cx, const double *Z, int t, const double *x0, int c0, int nc, double sing_tol,
                               double *rpiv, hipStream_t st) const
    {
        return (p ? launch_cupd_capacitance : launch_upd_capacitance)(T, cx, Z, t, x0, c0, nc, sing_tol, rpiv, st);
    }
    hipError_t upd_apply(const UpdTables &T, const double *Z, int t, const double *x0, long long n, int c0, int nc, int rmax, long long ldx,
                         double *X, hipStream_t st) const
    {
        return (p ? launch_cupd_apply : launch_upd_apply)(T, Z, t, x0, n, c0, nc, rmax, ldx, X, st);
    }
    hipError_t sens_scatter(double *T, long long n, int w, const SensOperand &op, long long c0, int t, const CsensGlue &g, hipStream_t st) const
    {
        return p ? launch_csens_scatter(T, n, w, CsensOperand{op.p, op.i, op.x}, c0, t, g, st) : launch_sens_scatter(T, n, w, op, c0, t, st);
    }
    hipError_t sens_combine(const double *T, int w, int t, const SensOperand &op, long long ng, long long c0, long long ldy, bool transposed,
                            const CsensGlue &g, double *Y, hipStream_t st) const
    {
        return p ? launch_csens_combine(T, w, t, CsensOperand{op.p, op.i, op.x}, ng, c0, ldy, transposed, g, Y, st)
                 : launch_sens_combine(T, w, t, op, ng, c0, ldy, transposed, Y, st);
    }
};
PlanFlavor real_flavor(const char *who) { return PlanFlavor{1, nullptr, who}; }
PlanFlavor cplx_flavor(cs3_cplx p, const char *who) { return PlanFlavor{2, p, who}; }

int bad_arg(const char *who, const char *msg) { set_error(std::string(who) + ": " + msg); return CS3_ERR_ARG; }

// A complex array as the device forms take it: 16-byte aligned (a real call has no such rule)
bool misaligned(const PlanFlavor &F, bool device, uintptr_t used) { return F.complex() && device && (used & 15); }
uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// Frees a plan of any kind.  While its handle lives the plan leaves the handle's list, after the work that may still read
// its device copies; a plan whose handle went first has neither.
int plan_free(HeldPlan *u)
{
    if (!u) return CS3_OK;
    if (u->h) {
        if (u->on_device) { (void) hipDeviceSynchronize(); u->drop_device(); }
        auto &pl = u->h->plans;
        pl.erase(std::remove(pl.begin(), pl.end(), u), pl.end());
    }
    delete u;
    return CS3_OK;
}

// A tile buffer of the handle, `need` doubles.  A wider plan than any before: the old tile may still be in use.
int grow_tile(cs3_handle h, DevBuf<double> &T, size_t need)
{
    if (T.count() >= need) return CS3_OK;
    if (T.get()) {
        CS3_HIP(hipDeviceSynchronize());
        h->dbg_syncs += 1;
    }
    CS3_HIP(T.alloc(need));
    h->dbg_allocs += 1;
    return CS3_OK;
}

// ---- many low-rank-modified systems (A + dA_c) x = b on the held factors (updates.hip, cplxupd.hip) ---------------------
// Plan: per case its distinct rows R_c and columns C_c (ascending) and the entry of D_c every triplet adds to; the cases
// in their order cut into tiles (a case joins the current tile unless the union of touched rows would pass the tile
// width, or the tile already has UPD_MAX_TILE_CASES cases); per tile the touched rows in order of first use = the columns
// of its Z.  A row that cases of two tiles touch is a column of both.
int updates_build(cs3_updates_s &u, int64_t n, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj, const char *who)
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
            set_error(std::string(who) + ": case " + std::to_string(c) + " touches " + std::to_string(rows.size()) + " rows and " +
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

// What both plan calls do once their leading checks have passed: the case lists (ncases, cp monotone from 0, the index
// arrays and their range, in this order; n: the order the indices live in), the plan (which refuses a case of more than
// 16 rows or columns), then what the header puts behind that -- a batched handle; for a complex plan p also a batched
// plan, a plan with a border and a Schur handle --, and the plan joins its handle.
template <class Plan>
int updates_plan_make(const char *who_, cs3_cplx p, cs3_handle h, int64_t n, int64_t ncases, const int32_t *cp, const int32_t *ci,
                      const int32_t *cj, Plan **out)
{
    const std::string who(who_);
    if (ncases < 1 || ncases > INT_MAX / 2) { set_error(who + ": ncases must be >= 1"); return CS3_ERR_ARG; }
    if (cp[0] != 0) { set_error(who + ": cp[0] != 0"); return CS3_ERR_ARG; }
    for (int64_t c = 0; c < ncases; ++c)
        if (cp[c + 1] < cp[c]) { set_error(who + ": cp not monotone at case " + std::to_string(c)); return CS3_ERR_ARG; }
    if (cp[ncases] > 0 && (!ci || !cj)) { set_error(who + ": null index arrays"); return CS3_ERR_ARG; }
    for (int64_t c = 0; c < ncases; ++c)
        for (int e = cp[c]; e < cp[c + 1]; ++e)
            if (ci[e] < 0 || ci[e] >= n || cj[e] < 0 || cj[e] >= n) {
                set_error(who + ": index out of range in case " + std::to_string(c));
                return CS3_ERR_ARG;
            }
    try {
        std::unique_ptr<Plan> u(new Plan());
        if (int rc = updates_build(*u, n, ncases, cp, ci, cj, who_)) return rc;
        if (!p && h->batch > 1) return bad_arg(who_, "handles with batch > 1 are not supported");
        if (p && (h->batch > 1 || p->batch > 1)) return bad_arg(who_, "plans and handles with batch > 1 are not supported");
        if (p && !p->schur_idx.empty()) return bad_arg(who_, "not available on a complex plan with a border (cs3_cplx_plan_create_schur)");
        if (p) if (int rc = refuse_schur(h, who_)) return rc;
        h->plans.push_back(u.get());
        u->h = h;
        u->p = p;
        *out = u.release();
    } catch (const std::bad_alloc &) {
        set_error(who + ": out of memory"); return CS3_ERR_ALLOC;
    }
    return CS3_OK;
}

int updates_check(const PlanFlavor &F, cs3_handle h, cs3_updates_s *u, const double *cx, const double *b, const double *X, bool device)
{
    if (F.complex() && !F.p) { set_error(F.name() + ": null complex plan"); return CS3_ERR_ARG; }
    int rc = guard(h); if (rc) return rc;
    if (!u) { set_error(F.name() + ": null plan"); return CS3_ERR_ARG; }
    if (!b || !X || (u->ntrip > 0 && !cx)) { set_error(F.name() + ": null argument"); return CS3_ERR_ARG; }
    if (u->h != h) { set_error(F.name() + ": the plan was made for another handle"); return CS3_ERR_ARG; }
    if (F.complex() && u->p != F.p) { set_error(F.name() + ": the plan was made for another complex plan"); return CS3_ERR_ARG; }
    if (misaligned(F, device, addr(cx) | addr(b) | addr(X))) { set_error(F.name() + ": complex arrays must be aligned to 16 bytes"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(F.name() + ": no successful factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

// Tables of the plan in HBM, the handle's x0 and its tile Z (a real plan's mem.upd.z, a complex plan's mem.sens.t, the
// one cs3_sens_* use; both stable addresses), room for the widest tile in the sweep buffers: everything a call needs, so
// that later calls neither allocate nor synchronise.  A complex plan's arrays have the handle's 2 n rows.
int ensure_updates(const PlanFlavor &F, cs3_handle h, cs3_updates_s *u, DevBuf<double> &Z)
{
    int wmax = 1;
    for (const auto &t : u->tiles) wmax = std::max(wmax, t.t_solve);
    if (!u->on_device) {
        static bool prepared[2] = {false, false};
        if (!prepared[F.cpl - 1]) { CS3_HIP(F.prepare_updates()); prepared[F.cpl - 1] = true; }
        auto &P = u->mem;
        CS3_HIP(P.cases.upload(u->cases));
        CS3_HIP(P.cp.upload(u->cp));
        CS3_HIP(P.tpos.upload(u->tpos));
        CS3_HIP(P.unit.upload(u->unit_row));
        CS3_HIP(P.y.alloc((size_t) u->ncases * F.cpl * UPD_MAX_RANK));
        CS3_HIP(P.flag.alloc((size_t) u->ncases));
        CS3_HIP(P.rpiv.alloc((size_t) u->ncases));
        h->dbg_allocs += 7;
        u->on_device = true;
    }
    const size_t rows = std::max<size_t>(F.cpl, (size_t) h->S.n);
    auto &x0 = h->mem.upd.x0;
    if (!x0.get()) { CS3_HIP(x0.alloc(rows)); h->dbg_allocs += 1; }
    if (int rc = grow_tile(h, Z, rows * (size_t) wmax)) return rc;
    return ensure_rhs_capacity(h, wmax);
}

// x0 = A^-1 b, then per tile: the unit right-hand sides, the handle's solve in place, capacitance and apply.  A complex
// call packs b and the units with the complex plan's rotation.  parts (diagnostics): 1 x0 and the units, 2 the tiles'
// solves, 4 capacitance + apply.
int updates_run(const PlanFlavor &F, cs3_handle h, cs3_updates_s *u, const double *cx_dev, const double *b_dev, double sing_tol,
                double *X_dev, double *rpiv_dev, hipStream_t st, int parts = 7)
{
    int rc = F.p ? cs3_cplx_upload(F.p) : CS3_OK;             // (the tables and s = (1, +0): a plan that never saw a values call)
    if (rc) return rc;
    DevBuf<double> &tile = F.p ? h->mem.sens.t : h->mem.upd.z;
    if ((rc = ensure_updates(F, h, u, tile))) return rc;
    const i64 n = u->n;
    const auto &P = u->mem;
    const UpdTables T{P.cases.get(), P.cp.get(), P.tpos.get(), P.y.get(), P.flag.get()};
    double *rpiv = rpiv_dev ? rpiv_dev : P.rpiv.get();
    double *Z = tile.get(), *x0 = h->mem.upd.x0.get();
    if (n > 0 && (parts & 1)) {
        if (F.p) { if ((rc = cs3_cplx_pack_dev(F.p, CS3_CPLX_N, b_dev, x0, 1, st))) return rc; }
        else CS3_HIP(hipMemcpyAsync(x0, b_dev, (size_t) n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if ((rc = run_solve(h, x0, 1, 0, st))) return rc;
    }
    for (const auto &t : u->tiles) {
        if (n > 0 && t.t > 0) {
            if (parts & 1) CS3_HIP(F.upd_units(Z, n, t.t_solve, P.unit.get() + t.unit0, st));
            if ((parts & 2) && (rc = run_solve(h, Z, t.t_solve, 0, st))) return rc;
        }
        if (parts & 4) {
            CS3_HIP(F.upd_capacitance(T, cx_dev, Z, t.t_solve, x0, t.c0, t.nc, sing_tol, rpiv, st));
            CS3_HIP(F.upd_apply(T, Z, t.t_solve, x0, n, t.c0, t.nc, t.rmax, u->ncases, X_dev, st));
        }
    }
    return CS3_OK;
}

// The device forms: cs3_*updates_solve_dev, and with a mask the diagnostic one
int updates_solve_dev(const PlanFlavor &F, cs3_handle h, cs3_updates_s *u, const double *cx_dev, const double *b_dev, double sing_tol,
                      double *X_dev, double *rpiv_dev, void *stream, int64_t parts = 7)
{
    int rc = updates_check(F, h, u, cx_dev, b_dev, X_dev, true);
    if (rc) return rc;
    if (parts < 1 || parts > 7) return bad_arg(F.who, "parts must be a mask of 1, 2 and 4");
    return updates_run(F, h, u, cx_dev, b_dev, sing_tol, X_dev, rpiv_dev, (hipStream_t) stream, (int) parts);
}

// The host form: the values on the plan, b [n] and X [n, ncases] in one block of this call
int updates_solve_host(const PlanFlavor &F, cs3_handle h, cs3_updates_s *u, const double *cx, const double *b, double sing_tol, double *X,
                       double *rpiv)
{
    int rc = updates_check(F, h, u, cx, b, X, false);
    if (rc) return rc;
    const size_t n = (size_t) F.cpl * (size_t) u->n, nc = (size_t) u->ncases, nt = (size_t) F.cpl * (size_t) u->ntrip;
    CS3_HIP(u->mem.cx.reserve(nt));
    DevBuf<double> bx;
    CS3_HIP(bx.alloc(n * (nc + 1)));
    double *d_b = bx.get(), *d_x = d_b + n;
    if (nt) CS3_HIP(hipMemcpy(u->mem.cx.get(), cx, nt * sizeof(double), hipMemcpyHostToDevice));
    if (n) CS3_HIP(hipMemcpy(d_b, b, n * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = updates_run(F, h, u, u->mem.cx.get(), d_b, sing_tol, d_x, nullptr, nullptr))) return rc;
    if (n) CS3_HIP(hipMemcpy(X, d_x, n * nc * sizeof(double), hipMemcpyDeviceToHost));
    if (rpiv) CS3_HIP(hipMemcpy(rpiv, u->mem.rpiv.get(), nc * sizeof(double), hipMemcpyDeviceToHost));
    CS3_HIP(hipDeviceSynchronize());
    return CS3_OK;
}

// ---- sparse right-hand sides: Y = C op(A)^-1 B on the held factors (sens.hip, cplxsens.hip) ------------------------------
// What cs3_sens_plan and cs3_cplx_sens_plan refuse whatever the operands are, in this order.  The real call comes here
// last, the complex one first.
int sens_refuse_handle(const char *who, cs3_handle h)
{
    if (h->batch > 1) return bad_arg(who, "handles with batch > 1 are not supported");
    return refuse_schur(h, who);
}

// One operand's pattern: pointers monotone from 0 (check 5); the indices are looked at afterwards (check 6), so that a
// bad pointer array of either operand wins over a bad index of either.
int sens_check_pointers(const char *who, const char *name, int64_t ncols, const int32_t *P, const int32_t *I)
{
    if (P[0] != 0) { set_error(std::string(who) + ": " + name + "[0] != 0"); return CS3_ERR_ARG; }
    for (int64_t c = 0; c < ncols; ++c)
        if (P[c + 1] < P[c]) { set_error(std::string(who) + ": " + name + " not monotone at column " + std::to_string(c)); return CS3_ERR_ARG; }
    if (P[ncols] > 0 && !I) { set_error(std::string(who) + ": null index array behind " + name); return CS3_ERR_ARG; }
    return CS3_OK;
}

int sens_check_indices(const char *who, const char *name, int64_t n, int64_t ncols, const int32_t *P, const int32_t *I)
{
    for (int64_t c = 0; c < ncols; ++c)
        for (int e = P[c]; e < P[c + 1]; ++e)
            if (I[e] < 0 || I[e] >= n) {
                set_error(std::string(who) + ": index out of range in column " + std::to_string(c) + " of " + name);
                return CS3_ERR_ARG;
            }
    return CS3_OK;
}

// What both plan calls do once their leading checks have passed: the checks of cs3_sens_plan from "k < 1" on (n: the
// order the indices live in), then the handle (the complex call has looked at it already, so that for it op is last), the
// side, the tiles, and the plan joins its handle.
template <class Plan>
int sens_plan_build(const char *who, cs3_handle h, int64_t n, int64_t k, const int32_t *Bp, const int32_t *Bi, int64_t p, const int32_t *Ctp,
                    const int32_t *Cti, int64_t side, int64_t op, Plan **out)
{
    int rc;
    if (k < 1 || p < 1 || k > INT_MAX / 2 || p > INT_MAX / 2) return bad_arg(who, "k and p must be >= 1");
    if (!Bp && !Ctp) return bad_arg(who, "B and C are both the identity (the dense inverse is not offered)");
    if (!Bp && k != n) return bad_arg(who, "B is the identity but k != n");
    if (!Ctp && p != n) return bad_arg(who, "C is the identity but p != n");
    if (Bp && (rc = sens_check_pointers(who, "Bp", k, Bp, Bi))) return rc;
    if (Ctp && (rc = sens_check_pointers(who, "Ctp", p, Ctp, Cti))) return rc;
    if (Bp && (rc = sens_check_indices(who, "B", n, k, Bp, Bi))) return rc;
    if (Ctp && (rc = sens_check_indices(who, "C'", n, p, Ctp, Cti))) return rc;
    if (side < 0 || side > 2) return bad_arg(who, "side must be 0 (auto), 1 (right) or 2 (left)");
    if (!Bp && side == 1) return bad_arg(who, "B is the identity, side right would solve for all n columns: use side 0 or 2");
    if (!Ctp && side == 2) return bad_arg(who, "C is the identity, side left would solve for all n rows: use side 0 or 1");
    if ((rc = sens_refuse_handle(who, h))) return rc;
    if (op != CS3_CPLX_N && op != CS3_CPLX_T && op != CS3_CPLX_H) return bad_arg(who, "op must be 0 (N), 1 (T) or 2 (H)");
    try {
        std::unique_ptr<Plan> u(new Plan());
        u->n = n; u->k = k; u->p = p;
        u->op = (int) op;
        u->b_ident = !Bp; u->c_ident = !Ctp;
        u->side = !Bp ? 2 : !Ctp ? 1 : side ? (int) side : (p < k ? 2 : 1);
        if (Bp) { u->bp.assign(Bp, Bp + k + 1); u->bi.assign(Bi, Bi + Bp[k]); }
        if (Ctp) { u->ctp.assign(Ctp, Ctp + p + 1); u->cti.assign(Cti, Cti + Ctp[p]); }
        long long cap = SENS_MAX_TILE;
        if (const char *e = std::getenv("CS3_SENS_TILE")) cap = std::min<long long>(SENS_MAX_TILE, std::max<long long>(1, std::atoll(e)));
        u->tile_cap = (int) cap;
        // full tiles at the tile width; the last at its own, padded to SENS_PAD_WIDTH where the tile width allows it.  (A
        // complex solved-for column is ONE real column of the [2n, w] tile.)
        const i64 ns = (u->side == 1) ? k : p;
        for (i64 c0 = 0; c0 < ns; c0 += cap) {
            const int t = (int) std::min<i64>(cap, ns - c0);
            const int w = (t < SENS_PAD_WIDTH && cap >= SENS_PAD_WIDTH) ? SENS_PAD_WIDTH : t;
            u->tiles.push_back(cs3_sens_s::Tile{c0, t, w});
            u->wmax = std::max(u->wmax, w);
        }
        h->plans.push_back(u.get());
        u->h = h;
        *out = u.release();
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of memory"); return CS3_ERR_ALLOC;
    }
    return CS3_OK;
}

// (.trans of a real plan is 0 or 1, of a complex plan its op: the same field)
int sens_info(const char *who, const cs3_sens_s *u, cs3_sens_info_t *out)
{
    if (!u || !out) return bad_arg(who, "null argument");
    *out = cs3_sens_info_t{u->k, u->p, u->side, u->op, (int64_t) u->tiles.size(), u->wmax, u->nnz_b(), u->nnz_c()};
    return CS3_OK;
}

int sens_check(const PlanFlavor &F, cs3_handle h, cs3_sens_s *u, const double *bx, const double *ctx, const double *Y, bool device)
{
    if (F.complex() && !F.p) { set_error(F.name() + ": null complex plan"); return CS3_ERR_ARG; }
    int rc = guard(h); if (rc) return rc;
    if (!u) { set_error(F.name() + ": null plan"); return CS3_ERR_ARG; }
    if (!Y || (!u->b_ident && u->nnz_b() > 0 && !bx) || (!u->c_ident && u->nnz_c() > 0 && !ctx)) {
        set_error(F.name() + ": null argument");
        return CS3_ERR_ARG;
    }
    if (u->h != h) { set_error(F.name() + ": the plan was made for another handle"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(F.name() + ": no successful factorisation"); return CS3_ERR_STATE; }
    if (F.complex() && F.p->n != u->n) { set_error(F.name() + ": the complex plan has another order than the one the plan was made with"); return CS3_ERR_ARG; }
    if (misaligned(F, device, (u->b_ident ? 0 : addr(bx)) | (u->c_ident ? 0 : addr(ctx)) | addr(Y))) {
        set_error(F.name() + ": complex arrays must be aligned to 16 bytes");
        return CS3_ERR_ARG;
    }
    return CS3_OK;
}

// Tables of the plan in HBM, the handle's tile buffer, room for the widest tile in the sweep buffers: everything a call
// needs, so that later calls neither allocate nor synchronise.
int ensure_sens(cs3_handle h, cs3_sens_s *u)
{
    if (!u->on_device) {
        auto &P = u->mem;
        if (!u->b_ident) { CS3_HIP(P.bp.upload(u->bp)); CS3_HIP(P.bi.upload(u->bi)); h->dbg_allocs += 2; }
        if (!u->c_ident) { CS3_HIP(P.ctp.upload(u->ctp)); CS3_HIP(P.cti.upload(u->cti)); h->dbg_allocs += 2; }
        u->on_device = true;
    }
    if (int rc = grow_tile(h, h->mem.sens.t, std::max<size_t>(1, (size_t) h->S.n) * (size_t) u->wmax)) return rc;
    return ensure_rhs_capacity(h, u->wmax);
}

// Per tile: scatter the solved-for columns, solve in place, combine with the other operand.  Side left solves with the
// transpose: inner T for op N, inner N for op T, and for op H inner N between two conjugations (A^-H = conj(A^-T)).  A
// complex call's scatter packs and its combine unpacks, the handle solves the real tile in between (plain for inner N,
// transposed for T and H).  parts (diagnostics): 1 the scatter, 2 the solve, 4 the combine.
int sens_run(const PlanFlavor &F, cs3_handle h, cs3_sens_s *u, const double *bx_dev, const double *ctx_dev, double *Y_dev, hipStream_t st,
             int parts = 7)
{
    int rc = F.p ? cs3_cplx_upload(F.p) : CS3_OK;             // (the tables and s = (1, +0): a plan that never saw a values call)
    if (rc) return rc;
    if ((rc = ensure_sens(h, u))) return rc;
    const auto &P = u->mem;
    const SensOperand B{u->b_ident ? nullptr : P.bp.get(), P.bi.get(), bx_dev};
    const SensOperand Ct{u->c_ident ? nullptr : P.ctp.get(), P.cti.get(), ctx_dev};
    const bool right = u->side == 1;
    const SensOperand &solved = right ? B : Ct, &other = right ? Ct : B;
    const i64 ng = right ? u->p : u->k;
    const int inner = right ? u->op : (u->op == CS3_CPLX_N ? CS3_CPLX_T : CS3_CPLX_N);
    const CsensGlue glue{inner, (!right && u->op == CS3_CPLX_H) ? 1 : 0, F.s()};
    double *T = h->mem.sens.t.get();
    for (const auto &t : u->tiles) {
        if (parts & 1) CS3_HIP(F.sens_scatter(T, u->n, t.w, solved, t.c0, t.t, glue, st));
        if ((parts & 2) && (rc = run_solve(h, T, t.w, 0, st, inner != CS3_CPLX_N))) return rc;
        if (parts & 4) CS3_HIP(F.sens_combine(T, t.w, t.t, other, ng, t.c0, u->k, !right, glue, Y_dev, st));
    }
    return CS3_OK;
}

// The device forms: cs3_*sens_solve_dev, and with a mask the diagnostic ones
int sens_solve_dev(const PlanFlavor &F, cs3_handle h, cs3_sens_s *u, const double *bx_dev, const double *ctx_dev, double *Y_dev, void *stream,
                   int64_t parts = 7)
{
    int rc = sens_check(F, h, u, bx_dev, ctx_dev, Y_dev, true);
    if (rc) return rc;
    if (parts < 1 || parts > 7) return bad_arg(F.who, "parts must be a mask of 1, 2 and 4");
    return sens_run(F, h, u, bx_dev, ctx_dev, Y_dev, (hipStream_t) stream, (int) parts);
}

// The host form: its device copies of the values and of Y stay on the plan
int sens_solve_host(const PlanFlavor &F, cs3_handle h, cs3_sens_s *u, const double *Bx, const double *Ctx, double *Y)
{
    int rc = sens_check(F, h, u, Bx, Ctx, Y, false);
    if (rc) return rc;
    const size_t nb = u->b_ident ? 0 : F.cpl * (size_t) u->nnz_b(), nc = u->c_ident ? 0 : F.cpl * (size_t) u->nnz_c();
    const size_t ny = F.cpl * (size_t) u->p * (size_t) u->k;
    auto &P = u->mem;
    CS3_HIP(P.bx.reserve(nb)); CS3_HIP(P.ctx.reserve(nc)); CS3_HIP(P.y.reserve(ny));
    if (nb) CS3_HIP(hipMemcpy(P.bx.get(), Bx, nb * sizeof(double), hipMemcpyHostToDevice));
    if (nc) CS3_HIP(hipMemcpy(P.ctx.get(), Ctx, nc * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = sens_run(F, h, u, P.bx.get(), P.ctx.get(), P.y.get(), nullptr))) return rc;
    CS3_HIP(hipMemcpy(Y, P.y.get(), ny * sizeof(double), hipMemcpyDeviceToHost));
    CS3_HIP(hipDeviceSynchronize());
    return CS3_OK;
}

// ---- selected inversion: A^-1 on the pattern of L + U (selinv.hip, selinv.cpp) ------------------------------------------
// What every cs3_selinv_* call refuses, and why (no device needed)
int selinv_refuse(cs3_handle h, const char *who)
{
    if (int rc = refuse_schur(h, who)) return rc;
    if (h->match.on) {
        set_error(std::string(who) + ": not available for a matched handle (the row permutation makes the pattern of the factors unsymmetric)");
        return CS3_ERR_ARG;
    }
    if (h->S.il_len > 0) {
        set_error(std::string(who) + ": not available for a matrix-interleaved batch (128 or more matrices)");
        return CS3_ERR_ARG;
    }
    return CS3_OK;
}

// The plan and the maps of the entries of A and of the diagonal, from the analysis alone
int ensure_selinv_plan(cs3_handle h)
{
    auto &Q = h->selinv;
    if (Q.planned) return CS3_OK;
    const Symbolic &S = h->S;
    try {
        build_selinv_plan(S, Q.plan);
        Q.entry.resize((size_t) S.nnzA); Q.entry_t.resize((size_t) S.nnzA); Q.diag.resize((size_t) S.n);
        for (i64 j = 0; j < S.n; ++j) {
            Q.diag[j] = selinv_position(S, Q.plan, S.pinv[j], S.pinv[j]);
            for (i64 p = h->Ap_host[j]; p < h->Ap_host[j + 1]; ++p) {
                const i64 k = S.pinv[h->Ai_host[p]], l = S.pinv[j];
                Q.entry[p] = selinv_position(S, Q.plan, k, l);
                Q.entry_t[p] = selinv_position(S, Q.plan, l, k);
                if (Q.entry[p] < 0 || Q.entry_t[p] < 0) { set_error("cs3_selinv: an entry of A lies outside the symbolic structure"); return CS3_ERR_STATE; }
            }
        }
    } catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    Q.planned = true;
    return CS3_OK;
}

int ensure_selinv(cs3_handle h)
{
    int rc = ensure_selinv_plan(h);
    if (rc) return rc;
    auto &M = h->mem.selinv;
    if (M.fronts.get()) return CS3_OK;
    const auto &Q = h->selinv;
    CS3_HIP(prepare_selinv_kernels());
    CS3_HIP(M.z.alloc((size_t) (h->batch * Q.plan.zpool_doubles)));
    CS3_HIP(M.work.alloc((size_t) (h->batch * Q.plan.work_doubles)));
    CS3_HIP(M.entry.upload(Q.entry));
    CS3_HIP(M.entry_t.upload(Q.entry_t));
    CS3_HIP(M.diag.upload(Q.diag));
    CS3_HIP(M.fronts.upload(Q.plan.fronts));
    return CS3_OK;
}

// checks 1 to 3 of the header, in its order
int selinv_check(cs3_handle h, const char *who, bool null_output)
{
    int rc = guard(h); if (rc) return rc;
    if (null_output) { set_error(std::string(who) + ": null output"); return CS3_ERR_ARG; }
    if ((rc = selinv_refuse(h, who))) return rc;
    if (!h->factored) { set_error(std::string(who) + ": called before a successful factorisation"); return CS3_ERR_STATE; }
    return CS3_OK;
}

// out_dev [batch][count] through `map`, from the Z that cs3_selinv_dev left (check 4 of the header)
int selinv_get_dev(cs3_handle h, const char *who, const DevBuf<i64> &map, int64_t count, double *out_dev, hipStream_t st)
{
    if (!h->selinv_valid) { set_error(std::string(who) + ": no selected inverse of the current factors (call cs3_selinv_dev after the factorisation)"); return CS3_ERR_STATE; }
    CS3_HIP(launch_selinv_gather(h->mem.selinv.z.get(), h->selinv.plan.zpool_doubles, (const long long *) map.get(), out_dev, count, h->batch, st));
    return CS3_OK;
}

// The host forms: Z is computed when the handle does not hold that of the current factors, then read through `map`
int selinv_get_host(cs3_handle h, const DevBuf<i64> &map, int64_t count, long long nmat, const double *z, double *out)
{
    auto &M = h->mem.selinv;
    CS3_HIP(M.out.reserve((size_t) (nmat * count)));
    CS3_HIP(launch_selinv_gather(z, h->selinv.plan.zpool_doubles, (const long long *) map.get(), M.out.get(), count, nmat, nullptr));
    CS3_HIP(hipMemcpy(out, M.out.get(), (size_t) (nmat * count) * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- complex selected inversion: Z = A^-1 out of the real form's selected inverse (cplxselinv.hip) ---------------------
// checks 1 to 6 of the header, in its order; none needs a device
int cselinv_check(const char *who_, cs3_cplx p, cs3_handle h, const double *out, bool device, bool plan_only = false)
{
    const std::string who(who_);
    if (!p) { set_error(who + ": null complex plan"); return CS3_ERR_ARG; }
    int rc = guard(h); if (rc) return rc;
    if (!out && !plan_only) { set_error(who + ": null output"); return CS3_ERR_ARG; }
    if (h->S.n != 2 * p->n || h->S.nnzA != 4 * p->nnz || h->batch != p->batch) {
        set_error(who + ": the handle is not one on the real form of the complex plan (its order is not 2 n, its entries are not 4 nnz, "
                        "or the batches differ)");
        return CS3_ERR_ARG;
    }
    if ((rc = selinv_refuse(h, who_))) return rc;
    if (plan_only) return CS3_OK;                          // (cs3_debug_cplx_selinv_maps: the analysis alone)
    if (device && (reinterpret_cast<uintptr_t>(out) & 15)) { set_error(who + ": complex arrays must be aligned to 16 bytes"); return CS3_ERR_ARG; }
    if (!h->factored) { set_error(who + ": called before a successful factorisation"); return CS3_ERR_STATE; }
    if (device && !h->selinv_valid) {
        set_error(who + ": no selected inverse of the current factors (call cs3_selinv_dev after the factorisation)");
        return CS3_ERR_STATE;
    }
    return CS3_OK;
}

// The maps of the complex layer, once per handle and from the analysis alone (no device): the real maps of
// ensure_selinv_plan at the positions Rp[2j] + 2t, + 1 and Rp[2j + 1] + 2t of the real pattern, in pairs, and the one
// position they do not hold, (2i + 1, 2i).  The handle's pattern is compared with the real form of the plan's while they are
// built, so that the kernels read the handle's tables only.
int ensure_cselinv_plan(cs3_cplx p, cs3_handle h, const char *who_)
{
    auto &Q = h->selinv;
    if (Q.cplanned) return CS3_OK;
    const std::string who(who_);
    int rc = ensure_selinv_plan(h);
    if (rc) return rc;
    const Symbolic &S = h->S;
    const i64 n = p->n, nnz = p->nnz;
    const i32 *Ap = p->Ap.data(), *Ai = p->Ai.data(), *Rp = h->Ap_host.data(), *Ri = h->Ai_host.data();
    try {
        Q.centry.assign((size_t) (2 * nnz), -1); Q.centry_t.assign((size_t) (2 * nnz), -1); Q.cdiag.assign((size_t) (2 * n), -1);
        Q.cij.assign((size_t) (2 * nnz), 0);
        for (i64 j = 0; j < n; ++j) {
            const i64 r0 = 4LL * Ap[j], r1 = 2LL * Ap[j] + 2LL * Ap[j + 1];
            bool same = Rp[2 * j] == r0 && Rp[2 * j + 1] == r1;
            for (i64 e = Ap[j]; same && e < Ap[j + 1]; ++e) {
                const i64 lo = r0 + 2 * (e - Ap[j]), hi = r1 + 2 * (e - Ap[j]);
                const i32 i = Ai[e];
                same = Ri[lo] == 2 * i && Ri[lo + 1] == 2 * i + 1 && Ri[hi] == 2 * i && Ri[hi + 1] == 2 * i + 1;
                Q.centry[2 * e] = Q.entry[lo];     Q.centry[2 * e + 1] = Q.entry[lo + 1];       // ZR(2i, 2j), ZR(2i + 1, 2j)
                Q.centry_t[2 * e] = Q.entry_t[lo]; Q.centry_t[2 * e + 1] = Q.entry_t[hi];       // ZR(2j, 2i), ZR(2j + 1, 2i)
                Q.cij[2 * e] = i; Q.cij[2 * e + 1] = (i32) j;
            }
            if (!same) {
                set_error(who + ": the handle's pattern is not the real form of the complex plan's (cs3_cplx_plan_pattern), column " +
                          std::to_string(j));
                return CS3_ERR_ARG;
            }
            Q.cdiag[2 * j] = Q.diag[2 * j];
            Q.cdiag[2 * j + 1] = selinv_position(S, Q.plan, S.pinv[2 * j + 1], S.pinv[2 * j]);
            if (Q.cdiag[2 * j] < 0 || Q.cdiag[2 * j + 1] < 0) {
                set_error(who + ": the imaginary part of Z(" + std::to_string(j) + ", " + std::to_string(j) + ") lies outside the symbolic "
                          "structure (complex row " + std::to_string(j) + " has no stored diagonal)");
                return CS3_ERR_STATE;
            }
        }
    } catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
    Q.cplanned = true;
    return CS3_OK;
}

int ensure_cselinv(cs3_cplx p, cs3_handle h, const char *who)
{
    auto &M = h->mem.cselinv;
    if (M.ij.get()) return CS3_OK;
    int rc = ensure_cselinv_plan(p, h, who);
    if (rc) return rc;
    const auto &Q = h->selinv;
    CS3_HIP(M.entry.upload(Q.centry));
    CS3_HIP(M.entry_t.upload(Q.centry_t));
    CS3_HIP(M.diag.upload(Q.cdiag));
    CS3_HIP(M.ij.upload(Q.cij));                           // (last: what marks the maps as uploaded)
    return CS3_OK;
}

enum CselinvWhat : int { CSELINV_ENTRIES = 0, CSELINV_ENTRIES_T = 1, CSELINV_DIAG = 2, CSELINV_THEVENIN = 3 };

int cselinv_run(cs3_cplx p, cs3_handle h, const char *who, int what, double *out_dev, hipStream_t st)
{
    int rc = cs3_cplx_upload(p);                            // (the tables and s = (1, +0): a plan that never saw a values call)
    if (rc) return rc;
    if ((rc = ensure_cselinv(p, h, who))) return rc;
    const auto &M = h->mem.cselinv;
    const CselinvMaps maps{(const long long *) M.entry.get(), (const long long *) M.entry_t.get(), (const long long *) M.diag.get(),
                           M.ij.get()};
    const double *z = h->mem.selinv.z.get(), *s = p->d_s.get();
    const long long zs = h->selinv.plan.zpool_doubles;
    if (what == CSELINV_DIAG) CS3_HIP(launch_cselinv_diag(z, zs, maps, s, p->n, p->batch, out_dev, st));
    else if (what == CSELINV_THEVENIN) CS3_HIP(launch_cselinv_thevenin(z, zs, maps, s, p->n, p->nnz, p->batch, out_dev, st));
    else CS3_HIP(launch_cselinv_entries(z, zs, maps, what == CSELINV_ENTRIES_T, s, p->n, p->nnz, p->batch, out_dev, st));
    return CS3_OK;
}

int cselinv_dev(cs3_cplx p, cs3_handle h, const char *who, int what, double *out_dev, void *stream)
{
    int rc = cselinv_check(who, p, h, out_dev, true);
    if (rc) return rc;
    return cselinv_run(p, h, who, what, out_dev, (hipStream_t) stream);
}

// The host forms: ZR is computed when the handle does not hold that of the current factors; the result is staged through
// the block the real host getters use.
int cselinv_host(cs3_cplx p, cs3_handle h, const char *who, int what, double *out)
{
    int rc = cselinv_check(who, p, h, out, false);
    if (rc) return rc;
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    const size_t count = 2 * (size_t) p->batch * (size_t) (what == CSELINV_DIAG ? p->n : p->nnz);
    auto &stage = h->mem.selinv.out;
    CS3_HIP(stage.reserve(count));
    if ((rc = cselinv_run(p, h, who, what, stage.get(), nullptr))) return rc;
    CS3_HIP(hipMemcpy(out, stage.get(), count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- bilinear forms on the selected inverse: t_i = c_i' A^-1 b_i (quadform.hip) -------------------------------------------
// The term map (per row, a-major, the zpool offset of Z(pinv Cti[a], pinv Bti[b])), the class of every row by its term
// count, and the rows in class order.  The pattern has passed the pointer and index checks.
int quad_build(cs3_handle h, cs3_quad_s &u, int64_t m, const int32_t *Ctp, const int32_t *Cti, const int32_t *Btp, const int32_t *Bti,
               const char *who)
{
    const Symbolic &S = h->S;
    const SelinvPlan &P = h->selinv.plan;
    u.m = m; u.same = !Btp;
    if (!Btp) { Btp = Ctp; Bti = Cti; }
    u.nnz_c = Ctp[m]; u.nnz_b = Btp[m];
    u.term_ptr.assign((size_t) m + 1, 0);
    for (i64 i = 0; i < m; ++i) {
        u.term_ptr[i + 1] = u.term_ptr[i] + (i64) (Ctp[i + 1] - Ctp[i]) * (i64) (Btp[i + 1] - Btp[i]);
        if (u.term_ptr[i + 1] >= (i64) INT_MAX - 1023) return bad_arg(who, "2^31 - 1024 terms or more (a row has nnz(c) * nnz(b))");
    }
    u.term_pos.resize((size_t) u.term_ptr[m]);
    u.row_class.resize((size_t) m);
    std::vector<i32> order[3];
    for (i64 i = 0; i < m; ++i) {
        i64 at = u.term_ptr[i];
        for (i32 a = Ctp[i]; a < Ctp[i + 1]; ++a)
            for (i32 b = Btp[i]; b < Btp[i + 1]; ++b) {
                const i64 pos = selinv_position(S, P, S.pinv[Cti[a]], S.pinv[Bti[b]]);
                if (pos < 0) {
                    set_error(std::string(who) + ": row " + std::to_string(i) + " pairs columns " + std::to_string(Cti[a]) + " and " +
                              std::to_string(Bti[b]) + ", an entry of A^-1 outside the pattern of L + U");
                    return CS3_ERR_ARG;
                }
                u.term_pos[(size_t) at++] = pos;
            }
        const i64 nt = u.term_ptr[i + 1] - u.term_ptr[i];
        u.row_class[i] = nt <= QUAD_LANE_TERMS ? 0 : nt <= QUAD_WAVE_TERMS ? 1 : 2;
        order[u.row_class[i]].push_back((i32) i);
    }
    // lanes of one wave run as long as their longest row: the lane rows go by ascending term count
    std::stable_sort(order[0].begin(), order[0].end(),
                     [&](i32 x, i32 y) { return u.term_ptr[x + 1] - u.term_ptr[x] < u.term_ptr[y + 1] - u.term_ptr[y]; });
    u.rows.reserve((size_t) m);
    for (const auto &cls : order)
        for (i32 i : cls)
            u.rows.push_back(QuadRow{u.term_ptr[i], Ctp[i], Ctp[i + 1] - Ctp[i], Btp[i], Btp[i + 1] - Btp[i], i, 0});
    QuadShape &G = u.shape;
    G.n_lane = (i64) order[0].size(); G.n_wave = (i64) order[1].size(); G.n_wg = (i64) order[2].size();
    G.blk_wave = (unsigned) ((G.n_lane + QUAD_BLOCK - 1) / QUAD_BLOCK);
    G.blk_wg = G.blk_wave + (unsigned) ((G.n_wave + 3) / 4);
    G.blocks = G.blk_wg + (unsigned) G.n_wg;
    return CS3_OK;
}

// the checks of cs3_quad_dev in the header's order; `device`: the caller's forms need Z of the current factors
int quad_check(const char *who, cs3_handle h, cs3_quad_s *u, bool null_argument, bool device)
{
    int rc = guard(h); if (rc) return rc;
    if (!u || null_argument) return bad_arg(who, "null argument");
    if (u->h != h) return bad_arg(who, "the plan was made for another handle");
    if (!h->factored) { set_error(std::string(who) + ": no successful factorisation"); return CS3_ERR_STATE; }
    if (device && !h->selinv_valid) {
        set_error(std::string(who) + ": no selected inverse of the current factors (call cs3_selinv_dev after the factorisation)");
        return CS3_ERR_STATE;
    }
    return CS3_OK;
}

// Tables of the plan in HBM, t for the calls that want none, the partials of the residual reduction: everything a call
// needs, so that later calls neither allocate nor synchronise.
int ensure_quad(cs3_handle h, cs3_quad_s *u)
{
    if (u->on_device) return CS3_OK;
    auto &M = u->mem;
    CS3_HIP(M.rows.upload(u->rows));
    CS3_HIP(M.pos.upload(u->term_pos));
    CS3_HIP(M.t.alloc((size_t) (h->batch * u->m)));
    CS3_HIP(M.parts.alloc((size_t) (4 * h->batch * ((u->m + QUAD_BLOCK - 1) / QUAD_BLOCK))));
    h->dbg_allocs += 4;
    u->on_device = true;
    return CS3_OK;
}

int quad_run(cs3_handle h, cs3_quad_s *u, const double *cx_dev, const double *bx_dev, double *t_dev, hipStream_t st)
{
    if (int rc = ensure_quad(h, u)) return rc;
    if (u->same) bx_dev = cx_dev;
    CS3_HIP(launch_quad_forms(h->mem.selinv.z.get(), h->selinv.plan.zpool_doubles, u->mem.rows.get(), (const long long *) u->mem.pos.get(),
                              u->shape, cx_dev, u->nnz_c, bx_dev, u->nnz_b, u->m, h->batch, t_dev, st));
    return CS3_OK;
}

int quad_normres_run(cs3_handle h, cs3_quad_s *u, const double *hx_dev, const double *w_dev, const double *r_dev, double crit_tol,
                     double *t_dev, double *omega_dev, double *rn_dev, double *summary_dev, hipStream_t st)
{
    if (int rc = ensure_quad(h, u)) return rc;
    if (!t_dev) t_dev = u->mem.t.get();
    if (int rc = quad_run(h, u, hx_dev, hx_dev, t_dev, st)) return rc;
    CS3_HIP(launch_quad_normres(t_dev, w_dev, r_dev, crit_tol, u->m, h->batch, omega_dev, rn_dev, u->mem.parts.get(), summary_dev, st));
    return CS3_OK;
}

// host array -> a block of the plan (grow-only)
int quad_stage(DevBuf<double> &buf, const double *src, size_t count)
{
    CS3_HIP(buf.reserve(count));
    if (count) CS3_HIP(hipMemcpy(buf.get(), src, count * sizeof(double), hipMemcpyHostToDevice));
    return CS3_OK;
}

}  // namespace

extern "C" {

// ---- low-rank-modified systems --------------------------------------------------------------------------------------------
int cs3_updates_plan(cs3_handle h, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj, cs3_updates *out)
{
    const char *who = "cs3_updates_plan";
    int rc = guard(h); if (rc) return rc;
    if (!out) return bad_arg(who, "null output");
    *out = nullptr;
    if ((rc = refuse_schur(h, who))) return rc;
    if (!cp) return bad_arg(who, "null case pointers");
    return updates_plan_make(who, nullptr, h, h->S.n, ncases, cp, ci, cj, out);
}

int cs3_cplx_updates_plan(cs3_cplx p, cs3_handle h, int64_t ncases, const int32_t *cp, const int32_t *ci, const int32_t *cj,
                          cs3_cplx_updates *out)
{
    const char *who = "cs3_cplx_updates_plan";
    if (!p || !h) return bad_arg(who, "null plan or handle");
    if (!out) return bad_arg(who, "null output");
    *out = nullptr;
    if (!cp) return bad_arg(who, "null case pointers");
    if (h->S.n != 2 * p->n) return bad_arg(who, "the handle's order is not 2 n of the complex plan");
    return updates_plan_make(who, p, h, p->n, ncases, cp, ci, cj, out);
}

int cs3_updates_free(cs3_updates u) { return plan_free(u); }
int cs3_cplx_updates_free(cs3_cplx_updates u) { return plan_free(u); }

int cs3_updates_info(cs3_updates u, int64_t *ncases, int64_t *nrows_unique, int64_t *max_rank, int64_t *ntiles)
{
    if (!u) { set_error("cs3_updates_info: null plan"); return CS3_ERR_ARG; }
    if (ncases) *ncases = u->ncases;
    if (nrows_unique) *nrows_unique = u->nrows_unique;
    if (max_rank) *max_rank = u->max_rank;
    if (ntiles) *ntiles = (int64_t) u->tiles.size();
    return CS3_OK;
}

int cs3_cplx_updates_info(cs3_cplx_updates u, int64_t *ncases, int64_t *nrows_unique, int64_t *max_rank, int64_t *ntiles)
{
    if (!u) { set_error("cs3_cplx_updates_info: null plan"); return CS3_ERR_ARG; }
    return cs3_updates_info(u, ncases, nrows_unique, max_rank, ntiles);
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

int64_t cs3_debug_cplx_updates_tiles(cs3_cplx_updates u, int32_t *first_case, int32_t *ncases, int32_t *nrows, int32_t *width)
{
    if (!u) { set_error("cs3_debug_cplx_updates_tiles: null plan"); return CS3_ERR_ARG; }
    return cs3_debug_updates_tiles(u, first_case, ncases, nrows, width);
}

int cs3_cplx_updates_limits(cs3_cplx_updates_limits_t *out)
{
    if (!out) { set_error("cs3_cplx_updates_limits: null output"); return CS3_ERR_ARG; }
    *out = cs3_cplx_updates_limits_t{CUPD_UNIT_ROWS, CUPD_UNIT_THREADS, CUPD_APPLY_STAGE, CUPD_APPLY_ROWS, CUPD_APPLY_NT_MIN,
                                     UPD_MAX_RANK, UPD_MAX_TILE, UPD_MAX_TILE_CASES};
    return CS3_OK;
}

int cs3_updates_solve_dev(cs3_handle h, cs3_updates u, const double *cx_dev, const double *b_dev, double sing_tol, double *X_dev,
                          double *rpiv_dev, void *stream)
{
    return updates_solve_dev(real_flavor("cs3_updates_solve_dev"), h, u, cx_dev, b_dev, sing_tol, X_dev, rpiv_dev, stream);
}

int cs3_cplx_updates_solve_dev(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, const double *cz_dev, const double *b_dev, double sing_tol,
                               double *X_dev, double *rpiv_dev, void *stream)
{
    return updates_solve_dev(cplx_flavor(p, "cs3_cplx_updates_solve_dev"), h, u, cz_dev, b_dev, sing_tol, X_dev, rpiv_dev, stream);
}

int cs3_debug_cplx_updates_parts(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, int64_t parts, const double *cz_dev, const double *b_dev,
                                 double sing_tol, double *X_dev, double *rpiv_dev, void *stream)
{
    return updates_solve_dev(cplx_flavor(p, "cs3_debug_cplx_updates_parts"), h, u, cz_dev, b_dev, sing_tol, X_dev, rpiv_dev, stream, parts);
}

int cs3_updates_solve(cs3_handle h, cs3_updates u, const double *cx, const double *b, double sing_tol, double *X, double *rpiv)
{
    return updates_solve_host(real_flavor("cs3_updates_solve"), h, u, cx, b, sing_tol, X, rpiv);
}

int cs3_cplx_updates_solve(cs3_cplx p, cs3_handle h, cs3_cplx_updates u, const double *cz, const double *b, double sing_tol, double *X,
                           double *rpiv)
{
    return updates_solve_host(cplx_flavor(p, "cs3_cplx_updates_solve"), h, u, cz, b, sing_tol, X, rpiv);
}

// ---- sparse right-hand sides ------------------------------------------------------------------------------------------------
int cs3_sens_limits(cs3_sens_limits_t *out)
{
    if (!out) { set_error("cs3_sens_limits: null output"); return CS3_ERR_ARG; }
    *out = cs3_sens_limits_t{SENS_MAX_TILE, SENS_PAD_WIDTH, SENS_SCATTER_ROWS, SENS_SCATTER_THREADS, SENS_COMBINE_COLS,
                             SENS_COMBINE_LANES, SENS_TBLOCK};
    return CS3_OK;
}

int cs3_cplx_sens_limits(cs3_sens_limits_t *out)
{
    if (!out) { set_error("cs3_cplx_sens_limits: null output"); return CS3_ERR_ARG; }
    *out = cs3_sens_limits_t{SENS_MAX_TILE, SENS_PAD_WIDTH, 2 * CSENS_SCATTER_ROWS, SENS_SCATTER_THREADS, SENS_COMBINE_COLS,
                             SENS_COMBINE_LANES, SENS_TBLOCK};
    return CS3_OK;
}

int cs3_sens_plan(cs3_handle h, int64_t k, const int32_t *Bp, const int32_t *Bi, int64_t p, const int32_t *Ctp, const int32_t *Cti,
                  int64_t side, int64_t trans, cs3_sens *out)
{
    const char *who = "cs3_sens_plan";
    int rc = guard(h); if (rc) return rc;
    if (!out) return bad_arg(who, "null output");
    *out = nullptr;
    return sens_plan_build(who, h, h->S.n, k, Bp, Bi, p, Ctp, Cti, side, trans ? CS3_CPLX_T : CS3_CPLX_N, out);
}

int cs3_cplx_sens_plan(cs3_cplx p, cs3_handle h, int64_t k, const int32_t *Bp, const int32_t *Bi, int64_t pr, const int32_t *Ctp,
                       const int32_t *Cti, int64_t side, int64_t op, cs3_cplx_sens *out)
{
    const char *who = "cs3_cplx_sens_plan";
    if (!p || !h) return bad_arg(who, "null plan or handle");
    if (!out) return bad_arg(who, "null output");
    *out = nullptr;
    if (h->S.n != 2 * p->n) return bad_arg(who, "the handle's order is not 2 n of the complex plan");
    if (int rc = sens_refuse_handle(who, h)) return rc;
    return sens_plan_build(who, h, p->n, k, Bp, Bi, pr, Ctp, Cti, side, op, out);
}

int cs3_sens_free(cs3_sens u) { return plan_free(u); }
int cs3_cplx_sens_free(cs3_cplx_sens u) { return plan_free(u); }

int cs3_sens_info(cs3_sens u, cs3_sens_info_t *out) { return sens_info("cs3_sens_info", u, out); }
int cs3_cplx_sens_info(cs3_cplx_sens u, cs3_sens_info_t *out) { return sens_info("cs3_cplx_sens_info", u, out); }

int cs3_sens_solve_dev(cs3_handle h, cs3_sens u, const double *Bx_dev, const double *Ctx_dev, double *Y_dev, void *stream)
{
    return sens_solve_dev(real_flavor("cs3_sens_solve_dev"), h, u, Bx_dev, Ctx_dev, Y_dev, stream);
}

int cs3_cplx_sens_solve_dev(cs3_cplx p, cs3_handle h, cs3_cplx_sens u, const double *Bz_dev, const double *Ctz_dev, double *Y_dev,
                            void *stream)
{
    return sens_solve_dev(cplx_flavor(p, "cs3_cplx_sens_solve_dev"), h, u, Bz_dev, Ctz_dev, Y_dev, stream);
}

int cs3_debug_sens_parts(cs3_handle h, cs3_sens u, int64_t parts, const double *Bx_dev, const double *Ctx_dev, double *Y_dev,
                         void *stream)
{
    return sens_solve_dev(real_flavor("cs3_debug_sens_parts"), h, u, Bx_dev, Ctx_dev, Y_dev, stream, parts);
}

int cs3_debug_cplx_sens_parts(cs3_cplx p, cs3_handle h, cs3_cplx_sens u, int64_t parts, const double *Bz_dev, const double *Ctz_dev,
                              double *Y_dev, void *stream)
{
    return sens_solve_dev(cplx_flavor(p, "cs3_debug_cplx_sens_parts"), h, u, Bz_dev, Ctz_dev, Y_dev, stream, parts);
}

int cs3_sens_solve(cs3_handle h, cs3_sens u, const double *Bx, const double *Ctx, double *Y)
{
    return sens_solve_host(real_flavor("cs3_sens_solve"), h, u, Bx, Ctx, Y);
}

int cs3_cplx_sens_solve(cs3_cplx p, cs3_handle h, cs3_cplx_sens u, const double *Bz, const double *Ctz, double *Y)
{
    return sens_solve_host(cplx_flavor(p, "cs3_cplx_sens_solve"), h, u, Bz, Ctz, Y);
}

// diagnostics: the handle's tile buffer (of both sens paths) to or from host memory, so that a test can look at what a
// scatter wrote and choose what a combine reads
int cs3_debug_sens_tile(cs3_handle h, int64_t write, double *host, int64_t count)
{
    int rc = guard(h); if (rc) return rc;
    auto &T = h->mem.sens.t;
    if (!host || count < 0 || (size_t) count > T.count()) {
        set_error("cs3_debug_sens_tile: null array, or more doubles than the tile buffer holds (" + std::to_string(T.count()) + ")");
        return CS3_ERR_ARG;
    }
    CS3_HIP(hipDeviceSynchronize());
    if (count) CS3_HIP(write ? hipMemcpy(T.get(), host, (size_t) count * sizeof(double), hipMemcpyHostToDevice)
                             : hipMemcpy(host, T.get(), (size_t) count * sizeof(double), hipMemcpyDeviceToHost));
    return CS3_OK;
}

// ---- selected inversion -------------------------------------------------------------------------------------------------
int cs3_selinv_limits(cs3_selinv_limits_t *out)
{
    if (!out) { set_error("cs3_selinv_limits: null output"); return CS3_ERR_ARG; }
    out->lds_max_order = SELINV_LDS_R; out->wave_max_order = SELINV_WAVE_R;
    out->gemm_tile = SELINV_TILE; out->diag_block = SELINV_DIAG;
    return CS3_OK;
}

int cs3_selinv_info(cs3_handle h, cs3_selinv_info_t *out)
{
    int rc = guard(h); if (rc) return rc;
    if (!out) { set_error("cs3_selinv_info: null output"); return CS3_ERR_ARG; }
    if ((rc = selinv_refuse(h, "cs3_selinv_info"))) return rc;
    if ((rc = ensure_selinv_plan(h))) return rc;
    const SelinvPlan &P = h->selinv.plan;
    out->zpool_doubles = P.zpool_doubles; out->nfronts_small = P.nsmall; out->nfronts_big = P.nbig; out->nlaunches = P.nlaunches;
    return CS3_OK;
}

int64_t cs3_debug_selinv_plan(cs3_handle h, int32_t *front, int32_t *launch, int64_t *entry_map, int64_t *diag_map)
{
    if (guard(h) || selinv_refuse(h, "cs3_debug_selinv_plan") || ensure_selinv_plan(h)) return -1;
    const auto &Q = h->selinv;
    if (front) std::copy(Q.plan.front_sn.begin(), Q.plan.front_sn.end(), front);
    if (launch) std::copy(Q.plan.front_launch.begin(), Q.plan.front_launch.end(), launch);
    if (entry_map) std::copy(Q.entry.begin(), Q.entry.end(), entry_map);
    if (diag_map) std::copy(Q.diag.begin(), Q.diag.end(), diag_map);
    return (int64_t) Q.plan.front_sn.size();
}

int cs3_selinv_dev(cs3_handle h, void *stream)
{
    int rc = selinv_check(h, "cs3_selinv_dev", false); if (rc) return rc;
    if ((rc = ensure_selinv(h))) return rc;
    const DeviceFactor &D = h->D;
    const SelinvPlan &P = h->selinv.plan;
    const SelinvView V{D.pool_pm, D.pm_stride, h->mem.selinv.z.get(), h->mem.selinv.work.get(), P.zpool_doubles, P.work_doubles,
                       h->mem.selinv.fronts.get(), D.rel_idx, h->batch};
    for (const SelinvGroup &g : P.groups) CS3_HIP(launch_selinv_group(D.kind, V, g, (hipStream_t) stream));
    h->selinv_valid = true;
    return CS3_OK;
}

int cs3_selinv_entries_dev(cs3_handle h, int64_t trans, double *Zx_dev, void *stream)
{
    int rc = selinv_check(h, "cs3_selinv_entries_dev", !Zx_dev && h && h->S.nnzA > 0); if (rc) return rc;
    return selinv_get_dev(h, "cs3_selinv_entries_dev", trans ? h->mem.selinv.entry_t : h->mem.selinv.entry, h->S.nnzA, Zx_dev, (hipStream_t) stream);
}

int cs3_selinv_diag_dev(cs3_handle h, double *d_dev, void *stream)
{
    int rc = selinv_check(h, "cs3_selinv_diag_dev", !d_dev && h && h->S.n > 0); if (rc) return rc;
    return selinv_get_dev(h, "cs3_selinv_diag_dev", h->mem.selinv.diag, h->S.n, d_dev, (hipStream_t) stream);
}

int cs3_selinv_entries(cs3_handle h, int64_t trans, double *Zx)
{
    int rc = selinv_check(h, "cs3_selinv_entries", !Zx && h && h->S.nnzA > 0); if (rc) return rc;
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    auto &M = h->mem.selinv;
    return selinv_get_host(h, trans ? M.entry_t : M.entry, h->S.nnzA, h->batch, M.z.get(), Zx);
}

int cs3_selinv_diag(cs3_handle h, double *d)
{
    int rc = selinv_check(h, "cs3_selinv_diag", !d && h && h->S.n > 0); if (rc) return rc;
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    auto &M = h->mem.selinv;
    return selinv_get_host(h, M.diag, h->S.n, h->batch, M.z.get(), d);
}

int cs3_selinv_factors(cs3_handle h, int64_t b, double *Zl, double *Zu)
{
    int rc = guard(h); if (rc) return rc;
    if (!Zl && !Zu) { set_error("cs3_selinv_factors: null output"); return CS3_ERR_ARG; }
    if (b < 0 || b >= h->batch) { set_error("cs3_selinv_factors: batch index out of range"); return CS3_ERR_ARG; }
    if (h->S.kind == CS3_CHOLESKY && Zu) { set_error("cs3_selinv_factors: Cholesky has no U"); return CS3_ERR_ARG; }
    if ((rc = selinv_check(h, "cs3_selinv_factors", false))) return rc;
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    const Symbolic &S = h->S;
    auto &M = h->mem.selinv;
    if (!M.lmap.get()) {                                       // Z at the positions of the CSC factors, in their (pivot-order) labels
        try { build_csc_factors(h->S); }
        catch (const std::exception &e) { set_error(e.what()); return CS3_ERR_ALLOC; }
        std::vector<i64> lmap(S.Li.size()), umap(S.Ui.size());
        for (i64 j = 0; j < S.n; ++j) {
            for (i64 p = S.Lp[j]; p < S.Lp[j + 1]; ++p) lmap[p] = selinv_position(S, h->selinv.plan, S.Li[p], j);
            if (S.kind == CS3_LU)
                for (i64 p = S.Up[j]; p < S.Up[j + 1]; ++p) umap[p] = selinv_position(S, h->selinv.plan, S.Ui[p], j);
        }
        if (std::count(lmap.begin(), lmap.end(), -1) || std::count(umap.begin(), umap.end(), -1)) {
            set_error("cs3_selinv_factors: an entry of the factors lies outside the symbolic structure");
            return CS3_ERR_STATE;
        }
        CS3_HIP(M.umap.upload(umap));
        CS3_HIP(M.lmap.upload(lmap));
    }
    const double *z = M.z.get() + b * h->selinv.plan.zpool_doubles;
    if (Zl && (rc = selinv_get_host(h, M.lmap, (int64_t) S.Li.size(), 1, z, Zl))) return rc;
    if (Zu && (rc = selinv_get_host(h, M.umap, (int64_t) S.Ui.size(), 1, z, Zu))) return rc;
    return CS3_OK;
}

// ---- complex selected inversion ------------------------------------------------------------------------------------------
int cs3_cplx_selinv_limits(cs3_cplx_selinv_limits_t *out)
{
    if (!out) { set_error("cs3_cplx_selinv_limits: null output"); return CS3_ERR_ARG; }
    out->block = CSELINV_BLOCK; out->grid_cap = CSELINV_GRID_CAP;
    return CS3_OK;
}

int cs3_debug_cplx_selinv_maps(cs3_cplx p, cs3_handle h, int64_t *entry, int64_t *entry_t, int64_t *diag)
{
    const char *who = "cs3_debug_cplx_selinv_maps";
    int rc = cselinv_check(who, p, h, nullptr, false, true);
    if (rc) return rc;
    if ((rc = ensure_cselinv_plan(p, h, who))) return rc;
    const auto &Q = h->selinv;
    if (entry) std::copy(Q.centry.begin(), Q.centry.end(), entry);
    if (entry_t) std::copy(Q.centry_t.begin(), Q.centry_t.end(), entry_t);
    if (diag) std::copy(Q.cdiag.begin(), Q.cdiag.end(), diag);
    return CS3_OK;
}

int cs3_cplx_selinv_entries_dev(cs3_cplx p, cs3_handle h, int64_t trans, double *Zz_dev, void *stream)
{
    return cselinv_dev(p, h, "cs3_cplx_selinv_entries_dev", trans ? CSELINV_ENTRIES_T : CSELINV_ENTRIES, Zz_dev, stream);
}

int cs3_cplx_selinv_diag_dev(cs3_cplx p, cs3_handle h, double *d_dev, void *stream)
{
    return cselinv_dev(p, h, "cs3_cplx_selinv_diag_dev", CSELINV_DIAG, d_dev, stream);
}

int cs3_cplx_selinv_thevenin_dev(cs3_cplx p, cs3_handle h, double *T_dev, void *stream)
{
    return cselinv_dev(p, h, "cs3_cplx_selinv_thevenin_dev", CSELINV_THEVENIN, T_dev, stream);
}

int cs3_cplx_selinv_entries(cs3_cplx p, cs3_handle h, int64_t trans, double *Zz)
{
    return cselinv_host(p, h, "cs3_cplx_selinv_entries", trans ? CSELINV_ENTRIES_T : CSELINV_ENTRIES, Zz);
}

int cs3_cplx_selinv_diag(cs3_cplx p, cs3_handle h, double *d)
{
    return cselinv_host(p, h, "cs3_cplx_selinv_diag", CSELINV_DIAG, d);
}

int cs3_cplx_selinv_thevenin(cs3_cplx p, cs3_handle h, double *T)
{
    return cselinv_host(p, h, "cs3_cplx_selinv_thevenin", CSELINV_THEVENIN, T);
}

// ---- bilinear forms on the selected inverse -------------------------------------------------------------------------------
int cs3_quad_limits(cs3_quad_limits_t *out)
{
    if (!out) { set_error("cs3_quad_limits: null output"); return CS3_ERR_ARG; }
    *out = cs3_quad_limits_t{QUAD_LANE_TERMS, QUAD_WAVE_TERMS, QUAD_BLOCK, QUAD_CHUNK, QUAD_BLOCK};
    return CS3_OK;
}

int cs3_quad_plan(cs3_handle h, int64_t m, const int32_t *Ctp, const int32_t *Cti, const int32_t *Btp, const int32_t *Bti, cs3_quadplan *out)
{
    const char *who = "cs3_quad_plan";
    int rc = guard(h); if (rc) return rc;
    if (!out) return bad_arg(who, "null output");
    *out = nullptr;
    if (!Ctp) return bad_arg(who, "null row pointers of C");
    if (m < 1 || m > (1LL << 30)) return bad_arg(who, "m must be between 1 and 2^30");
    if ((rc = sens_check_pointers(who, "Ctp", m, Ctp, Cti))) return rc;
    if (Btp && (rc = sens_check_pointers(who, "Btp", m, Btp, Bti))) return rc;
    if ((rc = sens_check_indices(who, "C'", h->S.n, m, Ctp, Cti))) return rc;
    if (Btp && (rc = sens_check_indices(who, "B'", h->S.n, m, Btp, Bti))) return rc;
    if ((rc = selinv_refuse(h, who))) return rc;
    if ((rc = ensure_selinv_plan(h))) return rc;
    try {
        std::unique_ptr<cs3_quad_s> u(new cs3_quad_s());
        if ((rc = quad_build(h, *u, m, Ctp, Cti, Btp, Bti, who))) return rc;
        h->plans.push_back(u.get());
        u->h = h;
        *out = u.release();
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of memory"); return CS3_ERR_ALLOC;
    }
    return CS3_OK;
}

int cs3_quad_free(cs3_quadplan q) { return plan_free(q); }

int cs3_quad_info(cs3_quadplan q, cs3_quad_info_t *out)
{
    if (!q || !out) return bad_arg("cs3_quad_info", "null argument");
    *out = cs3_quad_info_t{q->m, q->nnz_c, q->nnz_b, q->term_ptr[(size_t) q->m], q->same ? 1 : 0, q->shape.n_lane, q->shape.n_wave,
                           q->shape.n_wg};
    return CS3_OK;
}

int cs3_debug_quad_plan(cs3_quadplan q, int32_t *row_class, int64_t *term_ptr, int64_t *term_pos)
{
    if (!q) return bad_arg("cs3_debug_quad_plan", "null plan");
    if (row_class) std::copy(q->row_class.begin(), q->row_class.end(), row_class);
    if (term_ptr) std::copy(q->term_ptr.begin(), q->term_ptr.end(), term_ptr);
    if (term_pos) std::copy(q->term_pos.begin(), q->term_pos.end(), term_pos);
    return CS3_OK;
}

int cs3_quad_dev(cs3_handle h, cs3_quadplan q, const double *Cx_dev, const double *Bx_dev, double *t_dev, void *stream)
{
    int rc = quad_check("cs3_quad_dev", h, q, q && (!t_dev || (q->nnz_c > 0 && !Cx_dev) || (!q->same && q->nnz_b > 0 && !Bx_dev)), true);
    if (rc) return rc;
    return quad_run(h, q, Cx_dev, Bx_dev, t_dev, (hipStream_t) stream);
}

int cs3_quad(cs3_handle h, cs3_quadplan q, const double *Cx, const double *Bx, double *t)
{
    int rc = quad_check("cs3_quad", h, q, q && (!t || (q->nnz_c > 0 && !Cx) || (!q->same && q->nnz_b > 0 && !Bx)), false);
    if (rc) return rc;
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    auto &M = q->mem;
    const size_t nt = (size_t) (h->batch * q->m);
    if ((rc = quad_stage(M.cx, Cx, (size_t) (h->batch * q->nnz_c)))) return rc;
    if (!q->same && (rc = quad_stage(M.bx, Bx, (size_t) (h->batch * q->nnz_b)))) return rc;
    CS3_HIP(M.out.reserve(nt));
    if ((rc = quad_run(h, q, M.cx.get(), M.bx.get(), M.out.get(), nullptr))) return rc;
    CS3_HIP(hipMemcpy(t, M.out.get(), nt * sizeof(double), hipMemcpyDeviceToHost));
    CS3_HIP(hipDeviceSynchronize());
    return CS3_OK;
}

int cs3_quad_normres_dev(cs3_handle h, cs3_quadplan q, const double *Hx_dev, const double *w_dev, const double *r_dev, double crit_tol,
                         double *t_dev, double *omega_dev, double *rn_dev, double *summary_dev, void *stream)
{
    const char *who = "cs3_quad_normres_dev";
    int rc = quad_check(who, h, q, q && (!summary_dev || !w_dev || !r_dev || (q->nnz_c > 0 && !Hx_dev)), true);
    if (rc) return rc;
    if (!q->same) return bad_arg(who, "the plan has a B of its own (the normalised residuals need B = C)");
    return quad_normres_run(h, q, Hx_dev, w_dev, r_dev, crit_tol, t_dev, omega_dev, rn_dev, summary_dev, (hipStream_t) stream);
}

int cs3_quad_normres(cs3_handle h, cs3_quadplan q, const double *Hx, const double *w, const double *r, double crit_tol, double *t,
                     double *omega, double *rn, double *summary)
{
    const char *who = "cs3_quad_normres";
    int rc = quad_check(who, h, q, q && (!summary || !w || !r || (q->nnz_c > 0 && !Hx)), false);
    if (rc) return rc;
    if (!q->same) return bad_arg(who, "the plan has a B of its own (the normalised residuals need B = C)");
    if (!h->selinv_valid && (rc = cs3_selinv_dev(h, nullptr))) return rc;
    auto &M = q->mem;
    const size_t nm = (size_t) (h->batch * q->m), ns = 4 * (size_t) h->batch;
    if ((rc = quad_stage(M.cx, Hx, (size_t) (h->batch * q->nnz_c)))) return rc;
    if ((rc = quad_stage(M.w, w, nm)) || (rc = quad_stage(M.r, r, nm))) return rc;
    CS3_HIP(M.out.reserve(3 * nm + ns));                   // t, omega, rn, summary
    double *o = M.out.get();
    if ((rc = quad_normres_run(h, q, M.cx.get(), M.w.get(), M.r.get(), crit_tol, o, o + nm, o + 2 * nm, o + 3 * nm, nullptr))) return rc;
    if (t) CS3_HIP(hipMemcpy(t, o, nm * sizeof(double), hipMemcpyDeviceToHost));
    if (omega) CS3_HIP(hipMemcpy(omega, o + nm, nm * sizeof(double), hipMemcpyDeviceToHost));
    if (rn) CS3_HIP(hipMemcpy(rn, o + 2 * nm, nm * sizeof(double), hipMemcpyDeviceToHost));
    CS3_HIP(hipMemcpy(summary, o + 3 * nm, ns * sizeof(double), hipMemcpyDeviceToHost));
    CS3_HIP(hipDeviceSynchronize());
    return CS3_OK;
}

}  // extern "C"
