// AC state estimation, host side (include/csparse3_amd.h, "AC state estimation"): from the pattern of a bus admittance
// matrix, a table of branch ends, the reference buses and a list of measurements, the pattern of the measurement Jacobian H
// by rows and in CSC, the descriptor of every entry that k_se_jacobian reads, and Y by rows.  The first call that needs the
// solver adds the three existing subsystems on top: the sparse product H' (W H), a Cholesky handle on its pattern, the
// bilinear-form plan of the rows of H.  Then the entry points around the launches of stateest.hip and the Gauss-Newton driver.
//
// Cost of the plan: O(nnz_y + n + ne + nnz_h); the analysis of the gain matrix (cs3_analyze) comes with the first solve.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_handle.hpp"
#include "cs3_internal.hpp"
#include "cs3_se.hpp"

using namespace cs3;

namespace {

constexpr long long SE_ENTRY_LIMIT = (1LL << 29) - 256;      // entries of Y, and of H
constexpr unsigned long long SE_INF_BITS = 0x7ff0000000000000ull;

int se_bad(const std::string &msg) { set_error("cs3_se_plan_create: " + msg); return CS3_ERR_ARG; }

}  // namespace

extern "C" {

int cs3_se_plan_create(int64_t n, const int32_t *Yp, const int32_t *Yi, int64_t nref, const int32_t *ref, int64_t ne,
                       const int32_t *end_from, const int32_t *end_to, int64_t m, const int32_t *kind, const int32_t *where,
                       int64_t order, cs3_se *out)
{
    // 1. null pointers
    if (!out) return se_bad("null output");
    *out = nullptr;
    if (!Yp) return se_bad("null column pointers");
    if (nref > 0 && !ref) return se_bad("null reference list");
    if (ne > 0 && (!end_from || !end_to)) return se_bad("null branch-end table");
    if (m > 0 && (!kind || !where)) return se_bad("null measurement list");
    // 2. the pattern, by the checks of cs3_pf_plan_create; the order
    if (n < 0 || n >= ((int64_t) 1 << 30)) return se_bad("bad order n");
    if (Yp[0] != 0) return se_bad("Yp[0] != 0");
    for (int64_t j = 0; j < n; ++j)
        if (Yp[j + 1] < Yp[j]) return se_bad("Yp decreases at column " + std::to_string(j));
    const int64_t nnz = Yp[n];
    if (nnz > 0 && !Yi) return se_bad("null row indices");
    for (int64_t q = 0; q < nnz; ++q)
        if (Yi[q] < 0 || Yi[q] >= n) return se_bad("row index out of range at entry " + std::to_string(q));
    if (nnz >= SE_ENTRY_LIMIT) return se_bad("Y has " + std::to_string(nnz) + " entries (limit 2^29 - 256)");
    if (order != CS3_ORDER_NATURAL && order != CS3_ORDER_AMD) return se_bad("order must be 0 (natural) or 1 (AMD)");

    cs3_se_s *pl = nullptr;
    try {
        pl = new cs3_se_s;
        pl->n = n; pl->nnz_y = nnz; pl->ne = ne; pl->m = m; pl->order = order;
        std::vector<char> has_diag((size_t) n, 0);
        {
            std::vector<int32_t> stamp((size_t) n, -1);
            for (int64_t j = 0; j < n; ++j)
                for (int32_t q = Yp[j]; q < Yp[j + 1]; ++q) {
                    const int32_t i = Yi[q];
                    if (stamp[(size_t) i] == (int32_t) j) {
                        delete pl;
                        return se_bad("row " + std::to_string(i) + " is stored twice in column " + std::to_string(j));
                    }
                    stamp[(size_t) i] = (int32_t) j;
                    if (i == j) has_diag[(size_t) j] = 1;
                }
        }
        // 3. the reference buses
        if (nref < 1) { delete pl; return se_bad("nref < 1: a reference bus is required"); }
        if (nref > n) { delete pl; return se_bad("bad length of the reference list"); }
        pl->upos_a.assign((size_t) n, 0);
        for (int64_t k = 0; k < nref; ++k) {
            if (ref[k] < 0 || ref[k] >= n) { delete pl; return se_bad("ref[" + std::to_string(k) + "] out of range"); }
            if (pl->upos_a[(size_t) ref[k]] < 0) { delete pl; return se_bad("ref[" + std::to_string(k) + "] repeats an earlier entry"); }
            pl->upos_a[(size_t) ref[k]] = -1;
        }
        pl->nref = nref; pl->na = n - nref; pl->ns = 2 * n - nref;
        pl->upos_m.resize((size_t) n);
        pl->sbus.resize((size_t) pl->ns);
        {
            int32_t next = 0;
            for (int64_t i = 0; i < n; ++i) {
                if (pl->upos_a[(size_t) i] >= 0) { pl->upos_a[(size_t) i] = next; pl->sbus[(size_t) next++] = (int32_t) i; }
                pl->upos_m[(size_t) i] = (int32_t) (pl->na + i);
                pl->sbus[(size_t) (pl->na + i)] = (int32_t) i;
            }
        }
        // 4. the branch ends
        if (ne < 0 || ne > INT_MAX) { delete pl; return se_bad("bad number of branch ends"); }
        for (int64_t k = 0; k < ne; ++k) {
            if (end_from[k] < 0 || end_from[k] >= n || end_to[k] < 0 || end_to[k] >= n) { delete pl; return se_bad("branch end " + std::to_string(k) + " out of range"); }
            if (end_from[k] == end_to[k]) { delete pl; return se_bad("branch end " + std::to_string(k) + " has from == to"); }
        }
        if (ne) { pl->end_from.assign(end_from, end_from + ne); pl->end_to.assign(end_to, end_to + ne); }
        // 5. - 8. the measurements
        if (m < 1) { delete pl; return se_bad("m < 1: a measurement is required"); }
        if (m > INT_MAX) { delete pl; return se_bad("m does not fit 32-bit row indices"); }
        for (int64_t i = 0; i < m; ++i)
            if (kind[i] < 0 || kind[i] > 4) { delete pl; return se_bad("kind[" + std::to_string(i) + "] outside 0..4"); }
        for (int64_t i = 0; i < m; ++i)
            if (where[i] < 0 || where[i] >= (kind[i] <= 2 ? n : ne)) {
                delete pl;
                return se_bad("where[" + std::to_string(i) + "] out of range for " + (kind[i] <= 2 ? "a bus" : "a branch end"));
            }
        for (int64_t i = 0; i < m; ++i)
            if ((kind[i] == 1 || kind[i] == 2) && !has_diag[(size_t) where[i]]) {
                delete pl;
                return se_bad("injection row " + std::to_string(i) + ": bus " + std::to_string(where[i]) + " has no stored diagonal entry");
            }
        pl->kind.assign(kind, kind + m); pl->where.assign(where, where + m);

        // Y by rows, ascending column (a counting sort over the columns in order), with the entry behind every one
        pl->Rp.assign((size_t) n + 1, 0);
        for (int64_t q = 0; q < nnz; ++q) ++pl->Rp[(size_t) Yi[q] + 1];
        for (int64_t i = 0; i < n; ++i) pl->Rp[(size_t) i + 1] += pl->Rp[(size_t) i];
        pl->Rj.resize((size_t) nnz); pl->Rpos.resize((size_t) nnz);
        {
            std::vector<int32_t> next(pl->Rp.begin(), pl->Rp.end() - 1);
            for (int64_t j = 0; j < n; ++j)
                for (int32_t q = Yp[j]; q < Yp[j + 1]; ++q) {
                    const int32_t at = next[(size_t) Yi[q]]++;
                    pl->Rj[(size_t) at] = (int32_t) j; pl->Rpos[(size_t) at] = q;
                }
        }
        for (int64_t i = 0; i < n; ++i) {
            const int64_t d = pl->Rp[(size_t) i + 1] - pl->Rp[(size_t) i];
            pl->max_row = std::max(pl->max_row, d);
            if (d > SE_WAVE_ROW) pl->wave_rows.push_back((int32_t) i);
        }

        // 9. the size of H
        long long total = 0;
        for (int64_t i = 0; i < m; ++i) {
            ++pl->nkind[kind[i]];
            if (kind[i] == 0) { total += 1; continue; }
            if (kind[i] >= 3) {
                total += 2 + (pl->upos_a[(size_t) end_from[where[i]]] >= 0) + (pl->upos_a[(size_t) end_to[where[i]]] >= 0);
                continue;
            }
            const int32_t b = where[i];
            total += pl->Rp[(size_t) b + 1] - pl->Rp[(size_t) b];
            for (int32_t p = pl->Rp[(size_t) b]; p < pl->Rp[(size_t) b + 1]; ++p) total += pl->upos_a[(size_t) pl->Rj[(size_t) p]] >= 0;
            if (total >= SE_ENTRY_LIMIT) break;
        }
        if (total >= SE_ENTRY_LIMIT) { delete pl; return se_bad("H has 2^29 - 256 entries or more"); }
        pl->nnz_h = total;

        // H by rows with the descriptor of every entry: the angle entries of a row, then its magnitude entries
        pl->Hrp.assign((size_t) m + 1, 0);
        pl->Hrj.reserve((size_t) total); pl->e_row.reserve((size_t) total); pl->e_src.reserve((size_t) total);
        pl->e_code.reserve((size_t) total); pl->e_bus.reserve((size_t) total);
        auto put = [&](int64_t row, int32_t state, int32_t src, int32_t code, int32_t bus) {
            pl->Hrj.push_back(state); pl->e_row.push_back((int32_t) row); pl->e_src.push_back(src); pl->e_code.push_back(code);
            pl->e_bus.push_back(bus);
        };
        for (int64_t i = 0; i < m; ++i) {
            const int32_t at = where[i];
            const int32_t imag = (kind[i] == 2 || kind[i] == 4) ? SE_E_IMAG : 0;
            if (kind[i] == 0) {
                put(i, pl->upos_m[(size_t) at], 0, SE_E_ONE, at);
            } else if (kind[i] <= 2) {
                for (int pass = 0; pass < 2; ++pass)
                    for (int32_t p = pl->Rp[(size_t) at]; p < pl->Rp[(size_t) at + 1]; ++p) {
                        const int32_t j = pl->Rj[(size_t) p];
                        const int32_t state = pass ? pl->upos_m[(size_t) j] : pl->upos_a[(size_t) j];
                        if (state >= 0) put(i, state, pl->Rpos[(size_t) p], SE_E_INJ | imag | (pass ? SE_E_MAG : 0) | (j == at ? SE_E_NEAR : 0), j);
                    }
            } else {
                const int32_t ends[2] = {end_from[at], end_to[at]};
                for (int pass = 0; pass < 2; ++pass)
                    for (int side = 0; side < 2; ++side) {
                        const int32_t j = ends[side];
                        const int32_t state = pass ? pl->upos_m[(size_t) j] : pl->upos_a[(size_t) j];
                        if (state >= 0) put(i, state, at, SE_E_FLOW | imag | (pass ? SE_E_MAG : 0) | (side == 0 ? SE_E_NEAR : 0), j);
                    }
            }
            pl->Hrp[(size_t) i + 1] = (int32_t) pl->Hrj.size();
        }
        // H in CSC: a counting sort of the row-order entries by column keeps the measurements of a column ascending
        pl->Hp.assign((size_t) pl->ns + 1, 0);
        for (int32_t c : pl->Hrj) ++pl->Hp[(size_t) c + 1];
        for (int64_t j = 0; j < pl->ns; ++j) pl->Hp[(size_t) j + 1] += pl->Hp[(size_t) j];
        pl->Hi.resize((size_t) total); pl->cpos.resize((size_t) total);
        {
            std::vector<int32_t> next(pl->Hp.begin(), pl->Hp.end() - 1);
            for (int64_t q = 0; q < total; ++q) {
                const int32_t at = next[(size_t) pl->Hrj[(size_t) q]]++;
                pl->Hi[(size_t) at] = pl->e_row[(size_t) q]; pl->cpos[(size_t) q] = at;
            }
        }
        for (int64_t j = 0; j < pl->ns; ++j) {
            const int64_t d = pl->Hp[(size_t) j + 1] - pl->Hp[(size_t) j];
            pl->max_col = std::max(pl->max_col, d);
            if (d > SE_WAVE_COL) pl->wave_cols.push_back((int32_t) j);
        }
    } catch (const std::bad_alloc &) {
        delete pl; set_error("cs3_se_plan_create: out of memory"); return CS3_ERR_ALLOC;
    }
    *out = pl;
    return CS3_OK;
}

int cs3_se_plan_free(cs3_se p)
{
    if (!p) return CS3_OK;
    cs3_quad_free(p->quad);
    cs3_free(p->h);
    cs3_spgemm_plan_free(p->gain);
    delete p;
    return CS3_OK;
}

int cs3_se_plan_info(cs3_se p, cs3_se_info *info)
{
    if (!p || !info) { set_error("cs3_se_plan_info: null argument"); return CS3_ERR_ARG; }
    info->n = p->n; info->nnz_y = p->nnz_y; info->nref = p->nref; info->na = p->na; info->ns = p->ns; info->ne = p->ne;
    info->m = p->m; info->nnz_h = p->nnz_h;
    for (int k = 0; k < 5; ++k) info->nkind[k] = p->nkind[k];
    info->max_row = p->max_row; info->max_col = p->max_col;
    info->rows_wave = (int64_t) p->wave_rows.size(); info->cols_wave = (int64_t) p->wave_cols.size();
    info->nnz_g = p->h ? (int64_t) p->Gi.size() : 0;
    return CS3_OK;
}

int cs3_se_plan_pattern(cs3_se p, int32_t *Hp, int32_t *Hi, int32_t *Rp, int32_t *Rj)
{
    if (!p) { set_error("cs3_se_plan_pattern: null plan"); return CS3_ERR_ARG; }
    const size_t nnz = (size_t) p->nnz_h;
    if (Hp) std::memcpy(Hp, p->Hp.data(), p->Hp.size() * 4);
    if (Hi) std::memcpy(Hi, p->Hi.data(), nnz * 4);
    if (Rp) std::memcpy(Rp, p->Hrp.data(), p->Hrp.size() * 4);
    if (Rj) std::memcpy(Rj, p->Hrj.data(), nnz * 4);
    return CS3_OK;
}

int cs3_se_plan_maps(cs3_se p, int32_t *cpos, int32_t *upos_a, int32_t *upos_m)
{
    if (!p) { set_error("cs3_se_plan_maps: null plan"); return CS3_ERR_ARG; }
    if (cpos) std::memcpy(cpos, p->cpos.data(), (size_t) p->nnz_h * 4);
    if (upos_a && p->n) std::memcpy(upos_a, p->upos_a.data(), (size_t) p->n * 4);
    if (upos_m && p->n) std::memcpy(upos_m, p->upos_m.data(), (size_t) p->n * 4);
    return CS3_OK;
}

int cs3_se_limits(cs3_se_limits_t *out)
{
    if (!out) { set_error("cs3_se_limits: null output"); return CS3_ERR_ARG; }
    out->block = SE_BLOCK;
    out->grid_cap = SE_GRID_CAP;
    out->wave_row = SE_WAVE_ROW;
    out->wave_col = SE_WAVE_COL;
    return CS3_OK;
}

}  // extern "C"

// ---- the numeric phase: the solver behind the plan, entry points around the launches of stateest.hip, the driver -------
namespace {

// The spgemm plan H' (W H), the Cholesky handle on its pattern, the rows of H as a bilinear-form plan, the work arrays.
int se_ensure_solver(cs3_se_s *p)
{
    if (int rc = se_upload(p)) return rc;
    if (!p->gain) {
        const int rc = cs3_spgemm_plan_create(p->m, p->ns, p->Hp.data(), p->Hi.data(), p->m, p->ns, p->Hp.data(), p->Hi.data(), 1, &p->gain);
        if (rc) { p->gain = nullptr; return rc; }
    }
    if (!p->h) {
        cs3_spgemm_info gi;
        if (int rc = cs3_spgemm_plan_info(p->gain, &gi)) return rc;
        try {
            p->Gp.assign((size_t) p->ns + 1, 0);
            p->Gi.assign((size_t) gi.nnz_c, 0);
        } catch (const std::bad_alloc &) { set_error("cs3_se: out of memory"); return CS3_ERR_ALLOC; }
        if (int rc = cs3_spgemm_plan_pattern(p->gain, p->Gp.data(), p->Gi.data())) return rc;
        const int rc = cs3_analyze(CS3_CHOLESKY, p->order, p->ns, p->Gp.data(), p->Gi.data(), nullptr, 1, &p->h);
        if (rc) { p->h = nullptr; return rc; }                          // (a refusal of the analysis, with its message)
    }
    if (!p->quad) {
        const int rc = cs3_quad_plan(p->h, p->m, p->Hrp.data(), p->Hrj.data(), nullptr, nullptr, &p->quad);
        if (rc) { p->quad = nullptr; return rc; }
    }
    if (!p->work) {
        auto &m = p->mem;
        CS3_HIP(m.hr.reserve((size_t) p->nnz_h));
        CS3_HIP(m.hc.reserve((size_t) p->nnz_h));
        CS3_HIP(m.whc.reserve((size_t) p->nnz_h));
        CS3_HIP(m.gx.reserve(p->Gi.size()));
        CS3_HIP(m.rhs.reserve((size_t) p->ns));
        p->work = true;
    }
    return CS3_OK;
}

int se_stage(DevBuf<double> &d, const double *src, size_t count) { CS3_HIP(d.upload(src, count)); return CS3_OK; }

int se_check_solve(const char *who, double tol, int64_t max_iters)
{
    if (!(tol >= 0.0) || !std::isfinite(tol)) { set_error(std::string(who) + ": tol must be finite and >= 0"); return CS3_ERR_ARG; }
    if (max_iters < 0 || max_iters > INT_MAX) { set_error(std::string(who) + ": max_iters must be >= 0"); return CS3_ERR_ARG; }
    return CS3_OK;
}

}  // namespace

extern "C" {

int cs3_se_handle(cs3_se p, cs3_handle *h)
{
    if (!p || !h) { set_error("cs3_se_handle: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_ensure_solver(p)) return rc;
    *h = p->h;
    return CS3_OK;
}

int cs3_se_gain_pattern(cs3_se p, int32_t *Gp, int32_t *Gi)
{
    if (!p) { set_error("cs3_se_gain_pattern: null plan"); return CS3_ERR_ARG; }
    if (int rc = se_ensure_solver(p)) return rc;
    if (Gp) std::memcpy(Gp, p->Gp.data(), p->Gp.size() * 4);
    if (Gi && !p->Gi.empty()) std::memcpy(Gi, p->Gi.data(), p->Gi.size() * 4);
    return CS3_OK;
}

int cs3_se_residuals_dev(cs3_se p, const double **r_dev, const double **wr_dev)
{
    if (!p) { set_error("cs3_se_residuals_dev: null plan"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    if (r_dev) *r_dev = p->mem.r.get();
    if (wr_dev) *wr_dev = p->mem.wr.get();
    return CS3_OK;
}

int cs3_se_measure_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev,
                       const double *vm_dev, const double *va_dev, double *r_dev, double *J_dev, void *stream)
{
    if (!p || !Yz_dev || (p->ne > 0 && !Ye_dev) || !z_dev || !w_dev || !vm_dev || !va_dev) { set_error("cs3_se_measure_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    if (int rc = se_launch_currents(p, Yz_dev, vm_dev, va_dev, st)) return rc;
    return se_launch_residual(p, Ye_dev, z_dev, w_dev, vm_dev, r_dev, J_dev, st);
}

int cs3_se_jacobian_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *w_dev, const double *vm_dev,
                        const double *va_dev, double *Hr_dev, double *Hc_dev, double *WHc_dev, void *stream)
{
    if (!p || !Yz_dev || (p->ne > 0 && !Ye_dev) || !vm_dev || !va_dev || (WHc_dev && !w_dev)) { set_error("cs3_se_jacobian_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    if (int rc = se_launch_currents(p, Yz_dev, vm_dev, va_dev, st)) return rc;
    return se_launch_jacobian(p, Yz_dev, Ye_dev, w_dev, vm_dev, Hr_dev, Hc_dev, WHc_dev, st);
}

int cs3_se_gradient_dev(cs3_se p, const double *Hc_dev, const double *wr_dev, double *g_dev, void *stream)
{
    if (!p || !Hc_dev || !wr_dev || !g_dev) { set_error("cs3_se_gradient_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    return se_launch_gradient(p, Hc_dev, wr_dev, g_dev, (hipStream_t) stream);
}

int cs3_se_solve_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev, double *vm_dev,
                     double *va_dev, double tol, int64_t max_iters, int32_t *iters, double *step, double *J, int32_t *flag, void *stream)
{
    if (!p || !Yz_dev || (p->ne > 0 && !Ye_dev) || !z_dev || !w_dev || !vm_dev || !va_dev) { set_error("cs3_se_solve_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_check_solve("cs3_se_solve_dev", tol, max_iters)) return rc;
    if (int rc = se_ensure_solver(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    auto &m = p->mem;
    int32_t done = 0, fl = 1;
    double last = 0.0;
    auto report = [&](int32_t n_done, double s, int32_t f) {
        if (iters) *iters = n_done;
        if (step) *step = s;
        if (flag) *flag = f;
    };
    for (int64_t it = 0; it < max_iters; ++it) {
        if (int rc = se_launch_currents(p, Yz_dev, vm_dev, va_dev, st)) return rc;
        if (int rc = se_launch_residual(p, Ye_dev, z_dev, w_dev, vm_dev, nullptr, nullptr, st)) return rc;
        if (int rc = se_launch_jacobian(p, Yz_dev, Ye_dev, w_dev, vm_dev, nullptr, m.hc.get(), m.whc.get(), st)) return rc;
        if (int rc = se_launch_gradient(p, m.hc.get(), m.wr.get(), m.rhs.get(), st)) return rc;
        if (int rc = cs3_spgemm_values_dev(p->gain, m.hc.get(), m.whc.get(), m.gx.get(), stream)) return rc;
        if (int rc = cs3_factor_solve_dev(p->h, m.gx.get(), 0.0, m.rhs.get(), 1, stream)) return rc;
        if (int rc = se_launch_update(p, m.rhs.get(), vm_dev, va_dev, p->h->D.status, st)) return rc;
        // the one host read of an iteration: max |dx| and the status of the factorisation behind it
        unsigned long long bits = 0;
        int status[4] = {0x7f7f7f7f, 0, 0, 0};
        CS3_HIP(hipMemcpyAsync(&bits, m.dxbits.get(), sizeof(bits), hipMemcpyDeviceToHost, st));
        CS3_HIP(hipMemcpyAsync(status, p->h->D.status, sizeof(status), hipMemcpyDeviceToHost, st));
        CS3_HIP(hipStreamSynchronize(st));
        if (status[0] != 0x7f7f7f7f || status[3] != 0) {                // (k_se_update moved nothing)
            report(done, last, 1);                                      // the completed iterations; J is not written
            return cs3_factor_status(p->h, stream);
        }
        done = (int32_t) (it + 1);
        std::memcpy(&last, &bits, sizeof(last));
        if (bits >= SE_INF_BITS) { fl = 2; break; }
        if (last <= tol) { fl = 0; break; }
        fl = 1;
    }
    // r and J of the returned state
    if (int rc = se_launch_currents(p, Yz_dev, vm_dev, va_dev, st)) return rc;
    if (int rc = se_launch_residual(p, Ye_dev, z_dev, w_dev, vm_dev, nullptr, m.jsum.get(), st)) return rc;
    if (J) CS3_HIP(hipMemcpyAsync(J, m.jsum.get(), sizeof(double), hipMemcpyDeviceToHost, st));
    CS3_HIP(hipStreamSynchronize(st));
    report(done, last, fl);
    return CS3_OK;
}

int cs3_se_baddata_dev(cs3_se p, const double *Yz_dev, const double *Ye_dev, const double *z_dev, const double *w_dev,
                       const double *vm_dev, const double *va_dev, double crit_tol, double *t_dev, double *omega_dev, double *rn_dev,
                       double *summary_dev, void *stream)
{
    if (!p || !Yz_dev || (p->ne > 0 && !Ye_dev) || !z_dev || !w_dev || !vm_dev || !va_dev || !summary_dev) { set_error("cs3_se_baddata_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_ensure_solver(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    auto &m = p->mem;
    if (int rc = se_launch_currents(p, Yz_dev, vm_dev, va_dev, st)) return rc;
    if (int rc = se_launch_residual(p, Ye_dev, z_dev, w_dev, vm_dev, nullptr, nullptr, st)) return rc;
    if (int rc = se_launch_jacobian(p, Yz_dev, Ye_dev, w_dev, vm_dev, m.hr.get(), m.hc.get(), m.whc.get(), st)) return rc;
    if (int rc = cs3_spgemm_values_dev(p->gain, m.hc.get(), m.whc.get(), m.gx.get(), stream)) return rc;
    if (int rc = cs3_factor_dev(p->h, m.gx.get(), 0.0, stream)) return rc;
    if (int rc = cs3_selinv_dev(p->h, stream)) return rc;
    return cs3_quad_normres_dev(p->h, p->quad, m.hr.get(), w_dev, m.r.get(), crit_tol, t_dev, omega_dev, rn_dev, summary_dev, stream);
}

// ---- the host-array forms: the null stream, the same kernels in the same order

int cs3_se_measure(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, const double *vm, const double *va,
                   double *r, double *J)
{
    if (!p || !Yz || (p->ne > 0 && !Ye) || !z || !w || !vm || !va) { set_error("cs3_se_measure: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    const size_t n = (size_t) p->n, m = (size_t) p->m;
    DevBuf<double> y, e, zz, ww, a, b, rr, jj;
    int rc;
    if ((rc = se_stage(y, Yz, (size_t) p->nnz_y * 2)) || (rc = se_stage(e, Ye, (size_t) p->ne * 4)) || (rc = se_stage(zz, z, m)) ||
        (rc = se_stage(ww, w, m)) || (rc = se_stage(a, vm, n)) || (rc = se_stage(b, va, n))) return rc;
    CS3_HIP(rr.alloc(m));
    CS3_HIP(jj.alloc(1));
    if ((rc = cs3_se_measure_dev(p, y.get(), e.get(), zz.get(), ww.get(), a.get(), b.get(), rr.get(), jj.get(), nullptr))) return rc;
    if (r) CS3_HIP(hipMemcpy(r, rr.get(), m * 8, hipMemcpyDeviceToHost));
    if (J) CS3_HIP(hipMemcpy(J, jj.get(), 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_se_jacobian(cs3_se p, const double *Yz, const double *Ye, const double *w, const double *vm, const double *va, double *Hr,
                    double *Hc, double *WHc)
{
    if (!p || !Yz || (p->ne > 0 && !Ye) || !vm || !va || (WHc && !w)) { set_error("cs3_se_jacobian: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    const size_t n = (size_t) p->n, m = (size_t) p->m, nnz = (size_t) p->nnz_h;
    DevBuf<double> y, e, ww, a, b, hr, hc, whc;
    int rc;
    if ((rc = se_stage(y, Yz, (size_t) p->nnz_y * 2)) || (rc = se_stage(e, Ye, (size_t) p->ne * 4)) || (w && (rc = se_stage(ww, w, m))) ||
        (rc = se_stage(a, vm, n)) || (rc = se_stage(b, va, n))) return rc;
    if (Hr) CS3_HIP(hr.alloc(nnz));
    if (Hc) CS3_HIP(hc.alloc(nnz));
    if (WHc) CS3_HIP(whc.alloc(nnz));
    if ((rc = cs3_se_jacobian_dev(p, y.get(), e.get(), w ? ww.get() : nullptr, a.get(), b.get(), Hr ? hr.get() : nullptr,
                                  Hc ? hc.get() : nullptr, WHc ? whc.get() : nullptr, nullptr))) return rc;
    CS3_HIP(hipDeviceSynchronize());
    if (Hr) CS3_HIP(hipMemcpy(Hr, hr.get(), nnz * 8, hipMemcpyDeviceToHost));
    if (Hc) CS3_HIP(hipMemcpy(Hc, hc.get(), nnz * 8, hipMemcpyDeviceToHost));
    if (WHc) CS3_HIP(hipMemcpy(WHc, whc.get(), nnz * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_se_solve(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, double *vm, double *va, double tol,
                 int64_t max_iters, int32_t *iters, double *step, double *J, int32_t *flag)
{
    if (!p || !Yz || (p->ne > 0 && !Ye) || !z || !w || !vm || !va) { set_error("cs3_se_solve: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_check_solve("cs3_se_solve", tol, max_iters)) return rc;
    if (int rc = se_upload(p)) return rc;
    const size_t n = (size_t) p->n, m = (size_t) p->m;
    DevBuf<double> y, e, zz, ww, a, b;
    int rc;
    if ((rc = se_stage(y, Yz, (size_t) p->nnz_y * 2)) || (rc = se_stage(e, Ye, (size_t) p->ne * 4)) || (rc = se_stage(zz, z, m)) ||
        (rc = se_stage(ww, w, m)) || (rc = se_stage(a, vm, n)) || (rc = se_stage(b, va, n))) return rc;
    rc = cs3_se_solve_dev(p, y.get(), e.get(), zz.get(), ww.get(), a.get(), b.get(), tol, max_iters, iters, step, J, flag, nullptr);
    if (rc && rc != CS3_ERR_NOT_SPD) return rc;
    CS3_HIP(hipMemcpy(vm, a.get(), n * 8, hipMemcpyDeviceToHost));          // (after a failed pivot: the last completed update)
    CS3_HIP(hipMemcpy(va, b.get(), n * 8, hipMemcpyDeviceToHost));
    return rc;
}

int cs3_se_baddata(cs3_se p, const double *Yz, const double *Ye, const double *z, const double *w, const double *vm, const double *va,
                   double crit_tol, double *t, double *omega, double *rn, double *summary)
{
    if (!p || !Yz || (p->ne > 0 && !Ye) || !z || !w || !vm || !va || !summary) { set_error("cs3_se_baddata: null argument"); return CS3_ERR_ARG; }
    if (int rc = se_upload(p)) return rc;
    const size_t n = (size_t) p->n, m = (size_t) p->m;
    DevBuf<double> y, e, zz, ww, a, b, tt, oo, rr, ss;
    int rc;
    if ((rc = se_stage(y, Yz, (size_t) p->nnz_y * 2)) || (rc = se_stage(e, Ye, (size_t) p->ne * 4)) || (rc = se_stage(zz, z, m)) ||
        (rc = se_stage(ww, w, m)) || (rc = se_stage(a, vm, n)) || (rc = se_stage(b, va, n))) return rc;
    CS3_HIP(tt.alloc(m)); CS3_HIP(oo.alloc(m)); CS3_HIP(rr.alloc(m)); CS3_HIP(ss.alloc(4));
    if ((rc = cs3_se_baddata_dev(p, y.get(), e.get(), zz.get(), ww.get(), a.get(), b.get(), crit_tol, tt.get(), oo.get(), rr.get(), ss.get(),
                                 nullptr))) return rc;
    if ((rc = cs3_factor_status(p->h, nullptr))) return rc;
    if (t) CS3_HIP(hipMemcpy(t, tt.get(), m * 8, hipMemcpyDeviceToHost));
    if (omega) CS3_HIP(hipMemcpy(omega, oo.get(), m * 8, hipMemcpyDeviceToHost));
    if (rn) CS3_HIP(hipMemcpy(rn, rr.get(), m * 8, hipMemcpyDeviceToHost));
    CS3_HIP(hipMemcpy(summary, ss.get(), 32, hipMemcpyDeviceToHost));
    return CS3_OK;
}

}  // extern "C"
