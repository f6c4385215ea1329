// AC power flow, host side (include/csparse3_amd.h, "AC power flow"): from the pattern of a bus admittance matrix and
// the bus types, the pattern of the Newton Jacobian [[H, N], [M, L]], the place of every entry of Y in its four blocks,
// Y by rows (positions only: no transposed copy of values is ever made, the way spgemm.hip reads through recorded
// positions) and the unknown behind every bus.  The plan owns a batched LU handle on the Jacobian's pattern.  No GPU is
// needed for anything here.
//
// Cost: O(nnz_y + n) plus the analysis of the Jacobian (cs3_analyze).
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
#include "cs3_pf.hpp"

using namespace cs3;

namespace {

constexpr long long PF_COUNT_LIMIT = 2147483647LL - 1024;

int pf_bad(const std::string &msg) { set_error("cs3_pf_plan_create: " + msg); return CS3_ERR_ARG; }

}  // namespace

extern "C" {

int cs3_pf_plan_create(int64_t n, const int32_t *Yp, const int32_t *Yi, int64_t npv, const int32_t *pv, int64_t npq,
                       const int32_t *pq, int64_t batch, int64_t y_batch, int64_t order, cs3_pf *out)
{
    // 1. null pointers
    if (!out) return pf_bad("null output");
    *out = nullptr;
    if (!Yp) return pf_bad("null column pointers");
    if ((npv > 0 && !pv) || (npq > 0 && !pq)) return pf_bad("null bus list");
    // 2. the pattern, as cs3_union_plan_create checks a member
    if (n < 0 || n >= ((int64_t) 1 << 30)) return pf_bad("bad order n");
    if (Yp[0] != 0) return pf_bad("Yp[0] != 0");
    for (int64_t j = 0; j < n; ++j)
        if (Yp[j + 1] < Yp[j]) return pf_bad("Yp decreases at column " + std::to_string(j));
    const int64_t nnz = Yp[n];
    if (nnz > 0 && !Yi) return pf_bad("null row indices");
    for (int64_t q = 0; q < nnz; ++q)
        if (Yi[q] < 0 || Yi[q] >= n) return pf_bad("row index out of range at entry " + std::to_string(q));
    if (nnz >= PF_COUNT_LIMIT / 4) return pf_bad("Y has " + std::to_string(nnz) + " entries (limit 2^29 - 256: a Jacobian holds four per entry)");
    // 3. the batch
    if (batch < 1 || batch > INT_MAX) return pf_bad("batch must be >= 1");
    if (y_batch != 1 && y_batch != batch) return pf_bad("y_batch must be 1 or batch");
    if (order != CS3_ORDER_NATURAL && order != CS3_ORDER_AMD) return pf_bad("order must be 0 (natural) or 1 (AMD)");
    // 4. the bus lists
    if (npv < 0 || npq < 0 || npv > n || npq > n) return pf_bad("bad length of a bus list");

    cs3_pf_s *pl = nullptr;
    try {
        pl = new cs3_pf_s;
        pl->n = n; pl->nnz_y = nnz; pl->npv = npv; pl->npq = npq; pl->batch = batch; pl->y_batch = y_batch;
        const int64_t npvpq = npv + npq;
        pl->upos_a.assign((size_t) n, -1);
        pl->upos_m.assign((size_t) n, -1);
        for (int64_t k = 0; k < npvpq; ++k) {
            const bool is_pv = k < npv;
            const int32_t bus = is_pv ? pv[k] : pq[k - npv];
            const std::string who = std::string(is_pv ? "pv[" : "pq[") + std::to_string(is_pv ? k : k - npv) + "]";
            if (bus < 0 || bus >= n) { delete pl; return pf_bad(who + " out of range"); }
            if (pl->upos_a[(size_t) bus] >= 0) {
                const bool other = pl->upos_a[(size_t) bus] < npv && !is_pv;
                delete pl;
                return pf_bad(who + (other ? " is also in pv" : " repeats an earlier entry"));
            }
            pl->upos_a[(size_t) bus] = (int32_t) k;
            if (!is_pv) pl->upos_m[(size_t) bus] = (int32_t) (npvpq + (k - npv));
        }
        // 5. something to solve for
        if (npvpq == 0) { delete pl; return pf_bad("npv + npq = 0: every bus is a reference bus"); }
        pl->nref = n - npvpq;
        pl->nj = npv + 2 * npq;
        pl->ubus.resize((size_t) pl->nj);
        for (int64_t k = 0; k < npv; ++k) pl->ubus[(size_t) k] = pv[k];
        for (int64_t k = 0; k < npq; ++k) pl->ubus[(size_t) (npv + k)] = pl->ubus[(size_t) (npvpq + k)] = pq[k];

        // 6. a row stored twice in a column; rows and columns of the entries, the stored diagonals
        pl->yrow.assign(Yi, Yi + nnz);
        pl->ycol.resize((size_t) nnz);
        std::vector<int32_t> stamp((size_t) n, -1);
        std::vector<char> has_diag((size_t) n, 0);
        for (int64_t j = 0; j < n; ++j)
            for (int32_t q = Yp[j]; q < Yp[j + 1]; ++q) {
                const int32_t i = Yi[q];
                if (stamp[(size_t) i] == (int32_t) j) {
                    delete pl;
                    return pf_bad("row " + std::to_string(i) + " is stored twice in column " + std::to_string(j));
                }
                stamp[(size_t) i] = (int32_t) j;
                pl->ycol[(size_t) q] = (int32_t) j;
                if (i == j) has_diag[(size_t) j] = 1;
            }
        // 7. the diagonal of every bus that has an unknown
        for (int64_t k = 0; k < npvpq; ++k) {
            const int32_t bus = pl->ubus[(size_t) k];
            if (!has_diag[(size_t) bus]) {
                delete pl;
                return pf_bad(std::string(k < npv ? "pv" : "pq") + " bus " + std::to_string(bus) + " has no stored diagonal entry");
            }
        }

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
            if (pl->upos_a[(size_t) i] < 0) continue;                  // a reference row is never summed
            const int64_t d = pl->Rp[(size_t) i + 1] - pl->Rp[(size_t) i];
            pl->max_row = std::max(pl->max_row, d);
            if (d > PF_WAVE_ROW) { pl->wave_rows.push_back((int32_t) i); ++pl->rows_wave; } else ++pl->rows_lane;
        }

        // the Jacobian: column c comes from column ubus[c] of Y: the top block's entries in storage order, then the bottom's
        pl->Jp.assign((size_t) pl->nj + 1, 0);
        pl->jpos.assign(4 * (size_t) nnz, -1);
        for (int64_t c = 0; c < pl->nj; ++c) {
            const int32_t j = pl->ubus[(size_t) c];
            const bool right = c >= npvpq;                              // the columns of N and L
            int32_t *top = pl->jpos.data() + (right ? 1 : 0) * (size_t) nnz, *bot = pl->jpos.data() + (right ? 3 : 2) * (size_t) nnz;
            for (int32_t q = Yp[j]; q < Yp[j + 1]; ++q)
                if (pl->upos_a[(size_t) Yi[q]] >= 0) { top[q] = (int32_t) pl->Ji.size(); pl->Ji.push_back(pl->upos_a[(size_t) Yi[q]]); }
            for (int32_t q = Yp[j]; q < Yp[j + 1]; ++q)
                if (pl->upos_m[(size_t) Yi[q]] >= 0) { bot[q] = (int32_t) pl->Ji.size(); pl->Ji.push_back(pl->upos_m[(size_t) Yi[q]]); }
            pl->Jp[(size_t) c + 1] = (int32_t) pl->Ji.size();
        }
        pl->nnz_j = (int64_t) pl->Ji.size();
    } catch (const std::bad_alloc &) {
        delete pl; set_error("cs3_pf_plan_create: out of memory"); return CS3_ERR_ALLOC;
    }
    const int rc = cs3_analyze(CS3_LU, order, pl->nj, pl->Jp.data(), pl->Ji.data(), nullptr, batch, &pl->h);
    if (rc) { delete pl; return rc; }
    *out = pl;
    return CS3_OK;
}

int cs3_pf_plan_free(cs3_pf p)
{
    if (!p) return CS3_OK;
    cs3_free(p->h);
    delete p;
    return CS3_OK;
}

int cs3_pf_handle(cs3_pf p, cs3_handle *h)
{
    if (!p || !h) { set_error("cs3_pf_handle: null argument"); return CS3_ERR_ARG; }
    *h = p->h;
    return CS3_OK;
}

int cs3_pf_plan_info(cs3_pf p, cs3_pf_info *info)
{
    if (!p || !info) { set_error("cs3_pf_plan_info: null argument"); return CS3_ERR_ARG; }
    info->n = p->n; info->nnz_y = p->nnz_y; info->npv = p->npv; info->npq = p->npq; info->nref = p->nref;
    info->nj = p->nj; info->nnz_j = p->nnz_j; info->batch = p->batch; info->y_batch = p->y_batch;
    info->rows_lane = p->rows_lane; info->rows_wave = p->rows_wave; info->max_row = p->max_row;
    return CS3_OK;
}

int cs3_pf_plan_pattern(cs3_pf p, int32_t *Jp, int32_t *Ji)
{
    if (!p) { set_error("cs3_pf_plan_pattern: null plan"); return CS3_ERR_ARG; }
    if (Jp) std::memcpy(Jp, p->Jp.data(), p->Jp.size() * 4);
    if (Ji && p->nnz_j) std::memcpy(Ji, p->Ji.data(), (size_t) p->nnz_j * 4);
    return CS3_OK;
}

int cs3_pf_plan_maps(cs3_pf p, int32_t *jpos, int32_t *Rp, int32_t *Rj, int32_t *Rpos, int32_t *upos_a, int32_t *upos_m)
{
    if (!p) { set_error("cs3_pf_plan_maps: null plan"); return CS3_ERR_ARG; }
    const size_t nnz = (size_t) p->nnz_y, n = (size_t) p->n;
    if (jpos && nnz) std::memcpy(jpos, p->jpos.data(), 4 * nnz * 4);
    if (Rp) std::memcpy(Rp, p->Rp.data(), (n + 1) * 4);
    if (Rj && nnz) std::memcpy(Rj, p->Rj.data(), nnz * 4);
    if (Rpos && nnz) std::memcpy(Rpos, p->Rpos.data(), nnz * 4);
    if (upos_a && n) std::memcpy(upos_a, p->upos_a.data(), n * 4);
    if (upos_m && n) std::memcpy(upos_m, p->upos_m.data(), n * 4);
    return CS3_OK;
}

int cs3_pf_limits(cs3_pf_limits_t *out)
{
    if (!out) { set_error("cs3_pf_limits: null output"); return CS3_ERR_ARG; }
    out->block = PF_BLOCK;
    out->grid_cap = PF_GRID_CAP;
    out->wave_row = PF_WAVE_ROW;
    return CS3_OK;
}

}  // extern "C"

// ---- the numeric phase: entry points around the launches of powerflow.hip, and the Newton driver -----------------------
namespace {

int pf_ensure_work(cs3_pf_s *p)
{
    if (int rc = pf_upload(p)) return rc;
    auto &m = p->mem;
    const size_t batch = (size_t) p->batch;
    CS3_HIP(m.rhs.reserve(batch * (size_t) p->nj));
    CS3_HIP(m.jx.reserve(batch * (size_t) p->nnz_j));
    CS3_HIP(m.norm.reserve(batch));
    CS3_HIP(m.nbits.reserve(batch));
    CS3_HIP(m.ints.reserve(3 * batch + 1));
    return CS3_OK;
}

// Uploads `count` doubles for a host-array form.
int pf_stage(DevBuf<double> &d, const double *src, size_t count) { CS3_HIP(d.upload(src, count)); return CS3_OK; }

}  // namespace

extern "C" {

int cs3_pf_mismatch_dev(cs3_pf p, const double *Yz_dev, const double *S_dev, const double *vm_dev, const double *va_dev,
                        double *F_dev, double *norm_dev, void *stream)
{
    if (!p || !Yz_dev || !S_dev || !vm_dev || !va_dev || !F_dev) { set_error("cs3_pf_mismatch_dev: null argument"); return CS3_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(norm_dev) & 7) { set_error("cs3_pf_mismatch_dev: norm not aligned to 8 bytes"); return CS3_ERR_ARG; }
    if (int rc = pf_upload(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    if (norm_dev) CS3_HIP(hipMemsetAsync(norm_dev, 0, (size_t) p->batch * 8, st));           // +0.0: the maximum starts there
    return pf_launch_mismatch(p, Yz_dev, S_dev, vm_dev, va_dev, nullptr, F_dev, reinterpret_cast<unsigned long long *>(norm_dev), st);
}

int cs3_pf_jacobian_dev(cs3_pf p, const double *Yz_dev, const double *vm_dev, const double *va_dev, double *Jx_dev, void *stream)
{
    if (!p || !Yz_dev || !vm_dev || !va_dev || !Jx_dev) { set_error("cs3_pf_jacobian_dev: null argument"); return CS3_ERR_ARG; }
    if (int rc = pf_upload(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    if (int rc = pf_launch_mismatch(p, Yz_dev, nullptr, vm_dev, va_dev, nullptr, nullptr, nullptr, st)) return rc;      // the currents
    return pf_launch_jacobian(p, Yz_dev, vm_dev, va_dev, nullptr, Jx_dev, st);
}

int cs3_pf_solve_dev(cs3_pf p, const double *Yz_dev, const double *S_dev, double *vm_dev, double *va_dev, double tol,
                     int64_t max_iters, int64_t refactor_every, double pivot_tol, int32_t *iters, double *norm, int32_t *flag,
                     void *stream)
{
    if (!p || !Yz_dev || !S_dev || !vm_dev || !va_dev) { set_error("cs3_pf_solve_dev: null argument"); return CS3_ERR_ARG; }
    if (!(tol >= 0.0) || !std::isfinite(tol)) { set_error("cs3_pf_solve_dev: tol must be finite and >= 0"); return CS3_ERR_ARG; }
    if (max_iters < 0 || max_iters > INT_MAX) { set_error("cs3_pf_solve_dev: max_iters must be >= 0"); return CS3_ERR_ARG; }
    if (refactor_every < 1) { set_error("cs3_pf_solve_dev: refactor_every must be >= 1"); return CS3_ERR_ARG; }
    if (int rc = pf_ensure_work(p)) return rc;
    hipStream_t st = (hipStream_t) stream;
    auto &m = p->mem;
    const size_t batch = (size_t) p->batch;
    int *state = m.ints.get();
    if (int rc = pf_launch_init(p, st)) return rc;
    bool factor_pending = false;                // a factorisation of this call whose status word has not been read yet
    for (int64_t it = 0;; ++it) {
        if (int rc = pf_launch_mismatch(p, Yz_dev, S_dev, vm_dev, va_dev, state, m.rhs.get(), m.nbits.get(), st)) return rc;
        if (int rc = pf_launch_decide(p, (int) it, (int) max_iters, tol, st)) return rc;
        // the one host read of an iteration: scenarios still active, and the status of the factorisation before it
        int active = 0, status[4] = {0x7f7f7f7f, 0, 0, 0};
        CS3_HIP(hipMemcpyAsync(&active, state + 3 * batch, sizeof(int), hipMemcpyDeviceToHost, st));
        if (factor_pending) CS3_HIP(hipMemcpyAsync(status, p->h->D.status, sizeof(status), hipMemcpyDeviceToHost, st));
        CS3_HIP(hipStreamSynchronize(st));
        if (status[0] != 0x7f7f7f7f || status[3] != 0) return cs3_factor_status(p->h, stream);    // (k_pf_update moved nothing)
        factor_pending = false;
        if (active == 0) break;
        if (it % refactor_every == 0) {
            if (int rc = pf_launch_jacobian(p, Yz_dev, vm_dev, va_dev, state, m.jx.get(), st)) return rc;
            if (int rc = cs3_factor_solve_dev(p->h, m.jx.get(), pivot_tol, m.rhs.get(), 1, stream)) return rc;
            factor_pending = true;
        } else {
            if (int rc = cs3_solve_dev(p->h, m.rhs.get(), 1, stream)) return rc;
        }
        if (int rc = pf_launch_update(p, vm_dev, va_dev, p->h->D.status, st)) return rc;
    }
    if (iters || flag) {
        std::vector<int32_t> host(3 * batch);
        CS3_HIP(hipMemcpyAsync(host.data(), state, host.size() * 4, hipMemcpyDeviceToHost, st));
        CS3_HIP(hipStreamSynchronize(st));
        if (iters) std::memcpy(iters, host.data() + batch, batch * 4);
        if (flag) std::memcpy(flag, host.data() + 2 * batch, batch * 4);
    }
    if (norm) {
        CS3_HIP(hipMemcpyAsync(norm, m.norm.get(), batch * 8, hipMemcpyDeviceToHost, st));
        CS3_HIP(hipStreamSynchronize(st));
    }
    return CS3_OK;
}

int cs3_pf_mismatch(cs3_pf p, const double *Yz, const double *S, const double *vm, const double *va, double *F, double *norm)
{
    if (!p || !Yz || !S || !vm || !va || !F) { set_error("cs3_pf_mismatch: null argument"); return CS3_ERR_ARG; }
    if (int rc = pf_upload(p)) return rc;
    const size_t batch = (size_t) p->batch, n = (size_t) p->n;
    DevBuf<double> y, s, m, a, f, nr;
    int rc;
    if ((rc = pf_stage(y, Yz, (size_t) p->y_batch * (size_t) p->nnz_y * 2)) || (rc = pf_stage(s, S, batch * n * 2)) ||
        (rc = pf_stage(m, vm, batch * n)) || (rc = pf_stage(a, va, batch * n))) return rc;
    CS3_HIP(f.alloc(batch * (size_t) p->nj));
    CS3_HIP(nr.alloc(batch));
    if ((rc = cs3_pf_mismatch_dev(p, y.get(), s.get(), m.get(), a.get(), f.get(), nr.get(), nullptr))) return rc;
    CS3_HIP(hipMemcpy(F, f.get(), batch * (size_t) p->nj * 8, hipMemcpyDeviceToHost));
    if (norm) CS3_HIP(hipMemcpy(norm, nr.get(), batch * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_pf_jacobian(cs3_pf p, const double *Yz, const double *vm, const double *va, double *Jx)
{
    if (!p || !Yz || !vm || !va || !Jx) { set_error("cs3_pf_jacobian: null argument"); return CS3_ERR_ARG; }
    if (int rc = pf_upload(p)) return rc;
    const size_t batch = (size_t) p->batch, n = (size_t) p->n;
    DevBuf<double> y, m, a, j;
    int rc;
    if ((rc = pf_stage(y, Yz, (size_t) p->y_batch * (size_t) p->nnz_y * 2)) || (rc = pf_stage(m, vm, batch * n)) ||
        (rc = pf_stage(a, va, batch * n))) return rc;
    CS3_HIP(j.alloc(batch * (size_t) p->nnz_j));
    if ((rc = cs3_pf_jacobian_dev(p, y.get(), m.get(), a.get(), j.get(), nullptr))) return rc;
    CS3_HIP(hipMemcpy(Jx, j.get(), batch * (size_t) p->nnz_j * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_pf_solve(cs3_pf p, const double *Yz, const double *S, double *vm, double *va, double tol, int64_t max_iters,
                 int64_t refactor_every, double pivot_tol, int32_t *iters, double *norm, int32_t *flag)
{
    if (!p || !Yz || !S || !vm || !va) { set_error("cs3_pf_solve: null argument"); return CS3_ERR_ARG; }
    if (!(tol >= 0.0) || !std::isfinite(tol)) { set_error("cs3_pf_solve: tol must be finite and >= 0"); return CS3_ERR_ARG; }
    if (max_iters < 0 || max_iters > INT_MAX) { set_error("cs3_pf_solve: max_iters must be >= 0"); return CS3_ERR_ARG; }
    if (refactor_every < 1) { set_error("cs3_pf_solve: refactor_every must be >= 1"); return CS3_ERR_ARG; }
    if (int rc = pf_upload(p)) return rc;
    const size_t batch = (size_t) p->batch, n = (size_t) p->n;
    DevBuf<double> y, s, m, a;
    int rc;
    if ((rc = pf_stage(y, Yz, (size_t) p->y_batch * (size_t) p->nnz_y * 2)) || (rc = pf_stage(s, S, batch * n * 2)) ||
        (rc = pf_stage(m, vm, batch * n)) || (rc = pf_stage(a, va, batch * n))) return rc;
    rc = cs3_pf_solve_dev(p, y.get(), s.get(), m.get(), a.get(), tol, max_iters, refactor_every, pivot_tol, iters, norm, flag, nullptr);
    if (rc && rc != CS3_ERR_PIVOT) return rc;
    CS3_HIP(hipMemcpy(vm, m.get(), batch * n * 8, hipMemcpyDeviceToHost));       // (after a rejected pivot: the last completed update)
    CS3_HIP(hipMemcpy(va, a.get(), batch * n * 8, hipMemcpyDeviceToHost));
    return rc;
}

}  // extern "C"
