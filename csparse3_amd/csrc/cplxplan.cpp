// Complex plans, host side (include/csparse3_amd.h, "complex matrices"): the real-equivalent pattern of a complex CSC
// pattern, the doubled fill-reducing order, and the two tables the kernels of cplxplan.hip read -- where the diagonal of
// every column is stored, and the entries of every row.  No GPU is needed for anything here.
//
// The real pattern needs no map: column j of the complex pattern, with len_j entries from Ap[j], becomes the real columns
// 2j and 2j + 1, both with 2 len_j entries, at Rp[2j] = 4 Ap[j] and Rp[2j + 1] = 4 Ap[j] + 2 len_j.  Entry t of the column
// (row i) owns the positions Rp[2j] + 2t, + 1 (rows 2i, 2i + 1: Re w, Im w) and Rp[2j + 1] + 2t, + 1 (rows 2i, 2i + 1:
// -Im w, Re w).  Cost: O(nnz + n).
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_cplx.hpp"

using namespace cs3;

namespace {

constexpr long long CPLX_COUNT_LIMIT = 2147483647LL - 1024;

int cx_bad(const char *who, const std::string &msg) { set_error(std::string(who) + ": " + msg); return CS3_ERR_ARG; }

// cs3_cplx_plan_create, and with `border` cs3_cplx_plan_create_schur: the border rows get no diagonal list, so the
// rotation kernel leaves their s at (1, +0) whatever the values.
int cx_create(const char *who, int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, bool border,
              int64_t ns, const int32_t *schur_idx, cs3_cplx *out)
{
    if (!out) return cx_bad(who, "null output");
    *out = nullptr;
    if (batch < 1) return cx_bad(who, "batch must be >= 1");
    if (rotate != CS3_CPLX_ROTATE_NONE && rotate != CS3_CPLX_ROTATE_DIAG) return cx_bad(who, "rotate must be 0 (none) or 1 (diagonal)");
    if (n < 0 || n >= ((int64_t) 1 << 29)) return cx_bad(who, "bad order n (2 n must stay in the range cs3_analyze takes)");
    if (!Ap) return cx_bad(who, "null column pointers");
    if (Ap[0] != 0) return cx_bad(who, "Ap[0] != 0");
    for (int64_t j = 0; j < n; ++j)
        if (Ap[j + 1] < Ap[j]) return cx_bad(who, "Ap decreases at column " + std::to_string(j));
    if (Ap[n] > 0 && !Ai) return cx_bad(who, "null row indices");
    for (int64_t q = 0; q < Ap[n]; ++q)
        if (Ai[q] < 0 || Ai[q] >= n) return cx_bad(who, "row index out of range at entry " + std::to_string(q));
    if (4LL * Ap[n] >= CPLX_COUNT_LIMIT)
        return cx_bad(who, "the real form has " + std::to_string(4LL * Ap[n]) + " entries (limit 2^31 - 1024)");
    if (border) {                                                   // the checks of cs3_analyze_schur on its set, in its order
        if (!schur_idx) return cx_bad(who, "null Schur index list");
        if (ns < 1 || ns >= n)
            return cx_bad(who, "the Schur set must hold at least 1 and fewer than n variables, got ns = " + std::to_string(ns));
        for (int64_t i = 0; i < ns; ++i)
            if (schur_idx[i] < 0 || schur_idx[i] >= n)
                return cx_bad(who, "Schur index " + std::to_string(schur_idx[i]) + " (entry " + std::to_string(i) + ") is outside [0, n)");
    }

    cs3_cplx_s *pl = nullptr;
    try {
        pl = new cs3_cplx_s;
        std::vector<char> is_border((size_t) n, 0);
        for (int64_t i = 0; border && i < ns; ++i) {
            const int32_t v = schur_idx[i];
            if (is_border[(size_t) v]) {
                delete pl;
                return cx_bad(who, "Schur index " + std::to_string(v) + " (entry " + std::to_string(i) + ") is repeated");
            }
            is_border[(size_t) v] = 1;
            pl->schur_idx.push_back(v);
        }
        const size_t nn = (size_t) n, nz = (size_t) Ap[n];
        pl->n = n; pl->nnz = (int64_t) nz; pl->batch = batch; pl->rotate = rotate;
        pl->Ap.assign(Ap, Ap + nn + 1);
        pl->Ai.assign(Ai, Ai + nz);
        pl->ecol.resize(nz);
        pl->dptr.assign(nn + 1, 0);
        pl->rptr.assign(nn + 1, 0);
        pl->rpos.resize(nz);
        for (size_t j = 0; j < nn; ++j) {
            for (int32_t q = Ap[j]; q < Ap[j + 1]; ++q) {
                pl->ecol[(size_t) q] = (int32_t) j;
                ++pl->rptr[(size_t) Ai[q] + 1];
                if ((size_t) Ai[q] == j && !is_border[j]) pl->dpos.push_back(q);
            }
            pl->dptr[j + 1] = (int32_t) pl->dpos.size();
            if (pl->dptr[j + 1] == pl->dptr[j]) ++pl->rows_without_diagonal;
        }
        for (size_t i = 0; i < nn; ++i) pl->rptr[i + 1] += pl->rptr[i];
        std::vector<int32_t> cursor(pl->rptr.begin(), pl->rptr.end() - 1);
        for (size_t q = 0; q < nz; ++q) pl->rpos[(size_t) cursor[(size_t) Ai[q]]++] = (int32_t) q;   // ascending q: column, then storage order
    } catch (const std::bad_alloc &) {
        delete pl; set_error(std::string(who) + ": out of memory"); return CS3_ERR_ALLOC;
    }
    *out = pl;
    return CS3_OK;
}

}  // namespace

extern "C" {

int cs3_cplx_plan_create(int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, cs3_cplx *out)
{
    return cx_create("cs3_cplx_plan_create", n, Ap, Ai, batch, rotate, false, 0, nullptr, out);
}

int cs3_cplx_plan_create_schur(int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, int64_t ns,
                               const int32_t *schur_idx, cs3_cplx *out)
{
    return cx_create("cs3_cplx_plan_create_schur", n, Ap, Ai, batch, rotate, true, ns, schur_idx, out);
}

int cs3_cplx_plan_schur_info(cs3_cplx p, int64_t *ns, int32_t *schur_idx)
{
    const char *who = "cs3_cplx_plan_schur_info";
    if (!p) return cx_bad(who, "null plan");
    if (p->schur_idx.empty()) { set_error(std::string(who) + ": the plan has no border (cs3_cplx_plan_create_schur)"); return CS3_ERR_STATE; }
    if (ns) *ns = (int64_t) p->schur_idx.size();
    if (schur_idx) std::memcpy(schur_idx, p->schur_idx.data(), p->schur_idx.size() * sizeof(int32_t));
    return CS3_OK;
}

int cs3_cplx_plan_free(cs3_cplx p)
{
    delete p;
    return CS3_OK;
}

int cs3_cplx_plan_info(cs3_cplx p, cs3_cplx_info *info)
{
    if (!p || !info) return cx_bad("cs3_cplx_plan_info", "null argument");
    info->n = p->n; info->nnz = p->nnz; info->batch = p->batch; info->rotate = p->rotate;
    info->n_real = 2 * p->n; info->nnz_real = 4 * p->nnz; info->rows_without_diagonal = p->rows_without_diagonal;
    return CS3_OK;
}

int cs3_cplx_plan_pattern(cs3_cplx p, int32_t *Rp, int32_t *Ri)
{
    if (!p) return cx_bad("cs3_cplx_plan_pattern", "null plan");
    const int32_t *Ap = p->Ap.data(), *Ai = p->Ai.data();
    if (Rp) {
        for (int64_t j = 0; j < p->n; ++j) { Rp[2 * j] = 4 * Ap[j]; Rp[2 * j + 1] = 2 * Ap[j] + 2 * Ap[j + 1]; }
        Rp[2 * p->n] = 4 * Ap[p->n];
    }
    if (Ri)
        for (int64_t j = 0; j < p->n; ++j)
            for (int32_t q = Ap[j]; q < Ap[j + 1]; ++q) {
                const int64_t lo = 2LL * Ap[j] + 2LL * q, hi = 2LL * Ap[j + 1] + 2LL * q;       // Rp[2j] + 2t, Rp[2j + 1] + 2t
                Ri[lo] = Ri[hi] = 2 * Ai[q];
                Ri[lo + 1] = Ri[hi + 1] = 2 * Ai[q] + 1;
            }
    return CS3_OK;
}

int cs3_cplx_plan_order(cs3_cplx p, int64_t order, const int32_t *q_given, int32_t *q2)
{
    const char *who = "cs3_cplx_plan_order";
    if (!p || !q2) return cx_bad(who, "null argument");
    if (order != CS3_ORDER_NATURAL && order != CS3_ORDER_AMD && order != CS3_ORDER_GIVEN) return cx_bad(who, "order must be 0, 1 or 2");
    if (p->n == 0) return CS3_OK;
    std::vector<int32_t> q;
    try {
        q.resize((size_t) p->n);
        if (order == CS3_ORDER_GIVEN) {
            if (p->n > 0 && !q_given) return cx_bad(who, "CS3_ORDER_GIVEN without q_given");
            std::vector<char> seen((size_t) p->n, 0);
            for (int64_t t = 0; t < p->n; ++t) {
                const int32_t v = q_given[t];
                if (v < 0 || v >= p->n || seen[(size_t) v]) return cx_bad(who, "q_given is not a permutation of 0 .. n - 1");
                seen[(size_t) v] = 1;
                q[(size_t) t] = v;
            }
        } else {
            const int rc = cs3_amd(order, p->n, p->n, p->Ap.data(), p->Ai.data(), q.data());
            if (rc) return rc;
        }
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of memory"); return CS3_ERR_ALLOC;
    }
    for (int64_t t = 0; t < p->n; ++t) { q2[2 * t] = 2 * q[(size_t) t]; q2[2 * t + 1] = 2 * q[(size_t) t] + 1; }
    return CS3_OK;
}

int cs3_cplx_plan_schur_order(cs3_cplx p, int64_t order, const int32_t *q_given, int32_t *q2_interior, int32_t *schur2)
{
    const char *who = "cs3_cplx_plan_schur_order";
    if (!p || !q2_interior || !schur2) return cx_bad(who, "null argument");
    if (p->schur_idx.empty()) { set_error(std::string(who) + ": the plan has no border (cs3_cplx_plan_create_schur)"); return CS3_ERR_STATE; }
    if (order != CS3_ORDER_NATURAL && order != CS3_ORDER_AMD && order != CS3_ORDER_GIVEN) return cx_bad(who, "order must be 0, 1 or 2");
    const int64_t n = p->n, ns = (int64_t) p->schur_idx.size(), n1 = n - ns;
    std::vector<int32_t> q;
    try {
        std::vector<int32_t> inner((size_t) n, -1), interior;       // index inside A11, -1 on the border; and back
        std::vector<char> is_border((size_t) n, 0);
        for (int32_t v : p->schur_idx) is_border[(size_t) v] = 1;
        for (int64_t i = 0; i < n; ++i)
            if (!is_border[(size_t) i]) { inner[(size_t) i] = (int32_t) interior.size(); interior.push_back((int32_t) i); }
        q.resize((size_t) n1);
        if (order == CS3_ORDER_GIVEN) {
            if (!q_given) return cx_bad(who, "CS3_ORDER_GIVEN without q_given");
            std::vector<char> seen((size_t) n, 0);
            for (int64_t t = 0; t < n1; ++t) {
                const int32_t v = q_given[t];
                if (v < 0 || v >= n || is_border[(size_t) v] || seen[(size_t) v])
                    return cx_bad(who, "q_given is not a permutation of the interior (the variables outside the Schur set)");
                seen[(size_t) v] = 1;
                q[(size_t) t] = v;
            }
        } else if (order == CS3_ORDER_NATURAL) {
            q = interior;
        } else {
            // A11: border rows and columns removed, entries in A's order -- what cs3_analyze_schur orders
            std::vector<int32_t> Bp((size_t) n1 + 1, 0), Bi, q1((size_t) n1);
            for (int64_t t = 0; t < n1; ++t) {
                const int32_t j = interior[(size_t) t];
                for (int32_t e = p->Ap[(size_t) j]; e < p->Ap[(size_t) j + 1]; ++e)
                    if (!is_border[(size_t) p->Ai[(size_t) e]]) Bi.push_back(inner[(size_t) p->Ai[(size_t) e]]);
                Bp[(size_t) t + 1] = (int32_t) Bi.size();
            }
            const int rc = cs3_amd(order, n1, n1, Bp.data(), Bi.data(), q1.data());
            if (rc) return rc;
            for (int64_t t = 0; t < n1; ++t) q[(size_t) t] = interior[(size_t) q1[(size_t) t]];
        }
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of memory"); return CS3_ERR_ALLOC;
    }
    for (int64_t t = 0; t < n1; ++t) { q2_interior[2 * t] = 2 * q[(size_t) t]; q2_interior[2 * t + 1] = 2 * q[(size_t) t] + 1; }
    for (int64_t i = 0; i < ns; ++i) { schur2[2 * i] = 2 * p->schur_idx[(size_t) i]; schur2[2 * i + 1] = 2 * p->schur_idx[(size_t) i] + 1; }
    return CS3_OK;
}

}  // extern "C"
