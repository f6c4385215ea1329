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

}  // namespace

extern "C" {

int cs3_cplx_plan_create(int64_t n, const int32_t *Ap, const int32_t *Ai, int64_t batch, int64_t rotate, cs3_cplx *out)
{
    const char *who = "cs3_cplx_plan_create";
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

    cs3_cplx_s *pl = nullptr;
    try {
        pl = new cs3_cplx_s;
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
                if ((size_t) Ai[q] == j) pl->dpos.push_back(q);
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

}  // extern "C"
