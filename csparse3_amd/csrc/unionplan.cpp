// Union plans, host side (include/csparse3_amd.h, "union plans"): the union of nmat patterns of one order, the place of
// every member entry in it and the gather map that cs3_union_values_dev reads.  No GPU is needed for anything here.
//
// Cost: O(entries of the distinct patterns + n) plus a sort of every union column.  Identical patterns are found first
// (a hash of (Ap, Ai), confirmed by comparison), so a family of T time steps x C topologies does the work of C patterns.
// A column of the union is collected with a stamp per row, as csc_add_ff collects a column of A + B, and then sorted: the
// result does not depend on the order of the members.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_union.hpp"

using namespace cs3;

namespace {

constexpr long long UNION_COUNT_LIMIT = 2147483647LL - 1024;

int un_bad(const std::string &msg) { set_error("cs3_union_plan_create: " + msg); return CS3_ERR_ARG; }

uint64_t un_hash(const int32_t *p, size_t count, uint64_t h)
{
    for (size_t i = 0; i < count; ++i) { h ^= (uint32_t) p[i]; h *= 0x100000001b3ULL; }      // FNV-1a over the words
    return h;
}

}  // namespace

extern "C" {

int cs3_union_plan_create(int64_t n, int64_t nmat, const int32_t *const *Ap, const int32_t *const *Ai, cs3_union *out)
{
    if (!out) return un_bad("null output");
    *out = nullptr;
    if (!Ap || !Ai) return un_bad("null array of pattern pointers");
    if (nmat < 1) return un_bad("nmat must be >= 1");
    if (n < 0 || n >= ((int64_t) 1 << 30)) return un_bad("bad order n");                     // (the range cs3_analyze takes)
    if (nmat > INT_MAX) return un_bad("nmat above INT_MAX");
    for (int64_t b = 0; b < nmat; ++b)
        if (!Ap[b]) return un_bad("null column pointers of member " + std::to_string(b));
    for (int64_t b = 0; b < nmat; ++b) {
        const int32_t *p = Ap[b], *idx = Ai[b];
        const std::string who = " of member " + std::to_string(b);
        if (p[0] != 0) return un_bad("Ap[0] != 0" + who);
        for (int64_t j = 0; j < n; ++j)
            if (p[j + 1] < p[j]) return un_bad("Ap" + who + " decreases at column " + std::to_string(j));
        if (p[n] > 0 && !idx) return un_bad("null row indices" + who);
        for (int64_t q = 0; q < p[n]; ++q)
            if (idx[q] < 0 || idx[q] >= n) return un_bad("row index" + who + " out of range at entry " + std::to_string(q));
    }
    for (int64_t b = 0; b < nmat; ++b)
        if (Ap[b][n] >= UNION_COUNT_LIMIT)
            return un_bad("member " + std::to_string(b) + " has " + std::to_string(Ap[b][n]) + " entries (limit 2^31 - 1024)");

    cs3_union_s *pl = nullptr;
    try {
        pl = new cs3_union_s;
        pl->n = n; pl->nmat = nmat;
        pl->off.assign((size_t) nmat + 1, 0);
        for (int64_t b = 0; b < nmat; ++b) pl->off[(size_t) b + 1] = pl->off[(size_t) b] + Ap[b][n];
        pl->nnz_total = pl->off[(size_t) nmat];

        // distinct patterns, numbered in order of first appearance
        pl->map_of.resize((size_t) nmat);
        std::vector<int64_t> rep;                                   // the first member with every distinct pattern
        std::unordered_map<uint64_t, std::vector<int32_t>> seen;   // hash -> distinct patterns with that hash
        for (int64_t b = 0; b < nmat; ++b) {
            const size_t nz = (size_t) Ap[b][n];
            std::vector<int32_t> &cands = seen[un_hash(Ai[b], nz, un_hash(Ap[b], (size_t) n + 1, 0xcbf29ce484222325ULL))];
            int32_t found = -1;
            for (int32_t d : cands) {
                const int64_t r = rep[(size_t) d];
                if (std::memcmp(Ap[r], Ap[b], ((size_t) n + 1) * 4) == 0 && (nz == 0 || std::memcmp(Ai[r], Ai[b], nz * 4) == 0)) { found = d; break; }
            }
            if (found < 0) { found = (int32_t) rep.size(); rep.push_back(b); cands.push_back(found); }
            pl->map_of[(size_t) b] = found;
        }
        const size_t nmaps = rep.size();
        pl->nmaps = (int64_t) nmaps;

        // the union, column by column, and the slot of every entry of every distinct pattern
        pl->Up.assign((size_t) n + 1, 0);
        pl->slot.resize(nmaps);
        for (size_t d = 0; d < nmaps; ++d) pl->slot[d].resize((size_t) Ap[rep[d]][n]);
        std::vector<int32_t> stamp((size_t) n, -1), pos((size_t) n, 0);
        for (int64_t j = 0; j < n; ++j) {
            const size_t c0 = pl->Ui.size();
            for (size_t d = 0; d < nmaps; ++d) {
                const int32_t *p = Ap[rep[d]], *idx = Ai[rep[d]];
                for (int32_t q = p[j]; q < p[j + 1]; ++q) {
                    const int32_t r = idx[q];
                    if (stamp[(size_t) r] != (int32_t) j) { stamp[(size_t) r] = (int32_t) j; pl->Ui.push_back(r); }
                }
            }
            if ((long long) pl->Ui.size() >= UNION_COUNT_LIMIT) {
                delete pl;
                return un_bad("the union has " + std::to_string(UNION_COUNT_LIMIT) + " or more entries (limit 2^31 - 1024)");
            }
            std::sort(pl->Ui.begin() + (std::ptrdiff_t) c0, pl->Ui.end());
            for (size_t q = c0; q < pl->Ui.size(); ++q) pos[(size_t) pl->Ui[q]] = (int32_t) q;
            for (size_t d = 0; d < nmaps; ++d) {
                const int32_t *p = Ap[rep[d]], *idx = Ai[rep[d]];
                for (int32_t q = p[j]; q < p[j + 1]; ++q) pl->slot[d][(size_t) q] = pos[(size_t) idx[q]];
            }
            pl->Up[(size_t) j + 1] = (int32_t) pl->Ui.size();
        }
        const size_t nnz_u = pl->Ui.size();
        pl->nnz_u = (int64_t) nnz_u;

        // the gather map of every distinct pattern; duplicates of a slot go to a list, in storage order
        pl->map.assign(nmaps * nnz_u, -1);
        pl->ovp.assign(1, 0);
        std::vector<int32_t> cnt(nnz_u), cursor;
        std::vector<long long> with_source(nmaps, 0), dups(nmaps, 0);
        for (size_t d = 0; d < nmaps; ++d) {
            int32_t *row = pl->map.data() + d * nnz_u;
            const std::vector<int32_t> &sl = pl->slot[d];
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int32_t s : sl) ++cnt[(size_t) s];
            for (size_t e = 0; e < sl.size(); ++e) {
                const size_t s = (size_t) sl[e];
                if (cnt[s] == 1) { row[s] = (int32_t) e; ++with_source[d]; continue; }
                if (row[s] == -1) {                                 // first sight of a duplicate slot: open its list
                    const long long q = (long long) pl->ovp.size() - 1;
                    if (q >= UNION_COUNT_LIMIT) { delete pl; return un_bad("too many duplicate slots (limit 2^31 - 1024)"); }
                    row[s] = (int32_t) (-2 - q);
                    cursor.push_back((int32_t) 0);
                    pl->ovp.push_back(pl->ovp.back() + cnt[s]);
                    pl->ovs.resize((size_t) pl->ovp.back());
                    ++with_source[d]; ++dups[d];
                }
                const size_t q = (size_t) (-2 - row[s]);
                pl->ovs[(size_t) pl->ovp[q] + (size_t) cursor[q]++] = (int32_t) e;
            }
        }
        long long sourced = 0;
        for (int64_t b = 0; b < nmat; ++b) { sourced += with_source[(size_t) pl->map_of[(size_t) b]]; pl->dup_slots += dups[(size_t) pl->map_of[(size_t) b]]; }
        pl->padded = nmat * pl->nnz_u - sourced;
    } catch (const std::bad_alloc &) {
        delete pl; set_error("cs3_union_plan_create: out of memory"); return CS3_ERR_ALLOC;
    }
    *out = pl;
    return CS3_OK;
}

int cs3_union_plan_free(cs3_union p)
{
    delete p;
    return CS3_OK;
}

int cs3_union_plan_info(cs3_union p, cs3_union_info *info)
{
    if (!p || !info) { set_error("cs3_union_plan_info: null argument"); return CS3_ERR_ARG; }
    info->n = p->n; info->nmat = p->nmat; info->nnz_union = p->nnz_u; info->nnz_total = p->nnz_total;
    info->distinct_patterns = p->nmaps; info->padded = p->padded; info->dup_slots = p->dup_slots;
    return CS3_OK;
}

int cs3_union_plan_pattern(cs3_union p, int32_t *Up, int32_t *Ui)
{
    if (!p) { set_error("cs3_union_plan_pattern: null plan"); return CS3_ERR_ARG; }
    if (Up) std::memcpy(Up, p->Up.data(), p->Up.size() * 4);
    if (Ui && p->nnz_u) std::memcpy(Ui, p->Ui.data(), (size_t) p->nnz_u * 4);
    return CS3_OK;
}

int cs3_union_plan_offsets(cs3_union p, int64_t *off)
{
    if (!p || !off) { set_error("cs3_union_plan_offsets: null argument"); return CS3_ERR_ARG; }
    for (size_t b = 0; b < p->off.size(); ++b) off[b] = p->off[b];
    return CS3_OK;
}

int cs3_union_plan_slots(cs3_union p, int64_t b, int32_t *slot)
{
    if (!p) { set_error("cs3_union_plan_slots: null plan"); return CS3_ERR_ARG; }
    if (b < 0 || b >= p->nmat) { set_error("cs3_union_plan_slots: member out of range"); return CS3_ERR_ARG; }
    const std::vector<int32_t> &sl = p->slot[(size_t) p->map_of[(size_t) b]];
    if (!sl.empty() && !slot) { set_error("cs3_union_plan_slots: null output"); return CS3_ERR_ARG; }
    if (!sl.empty()) std::memcpy(slot, sl.data(), sl.size() * 4);
    return CS3_OK;
}

}  // extern "C"
