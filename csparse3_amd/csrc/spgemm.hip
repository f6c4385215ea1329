// Sparse products on the device: C = A B (csc_multiply_ff, csc_numba.py:222-306) and C = A' B, as a PLAN -- the pattern
// of C and the list of products behind every entry are worked out once, the values are then refreshed as often as the
// caller likes (include/csparse3_amd.h, "sparse products").
//
// What "the same as the reference" means.  For column j of C the reference visits the products in the order
//     for pb in B(:, j):  for pa in A(:, Bi[pb]):  row Ai[pa] += Bx[pb] * Ax[pa]
// Call the position in that enumeration t.  The rows of C(:, j) are the distinct rows in order of FIRST occurrence in t
// (not sorted), and the value of a row is ((v1 + v2) + v3) + ... over its products in ascending t, the first one stored
// as it is (so (-1) * 0 stays -0.0) and every product rounded on its own (no FMA: the pragma below).
//
// Symbolic phase (once per pattern), deterministic whatever order the hardware serves atomics in:
//   1. products per column (the host counts them while it validates B) and the offset of every entry of B inside its
//      column's enumeration (k_spg_b_offsets): product t of column j is found by a binary search over those offsets.
//   2. first occurrence of every row = atomic MIN of t, keyed by row.  Columns of up to SPG_LDS_PRODUCTS products: one
//      wave, a hash table in LDS.  Wider columns: a workgroup of 256 and a table of Am words (plus Am counters) in global
//      memory per resident workgroup, cleaned through the touched entries.  (k_spg_symbolic, count mode)
//   3. distinct rows per column -> scan -> Cp.  In fill mode the same kernel walks the products in chunks, in t order:
//      a product that IS its row's minimum gets the next slot of the column (prefix count over the chunk), which is the
//      "sort by first occurrence" without a sort.
//   4. rank of a product in its row's list = the row's count from earlier chunks + the LOWER positions of this chunk
//      with the same row (a uniform compare loop over the chunk).
// Numeric phase (every call): every entry of C owns the list of its (pa, pb) pairs in ascending t and ONE lane adds them
// up in that order -- no float atomics anywhere.  Entries sit in slices of 64; inside a slice the pairs are stored
// [step][lane], so a step is one coalesced 512-byte load, and a slice is padded to its longest list with pa = -1.  An
// entry whose list has SPG_LONG or more pairs leaves its slice: one wave multiplies 64 of its products at a time and
// adds them in lane order as a serial chain, which is the same order of additions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_hipmem.hpp"

#pragma clang fp contract(off)          // v = b * a is rounded before it is added, as in the reference

namespace cs3 {

constexpr int SPG_LDS_PRODUCTS = 1024;          // most products of a column that takes the LDS hash table
constexpr int SPG_LDS_SLOTS = 2 * SPG_LDS_PRODUCTS;   // its slots: at most half full
constexpr int SPG_SLICE = 64;                   // entries of C per slice = lanes of a wave
constexpr int SPG_LONG_DEFAULT = 64;            // list length at which an entry leaves its slice (CS3_SPGEMM_LONG)
constexpr int SPG_GLOBAL_BLOCK = 256;           // workgroup of the global-table path
constexpr unsigned SPG_EMPTY = 0xffffffffu;     // table word: row not seen
constexpr unsigned SPG_SLOT = 0x80000000u;      // table word: flag | slot of the row in its column of C (t < 2^31 never matches)
constexpr long long SPG_COUNT_LIMIT = 2147483647LL - 1024;

struct SpgPattern {           // E = A, or A' with Epos = where every entry of A' sits in A's value array (null: in place)
    const int *Ep, *Ei, *Epos;
    const int *Bp, *Bi, *boff;
};

// product t of column j: the entry of B it belongs to and the entry of E
__device__ inline void spg_product(const SpgPattern &P, int j, int t, int &pa, int &pb)
{
    int lo = P.Bp[j], hi = P.Bp[j + 1] - 1;                       // the LAST pb with boff[pb] <= t (entries selecting
    while (lo < hi) {                                             //   empty columns share an offset with their successor)
        const int mid = (int) (((long long) lo + hi + 1) >> 1);
        if (P.boff[mid] <= t) lo = mid; else hi = mid - 1;
    }
    pb = lo;
    pa = P.Ep[P.Bi[pb]] + (t - P.boff[pb]);
}

// a table word as the atomics of the other waves left it (the tables of the wide columns live in global memory)
template <class T>
__device__ inline T spg_load(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256)
k_spg_b_offsets(const int *__restrict__ Ep, const int *__restrict__ Bp, const int *__restrict__ Bi, int Bn, int *__restrict__ boff)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < Bn; j += gridDim.x * blockDim.x) {
        int run = 0;
        for (int pb = Bp[j]; pb < Bp[j + 1]; ++pb) { boff[pb] = run; run += Ep[Bi[pb] + 1] - Ep[Bi[pb]]; }
    }
}

// In-place inclusive scan of ptr[1 .. n] (ptr[0] = 0 stays), one workgroup, sums carried in 64 bits (substrate.hip's k_scan)
template <class T>
__global__ void __launch_bounds__(1024)
k_spg_scan(T *ptr, long long n)
{
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long base = 1; base <= n; base += 4096) {
        const long long i0 = base + 4LL * tid;
        long long v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (i0 + q <= n) ? (long long) ptr[i0 + q] : 0;
        v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
        long long incl = v[3];
        for (int off = 1; off < 64; off <<= 1) { const long long o = __shfl_up(incl, off); if (lane >= off) incl += o; }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wv; ++w) before += wsum[w];
        const long long excl = before + incl - v[3];
#pragma unroll
        for (int q = 0; q < 4; ++q) if (i0 + q <= n) ptr[i0 + q] = (T) (excl + v[q]);
        __syncthreads();
        if (tid == 1023) carry_s = before + incl;
        __syncthreads();
    }
}

// One column of C per workgroup (steps 2 to 4 above).  HASH: one wave, tables in LDS.  Otherwise 256 threads and the
// tables ws[2 Am] of this workgroup in global memory, EMPTY / 0 on entry and on exit.
// fill = 0: count[j + 1] = distinct rows of column j.
// fill = 1: Ci, and per product g = pp[j] + t: its entry of C, its rank in that entry's list and its pair; len[entry] by
// atomic max of rank + 1 (len starts at 0).
template <int BLOCK, bool HASH>
__global__ void __launch_bounds__(BLOCK)
k_spg_symbolic(SpgPattern P, const long long *__restrict__ pp, const int *__restrict__ cols, int ncols, int fill,
               unsigned *__restrict__ ws, long long Am, int *__restrict__ Cp, int *__restrict__ Ci, int *__restrict__ len,
               int *__restrict__ ent, int *__restrict__ rnk, int2 *__restrict__ pair)
{
    constexpr int NW = BLOCK / 64;
    __shared__ int keys_s[HASH ? SPG_LDS_SLOTS : 1];
    __shared__ unsigned tmin_s[HASH ? SPG_LDS_SLOTS : 1];
    __shared__ int cnt_s[HASH ? SPG_LDS_SLOTS : 1];
    __shared__ int rows_s[BLOCK];
    __shared__ int wsum_s[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned *tmin = HASH ? tmin_s : ws + 2 * Am * (long long) blockIdx.x;
    int *cnt = HASH ? cnt_s : (int *) (tmin + Am);

    for (int c = blockIdx.x; c < ncols; c += gridDim.x) {
        const int j = cols[c];
        const long long g0 = pp[j];
        const int np = (int) (pp[j + 1] - g0);
        unsigned mask = 0, shift = 0;
        if (HASH) {
            int slots = 64, bits = 6;
            while (slots < 2 * np) { slots <<= 1; ++bits; }
            mask = (unsigned) slots - 1; shift = 32u - (unsigned) bits;
            for (int s = tid; s < slots; s += BLOCK) { keys_s[s] = -1; tmin_s[s] = SPG_EMPTY; cnt_s[s] = 0; }
            __syncthreads();
        }
        // where row r lives in the tables (HASH: linear probing; a row claims its slot on first sight, in any order)
        auto locate = [&](int r) -> int {
            if (!HASH) return r;
            unsigned h = ((unsigned) r * 0x9E3779B1u) >> shift;
            for (;;) {
                const int old = atomicCAS(&keys_s[h], -1, r);
                if (old == -1 || old == r) return (int) h;
                h = (h + 1) & mask;
            }
        };
        for (int t = tid; t < np; t += BLOCK) {
            int pa, pb;
            spg_product(P, j, t, pa, pb);
            atomicMin(&tmin[locate(P.Ei[pa])], (unsigned) t);       // a minimum: the same in any order of arrival
        }
        __syncthreads();

        int nfirst = 0;
        const int c0 = fill ? Cp[j] : 0;
        for (int t0 = 0; t0 < np; t0 += BLOCK) {
            const int t = t0 + tid;
            const bool valid = t < np;
            int pa = 0, pb = 0, r = -1, h = 0;
            if (valid) { spg_product(P, j, t, pa, pb); r = P.Ei[pa]; h = locate(r); }
            const bool first = valid && spg_load(&tmin[h]) == (unsigned) t;
            const unsigned long long m = __ballot(first);
            int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
            if (lane == 0) wsum_s[wv] = __popcll(m);
            __syncthreads();                                        // (also: every flag has been read)
            for (int w = 0; w < NW; ++w) { if (w < wv) before += wsum_s[w]; total += wsum_s[w]; }
            if (fill) {
                const int k = nfirst + before;                      // slot of a first occurrence = firsts before it in t order
                if (first) { tmin[h] = SPG_SLOT | (unsigned) k; Ci[c0 + k] = r; }
                rows_s[tid] = r;
                __syncthreads();
                int e = 0, rank = 0;
                if (valid) { e = c0 + (int) (spg_load(&tmin[h]) & ~SPG_SLOT); rank = spg_load(&cnt[h]); }
                const int nb = min(BLOCK, np - t0);
                for (int s = 0; s < nb; ++s) rank += (s < tid && rows_s[s] == r) ? 1 : 0;
                __syncthreads();                                    // the counts of the earlier chunks have been read
                if (valid) {
                    atomicAdd(&cnt[h], 1);
                    const long long g = g0 + t;
                    ent[g] = e; rnk[g] = rank;
                    pair[g] = make_int2(P.Epos ? P.Epos[pa] : pa, pb);
                    atomicMax(&len[e], rank + 1);
                }
            }
            nfirst += total;
            __syncthreads();
        }
        if (!fill && tid == 0) Cp[j + 1] = nfirst;
        if (!HASH) {                                                // leave the tables as they were found
            for (int t = tid; t < np; t += BLOCK) {
                int pa, pb;
                spg_product(P, j, t, pa, pb);
                const int r = P.Ei[pa];
                tmin[r] = SPG_EMPTY; cnt[r] = 0;
            }
            __syncthreads();
        }
    }
}

// Per slice of 64 entries: its width = the longest list that stays in it; per entry: is it long, and how long
__global__ void __launch_bounds__(256)
k_spg_slice_width(const int *__restrict__ len, long long nnz, int L, long long nslices, long long *__restrict__ sw,
                  int *__restrict__ lflag, long long *__restrict__ llen)
{
    const int lane = threadIdx.x & 63;
    for (long long s = ((long long) blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < nslices; s += ((long long) gridDim.x * blockDim.x) >> 6) {
        const long long e = s * SPG_SLICE + lane;
        const int l = e < nnz ? len[e] : 0;
        const bool is_long = l >= L;
        int w = is_long ? 0 : l;
        for (int off = 32; off > 0; off >>= 1) w = max(w, __shfl_xor(w, off));
        if (lane == 0) sw[s + 1] = w;
        if (e < nnz) { lflag[e + 1] = is_long ? 1 : 0; llen[e + 1] = is_long ? l : 0; }
    }
}

__global__ void __launch_bounds__(256)
k_spg_long_ids(const int *__restrict__ lflag, long long nnz, int *__restrict__ longs)
{
    for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long) gridDim.x * blockDim.x)
        if (lflag[e + 1] != lflag[e]) longs[lflag[e]] = (int) e;
}

// every product's pair goes to its place: [slice offset + rank][lane] or the long entry's own list
__global__ void __launch_bounds__(256)
k_spg_place(long long nprod, const int *__restrict__ ent, const int *__restrict__ rnk, const int2 *__restrict__ pair,
            const int *__restrict__ len, int L, const long long *__restrict__ sw, const long long *__restrict__ loff,
            int2 *__restrict__ spairs, int2 *__restrict__ lpairs)
{
    for (long long g = (long long) blockIdx.x * blockDim.x + threadIdx.x; g < nprod; g += (long long) gridDim.x * blockDim.x) {
        const int e = ent[g], k = rnk[g];
        if (len[e] >= L) lpairs[loff[e] + k] = pair[g];
        else spairs[(sw[e >> 6] + k) * SPG_SLICE + (e & 63)] = pair[g];
    }
}

// ---- numeric ---------------------------------------------------------------------------------------------------------
// one wave per slice, lane = entry: the lane adds its list in order.  A lane without pairs (an entry that went to the long
// path, or the tail of the last slice) writes nothing.
__global__ void __launch_bounds__(256)
k_spg_values_sliced(long long nslices, const long long *__restrict__ sw, const int2 *__restrict__ spairs,
                    const double *__restrict__ Ax, const double *__restrict__ Bx, double *__restrict__ Cx)
{
    const int lane = threadIdx.x & 63;
    for (long long s = ((long long) blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < nslices; s += ((long long) gridDim.x * blockDim.x) >> 6) {
        const long long base = sw[s] * SPG_SLICE + lane;
        const int w = (int) (sw[s + 1] - sw[s]);
        double acc = 0.0;
        bool have = false;
        for (int k = 0; k < w; ++k) {
            const int2 p = spairs[base + (long long) k * SPG_SLICE];
            if (p.x >= 0) {
                const double v = Bx[p.y] * Ax[p.x];
                acc = have ? acc + v : v;                           // the first product is stored, not added to zero
                have = true;
            }
        }
        if (have) Cx[s * SPG_SLICE + lane] = acc;
    }
}

// one wave per long entry: 64 products at a time, then added in lane order
__global__ void __launch_bounds__(256)
k_spg_values_long(int nlong, const int *__restrict__ longs, const long long *__restrict__ loff, const int2 *__restrict__ lpairs,
                  const double *__restrict__ Ax, const double *__restrict__ Bx, double *__restrict__ Cx)
{
    const int lane = threadIdx.x & 63;
    for (int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < nlong; q += (gridDim.x * blockDim.x) >> 6) {
        const int e = longs[q];
        const long long o = loff[e];
        const int n = (int) (loff[e + 1] - o);
        double acc = 0.0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            double v = 0.0;
            if (k0 + lane < n) { const int2 p = lpairs[o + k0 + lane]; v = Bx[p.y] * Ax[p.x]; }
            const int nb = min(64, n - k0);
            for (int i = 0; i < nb; ++i) {
                const double vi = __shfl(v, i);
                acc = (k0 + i) ? acc + vi : vi;
            }
        }
        if (lane == 0) Cx[e] = acc;
    }
}

static unsigned spg_blocks(long long work, int block)
{
    return (unsigned) std::max<long long>(1, std::min<long long>((work + block - 1) / block, 4096));
}

static int spg_long_threshold()
{
    const char *s = std::getenv("CS3_SPGEMM_LONG");
    if (s && *s) {
        const long v = std::strtol(s, nullptr, 10);
        if (v >= 2 && v <= (1L << 20)) return (int) v;
    }
    return SPG_LONG_DEFAULT;
}

}  // namespace cs3

using namespace cs3;

struct cs3_spgemm_s {
    int64_t Cm = 0, Cn = 0, nnz_a = 0, nnz_b = 0;
    int64_t nnz_c = 0, nprod = 0, cols_lds = 0, cols_global = 0, nslices = 0, nlong = 0, padded = 0;
    int L = SPG_LONG_DEFAULT;
    DevBuf<int> Cp, Ci, longs;
    DevBuf<long long> sw, loff;           // [nslices + 1] steps before every slice; [nnz_c + 1] pairs of long lists before every entry
    DevBuf<int2> spairs, lpairs;
};

namespace {

int spg_bad(const std::string &msg) { set_error("cs3_spgemm_plan_create: " + msg); return CS3_ERR_ARG; }

// indptr monotone from 0, indices in [0, rows)
int spg_check_pattern(const char *name, int64_t rows, int64_t n, const int32_t *p, const int32_t *idx)
{
    if (!p) return spg_bad(std::string("null indptr of ") + name);
    if (p[0] != 0) return spg_bad(std::string("indptr of ") + name + " does not start at 0");
    for (int64_t j = 0; j < n; ++j)
        if (p[j + 1] < p[j]) return spg_bad(std::string("indptr of ") + name + " decreases at column " + std::to_string(j));
    if (p[n] > 0 && !idx) return spg_bad(std::string("null indices of ") + name);
    for (int64_t q = 0; q < p[n]; ++q)
        if (idx[q] < 0 || idx[q] >= rows) return spg_bad(std::string("index of ") + name + " out of range at entry " + std::to_string(q));
    return CS3_OK;
}

int spg_run_values(const cs3_spgemm_s *pl, const double *Ax, const double *Bx, double *Cx, hipStream_t st)
{
    if (pl->nslices)
        hipLaunchKernelGGL(k_spg_values_sliced, dim3(spg_blocks(pl->nslices * 64, 256)), dim3(256), 0, st, (long long) pl->nslices,
                           pl->sw.get(), pl->spairs.get(), Ax, Bx, Cx);
    if (pl->nlong)
        hipLaunchKernelGGL(k_spg_values_long, dim3(spg_blocks(pl->nlong * 64, 256)), dim3(256), 0, st, (int) pl->nlong,
                           pl->longs.get(), pl->loff.get(), pl->lpairs.get(), Ax, Bx, Cx);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int spg_build(cs3_spgemm_s *pl, int64_t Em, int64_t En, const int32_t *Ep, const int32_t *Ei, const int32_t *Epos,
              int64_t Bn, const int32_t *Bp, const int32_t *Bi, const std::vector<long long> &pp)
{
    const long long nnz_e = Ep[En], nnz_b = Bp[Bn], nprod = pp[Bn];
    pl->nprod = nprod;
    CS3_HIP(pl->Cp.alloc((size_t) (Bn + 1)));
    CS3_HIP(hipMemset(pl->Cp.get(), 0, (size_t) (Bn + 1) * 4));
    if (nprod == 0) { CS3_HIP(pl->Ci.alloc(0)); return CS3_OK; }

    std::vector<int> cols_l, cols_g;
    for (int64_t j = 0; j < Bn; ++j) {
        const long long np = pp[j + 1] - pp[j];
        if (np > SPG_LDS_PRODUCTS) cols_g.push_back((int) j); else if (np > 0) cols_l.push_back((int) j);
    }
    pl->cols_lds = (int64_t) cols_l.size(); pl->cols_global = (int64_t) cols_g.size();

    DevBuf<int> ep, ei, epos, bp, bi, boff, dl, dg, len, ent, rnk;
    DevBuf<long long> dpp;
    DevBuf<int2> pair;
    DevBuf<unsigned> ws;
    CS3_HIP(ep.upload(Ep, (size_t) (En + 1))); CS3_HIP(ei.upload(Ei, (size_t) nnz_e));
    if (Epos) CS3_HIP(epos.upload(Epos, (size_t) nnz_e));
    CS3_HIP(bp.upload(Bp, (size_t) (Bn + 1))); CS3_HIP(bi.upload(Bi, (size_t) nnz_b));
    CS3_HIP(boff.alloc((size_t) nnz_b));
    CS3_HIP(dpp.upload(pp));
    CS3_HIP(dl.upload(cols_l)); CS3_HIP(dg.upload(cols_g));
    // the global tables: 2 Em words per workgroup, at most 64 workgroups and about 1 GiB
    unsigned gblocks = 0;
    if (!cols_g.empty()) {
        const long long per = 2 * (long long) Em * 4;
        gblocks = (unsigned) std::max<long long>(1, std::min<long long>({(long long) cols_g.size(), 64LL, (1LL << 30) / per}));
        CS3_HIP(ws.alloc((size_t) gblocks * 2 * (size_t) Em));
        CS3_HIP(hipMemset(ws.get(), 0xff, (size_t) gblocks * (size_t) per));               // EMPTY ...
        for (unsigned b = 0; b < gblocks; ++b)                                              // ... and the counters 0
            CS3_HIP(hipMemset(ws.get() + (size_t) b * 2 * (size_t) Em + (size_t) Em, 0, (size_t) Em * 4));
    }
    const SpgPattern P{ep.get(), ei.get(), Epos ? epos.get() : nullptr, bp.get(), bi.get(), boff.get()};
    hipLaunchKernelGGL(k_spg_b_offsets, dim3(spg_blocks(Bn, 256)), dim3(256), 0, 0, ep.get(), bp.get(), bi.get(), (int) Bn, boff.get());
    auto symbolic = [&](int fill) {
        if (!cols_l.empty())
            hipLaunchKernelGGL((k_spg_symbolic<64, true>), dim3(spg_blocks((long long) cols_l.size(), 1)), dim3(64), 0, 0, P, dpp.get(),
                               dl.get(), (int) cols_l.size(), fill, (unsigned *) nullptr, (long long) Em, pl->Cp.get(), pl->Ci.get(),
                               len.get(), ent.get(), rnk.get(), pair.get());
        if (!cols_g.empty())
            hipLaunchKernelGGL((k_spg_symbolic<SPG_GLOBAL_BLOCK, false>), dim3(gblocks), dim3(SPG_GLOBAL_BLOCK), 0, 0, P, dpp.get(),
                               dg.get(), (int) cols_g.size(), fill, ws.get(), (long long) Em, pl->Cp.get(), pl->Ci.get(),
                               len.get(), ent.get(), rnk.get(), pair.get());
    };
    symbolic(0);
    hipLaunchKernelGGL(k_spg_scan<int>, dim3(1), dim3(1024), 0, 0, pl->Cp.get(), (long long) Bn);
    CS3_HIP(hipGetLastError());
    int nnz_c = 0;
    CS3_HIP(hipMemcpy(&nnz_c, pl->Cp.get() + Bn, 4, hipMemcpyDeviceToHost));
    pl->nnz_c = nnz_c;
    pl->nslices = (nnz_c + SPG_SLICE - 1) / SPG_SLICE;

    CS3_HIP(pl->Ci.alloc((size_t) nnz_c));
    CS3_HIP(len.alloc((size_t) nnz_c)); CS3_HIP(hipMemset(len.get(), 0, (size_t) nnz_c * 4));
    CS3_HIP(ent.alloc((size_t) nprod)); CS3_HIP(rnk.alloc((size_t) nprod)); CS3_HIP(pair.alloc((size_t) nprod));
    symbolic(1);

    DevBuf<int> lflag;
    CS3_HIP(pl->sw.alloc((size_t) (pl->nslices + 1))); CS3_HIP(lflag.alloc((size_t) nnz_c + 1)); CS3_HIP(pl->loff.alloc((size_t) nnz_c + 1));
    CS3_HIP(hipMemset(pl->sw.get(), 0, 8)); CS3_HIP(hipMemset(lflag.get(), 0, 4)); CS3_HIP(hipMemset(pl->loff.get(), 0, 8));
    hipLaunchKernelGGL(k_spg_slice_width, dim3(spg_blocks(pl->nslices * 64, 256)), dim3(256), 0, 0, len.get(), (long long) nnz_c, pl->L,
                       (long long) pl->nslices, pl->sw.get(), lflag.get(), pl->loff.get());
    hipLaunchKernelGGL(k_spg_scan<long long>, dim3(1), dim3(1024), 0, 0, pl->sw.get(), (long long) pl->nslices);
    hipLaunchKernelGGL(k_spg_scan<int>, dim3(1), dim3(1024), 0, 0, lflag.get(), (long long) nnz_c);
    hipLaunchKernelGGL(k_spg_scan<long long>, dim3(1), dim3(1024), 0, 0, pl->loff.get(), (long long) nnz_c);
    CS3_HIP(hipGetLastError());
    long long steps = 0, long_pairs = 0;
    int nlong = 0;
    CS3_HIP(hipMemcpy(&steps, pl->sw.get() + pl->nslices, 8, hipMemcpyDeviceToHost));
    CS3_HIP(hipMemcpy(&nlong, lflag.get() + nnz_c, 4, hipMemcpyDeviceToHost));
    CS3_HIP(hipMemcpy(&long_pairs, pl->loff.get() + nnz_c, 8, hipMemcpyDeviceToHost));
    pl->nlong = nlong;
    pl->padded = steps * SPG_SLICE + long_pairs;
    if (pl->padded >= SPG_COUNT_LIMIT)
        return spg_bad("the padded lists would hold " + std::to_string(pl->padded) + " pairs (limit 2^31 - 1024)");
    CS3_HIP(pl->spairs.alloc((size_t) (steps * SPG_SLICE))); CS3_HIP(pl->lpairs.alloc((size_t) long_pairs));
    CS3_HIP(pl->longs.alloc((size_t) nlong));
    if (steps) CS3_HIP(hipMemset(pl->spairs.get(), 0xff, (size_t) (steps * SPG_SLICE) * sizeof(int2)));     // padding: pa = -1
    if (nlong) hipLaunchKernelGGL(k_spg_long_ids, dim3(spg_blocks(nnz_c, 256)), dim3(256), 0, 0, lflag.get(), (long long) nnz_c, pl->longs.get());
    hipLaunchKernelGGL(k_spg_place, dim3(spg_blocks(nprod, 256)), dim3(256), 0, 0, nprod, ent.get(), rnk.get(), pair.get(), len.get(),
                       pl->L, pl->sw.get(), pl->loff.get(), pl->spairs.get(), pl->lpairs.get());
    CS3_HIP(hipGetLastError());
    CS3_HIP(hipDeviceSynchronize());                                // the work arrays go out of scope here
    return CS3_OK;
}

}  // namespace

extern "C" {

int cs3_spgemm_limits(cs3_spgemm_limits_t *out)
{
    if (!out) { set_error("cs3_spgemm_limits: null output"); return CS3_ERR_ARG; }
    out->lds_products = SPG_LDS_PRODUCTS;
    out->lds_table_rows = SPG_LDS_PRODUCTS;
    out->long_list = spg_long_threshold();
    out->slice_width = SPG_SLICE;
    out->rank_chunk_lds = 64;
    out->rank_chunk_global = SPG_GLOBAL_BLOCK;
    return CS3_OK;
}

int cs3_spgemm_plan_create(int64_t Am, int64_t An, const int32_t *Ap, const int32_t *Ai,
                           int64_t Bm, int64_t Bn, const int32_t *Bp, const int32_t *Bi, int transpose_a, cs3_spgemm *out)
{
    if (!out) return spg_bad("null output");
    *out = nullptr;
    if (Am < 0 || An < 0 || Bm < 0 || Bn < 0) return spg_bad("negative dimension");
    if (Am > INT_MAX || An > INT_MAX || Bm > INT_MAX || Bn > INT_MAX) return spg_bad("dimension above INT_MAX");
    if ((transpose_a ? Am : An) != Bm)
        return spg_bad(std::string("inner dimensions differ: ") + (transpose_a ? "A' has " + std::to_string(Am) : "A has " + std::to_string(An)) +
                       " columns, B has " + std::to_string(Bm) + " rows");
    int rc;
    if ((rc = spg_check_pattern("A", Am, An, Ap, Ai))) return rc;
    if ((rc = spg_check_pattern("B", Bm, Bn, Bp, Bi))) return rc;

    cs3_spgemm_s *pl = nullptr;
    try {
        // E = A or A' (csc_transpose, csc_numba.py:400-436: rows of A become columns, entries in ascending column of A,
        // duplicates in storage order) with the place of every entry in A's value array
        const int64_t Em = transpose_a ? An : Am, En = transpose_a ? Am : An;
        std::vector<int32_t> Tp, Ti, Tpos;
        if (transpose_a) {
            const int64_t nnz = Ap[An];
            Tp.assign((size_t) Am + 1, 0); Ti.resize((size_t) nnz); Tpos.resize((size_t) nnz);
            for (int64_t p = 0; p < nnz; ++p) ++Tp[(size_t) Ai[p] + 1];
            for (int64_t i = 0; i < Am; ++i) Tp[(size_t) i + 1] += Tp[(size_t) i];
            std::vector<int32_t> w(Tp.begin(), Tp.end() - 1);
            for (int64_t j = 0; j < An; ++j)
                for (int32_t p = Ap[j]; p < Ap[j + 1]; ++p) { const int32_t q = w[(size_t) Ai[p]]++; Ti[(size_t) q] = (int32_t) j; Tpos[(size_t) q] = p; }
        }
        const int32_t *Ep = transpose_a ? Tp.data() : Ap, *Ei = transpose_a ? Ti.data() : Ai;
        // products before every column of C, in 64 bits
        std::vector<long long> pp((size_t) Bn + 1, 0);
        for (int64_t j = 0; j < Bn; ++j) {
            long long np = 0;
            for (int32_t pb = Bp[j]; pb < Bp[j + 1]; ++pb) np += Ep[Bi[pb] + 1] - Ep[Bi[pb]];
            pp[(size_t) j + 1] = pp[(size_t) j] + np;
            if (pp[(size_t) j + 1] >= SPG_COUNT_LIMIT)
                return spg_bad("the product needs " + std::to_string(pp[(size_t) j + 1]) + " or more multiplications (limit 2^31 - 1024)");
        }
        if (no_device("cs3_spgemm_plan_create")) return CS3_ERR_HIP;
        pl = new cs3_spgemm_s;
        pl->Cm = Em; pl->Cn = Bn; pl->nnz_a = Ap[An]; pl->nnz_b = Bp[Bn];
        pl->L = spg_long_threshold();
        rc = spg_build(pl, Em, En, Ep, Ei, transpose_a ? Tpos.data() : nullptr, Bn, Bp, Bi, pp);
    } catch (const std::bad_alloc &) {
        delete pl; set_error("cs3_spgemm_plan_create: out of memory"); return CS3_ERR_ALLOC;
    }
    if (rc) { delete pl; return rc; }
    *out = pl;
    return CS3_OK;
}

int cs3_spgemm_plan_free(cs3_spgemm plan)
{
    delete plan;
    return CS3_OK;
}

int cs3_spgemm_plan_info(cs3_spgemm plan, cs3_spgemm_info *info)
{
    if (!plan || !info) { set_error("cs3_spgemm_plan_info: null argument"); return CS3_ERR_ARG; }
    info->m = plan->Cm; info->n = plan->Cn; info->nnz_a = plan->nnz_a; info->nnz_b = plan->nnz_b;
    info->nnz_c = plan->nnz_c; info->products = plan->nprod;
    info->cols_lds = plan->cols_lds; info->cols_global = plan->cols_global;
    info->entries_sliced = plan->nnz_c - plan->nlong; info->entries_long = plan->nlong;
    info->padded_pairs = plan->padded;
    info->long_list = plan->L;
    return CS3_OK;
}

int cs3_spgemm_plan_pattern(cs3_spgemm plan, int32_t *Cp, int32_t *Ci)
{
    if (!plan || !Cp || (plan->nnz_c > 0 && !Ci)) { set_error("cs3_spgemm_plan_pattern: null argument"); return CS3_ERR_ARG; }
    CS3_HIP(hipMemcpy(Cp, plan->Cp.get(), (size_t) (plan->Cn + 1) * 4, hipMemcpyDeviceToHost));
    if (plan->nnz_c) CS3_HIP(hipMemcpy(Ci, plan->Ci.get(), (size_t) plan->nnz_c * 4, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_spgemm_plan_pattern_dev(cs3_spgemm plan, const int32_t **Cp_dev, const int32_t **Ci_dev)
{
    if (!plan) { set_error("cs3_spgemm_plan_pattern_dev: null plan"); return CS3_ERR_ARG; }
    if (Cp_dev) *Cp_dev = plan->Cp.get();
    if (Ci_dev) *Ci_dev = plan->Ci.get();
    return CS3_OK;
}

int cs3_spgemm_values_dev(cs3_spgemm plan, const double *Ax_dev, const double *Bx_dev, double *Cx_dev, void *stream)
{
    if (!plan) { set_error("cs3_spgemm_values_dev: null plan"); return CS3_ERR_ARG; }
    if (plan->nnz_c > 0 && (!Ax_dev || !Bx_dev || !Cx_dev)) { set_error("cs3_spgemm_values_dev: null value array"); return CS3_ERR_ARG; }
    return spg_run_values(plan, Ax_dev, Bx_dev, Cx_dev, (hipStream_t) stream);
}

int cs3_spgemm_values(cs3_spgemm plan, const double *Ax, const double *Bx, double *Cx)
{
    if (!plan) { set_error("cs3_spgemm_values: null plan"); return CS3_ERR_ARG; }
    if (plan->nnz_c == 0) return CS3_OK;
    if (!Ax || !Bx || !Cx) { set_error("cs3_spgemm_values: null value array"); return CS3_ERR_ARG; }
    DevBuf<double> ax, bx, cx;
    CS3_HIP(ax.upload(Ax, (size_t) plan->nnz_a)); CS3_HIP(bx.upload(Bx, (size_t) plan->nnz_b));
    CS3_HIP(cx.alloc((size_t) plan->nnz_c));
    const int rc = spg_run_values(plan, ax.get(), bx.get(), cx.get(), nullptr);
    if (rc) return rc;
    CS3_HIP(hipMemcpy(Cx, cx.get(), (size_t) plan->nnz_c * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

}  // extern "C"
