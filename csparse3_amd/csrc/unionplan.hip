// Union plans, numeric phase (include/csparse3_amd.h, "union plans"): the ragged value arrays of nmat matrices go to the
// [nmat][nnz_union] layout that a batched handle on the union pattern reads.  ONE launch, in gather form: every output
// entry is written exactly once by the lane that owns it -- no memset, no atomics, nothing allocated, nothing waited for.
//
// Output entry (b, e), with s = map[map_of[b]][e] (unionplan.cpp builds the tables):
//   s >= 0    the bits of Ax_cat[off[b] + s]                    (moved as a 64-bit word: -0.0, NaN payloads survive)
//   s == -1   +0.0
//   s <= -2   ((v1 + v2) + v3) + ... over list -2 - s, storage order, starting from v1 as stored
//
// Shape: grid-stride over the flat index b * nnz_union + e (64 bits), one entry per lane: (b, e) come from one division
// per lane, then advance by the precomputed quotient and remainder of the grid's stride.  Map loads and value stores are
// coalesced; the value loads of a member whose rows are sorted ascend with e.  Two entries per lane (8-byte map load,
// 16-byte store) were measured beside this and were not faster ("Union plans").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_union.hpp"

namespace cs3 {

constexpr int UNION_BLOCK = 256;
constexpr int UNION_GRID_CAP = 4096;
constexpr int UNION_PER_LANE = 1;

struct UnionTables {
    const int *map, *map_of, *ovs;
    const long long *off, *ovp;
};

using u64 = unsigned long long;

// the value behind source word s of a member whose values start at ax
__device__ inline u64 union_value(const UnionTables &T, const double *__restrict__ ax, int s)
{
    if (s >= 0) return reinterpret_cast<const u64 *>(ax)[s];
    if (s == -1) return 0ull;
    const long long q = -2 - (long long) s;
    const long long p0 = T.ovp[q], p1 = T.ovp[q + 1];
    double acc = ax[T.ovs[p0]];
    for (long long p = p0 + 1; p < p1; ++p) acc += ax[T.ovs[p]];
    return (u64) __double_as_longlong(acc);
}

__global__ void __launch_bounds__(UNION_BLOCK)
k_union_values(UnionTables T, long long nnz_u, long long total, long long step_b, long long step_e,
               const double *__restrict__ Ax, u64 *__restrict__ out)
{
    long long i = (long long) blockIdx.x * UNION_BLOCK + threadIdx.x;
    if (i >= total) return;
    const long long step = (long long) gridDim.x * UNION_BLOCK;
    long long b = i / nnz_u, e = i - b * nnz_u;
    for (; i < total; i += step) {
        out[i] = union_value(T, Ax + T.off[b], T.map[(long long) T.map_of[b] * nnz_u + e]);
        b += step_b; e += step_e;                                   // step_e < nnz_u: one carry at most
        if (e >= nnz_u) { e -= nnz_u; ++b; }
    }
}

}  // namespace cs3

using namespace cs3;

namespace {

int union_launch(cs3_union_s *p, const double *Ax, double *out, hipStream_t st)
{
    const long long total = (long long) p->nmat * p->nnz_u;
    if (total == 0) return CS3_OK;
    const unsigned blocks = (unsigned) std::min<long long>((total + UNION_BLOCK - 1) / UNION_BLOCK, UNION_GRID_CAP);
    const long long step = (long long) blocks * UNION_BLOCK;
    const UnionTables T{p->d_map.get(), p->d_map_of.get(), p->d_ovs.get(), p->d_off.get(), p->d_ovp.get()};
    hipLaunchKernelGGL(k_union_values, dim3(blocks), dim3(UNION_BLOCK), 0, st, T, (long long) p->nnz_u, total,
                       step / p->nnz_u, step % p->nnz_u, Ax, reinterpret_cast<u64 *>(out));
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

}  // namespace

extern "C" {

int cs3_union_limits(cs3_union_limits_t *out)
{
    if (!out) { set_error("cs3_union_limits: null output"); return CS3_ERR_ARG; }
    out->block = UNION_BLOCK;
    out->grid_cap = UNION_GRID_CAP;
    out->entries_per_lane = UNION_PER_LANE;
    return CS3_OK;
}

int cs3_union_upload(cs3_union p)
{
    if (!p) { set_error("cs3_union_upload: null plan"); return CS3_ERR_ARG; }
    if (p->uploaded) return CS3_OK;
    if (no_device("cs3_union_upload")) return CS3_ERR_HIP;
    CS3_HIP(p->d_map.upload(p->map));
    CS3_HIP(p->d_map_of.upload(p->map_of));
    CS3_HIP(p->d_ovs.upload(p->ovs));
    CS3_HIP(p->d_off.upload(p->off));
    CS3_HIP(p->d_ovp.upload(p->ovp));
    p->uploaded = true;
    return CS3_OK;
}

int cs3_union_values_dev(cs3_union p, const double *Ax_cat_dev, double *Ax_union_dev, void *stream)
{
    if (!p) { set_error("cs3_union_values_dev: null plan"); return CS3_ERR_ARG; }
    if (!p->uploaded) { const int rc = cs3_union_upload(p); if (rc) return rc; }      // (CS3_ERR_HIP without a device)
    if (p->nmat * p->nnz_u > 0 && (!Ax_union_dev || (p->nnz_total > 0 && !Ax_cat_dev))) {
        set_error("cs3_union_values_dev: null value array"); return CS3_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(Ax_union_dev) & 7) { set_error("cs3_union_values_dev: output not aligned to 8 bytes"); return CS3_ERR_ARG; }
    return union_launch(p, Ax_cat_dev, Ax_union_dev, (hipStream_t) stream);
}

int cs3_union_values(cs3_union p, const double *Ax_cat, double *Ax_union)
{
    if (!p) { set_error("cs3_union_values: null plan"); return CS3_ERR_ARG; }
    if (!p->uploaded) { const int rc = cs3_union_upload(p); if (rc) return rc; }
    const size_t total = (size_t) p->nmat * (size_t) p->nnz_u;
    if (total == 0) return CS3_OK;
    if (!Ax_union || (p->nnz_total > 0 && !Ax_cat)) { set_error("cs3_union_values: null value array"); return CS3_ERR_ARG; }
    DevBuf<double> cat, uni;
    CS3_HIP(cat.upload(Ax_cat, (size_t) p->nnz_total));
    CS3_HIP(uni.alloc(total));
    const int rc = union_launch(p, cat.get(), uni.get(), nullptr);
    if (rc) return rc;
    CS3_HIP(hipMemcpy(Ax_union, uni.get(), total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

}  // extern "C"
