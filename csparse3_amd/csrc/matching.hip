// Device side of a matched handle (cs3_analyze_matched): the handle factorises B = P (Dr A Dc) while its callers speak in
// terms of A.  Three bandwidth kernels around the unchanged factor and sweep kernels: the values of A scaled into the
// library's copy, the row permutations of a solve with the scalings folded in, and the two scalars that turn
// slogdet(B) into slogdet(A).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_device.hpp"

namespace cs3 {

namespace {

#define CS3_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

int match_grid(long long work, int block, int cap = 4096)
{
    return (int) std::max<long long>(1, std::min<long long>((work + block - 1) / block, cap));
}

}  // namespace

// dst[b nnz + p] = (dr[row(p)] * src[b nnz + p]) * dc[col(p)]: two roundings in this order, so that a host can rebuild B
// bit for bit.  src may be dst (the host form of cs3_factor has copied the values there already).  The values stream
// through coalesced; the gathers of dr / dc hit the cache (the entries of a column share dc, their rows are near).
__global__ void __launch_bounds__(256)
k_match_values(const double *src, double *dst, const int *__restrict__ erow, const int *__restrict__ ecol,
               const double *__restrict__ dr, const double *__restrict__ dc, long long nnz, long long total)
{
    for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x) {
        const long long p = e % nnz;
        const double t = dr[erow[p]] * src[e];
        dst[e] = t * dc[ecol[p]];
    }
}

// The matched forms of k_permute_rows, [row][rhs] row-major, consecutive threads along the right-hand sides of a row,
// the batch on blockIdx.y:  gather  dst[k, :] = scale[map[k]] * src[map[k], :],  scatter  dst[map[k], :] = scale[map[k]] * src[k, :].
__global__ void __launch_bounds__(256)
k_match_rows(const double *__restrict__ src, double *__restrict__ dst, const int *__restrict__ map,
             const double *__restrict__ scale, long long n, int nrhs, int scatter, long long stride)
{
    const double *s = src + (long long) blockIdx.y * stride;
    double *d = dst + (long long) blockIdx.y * stride;
    const long long total = n * nrhs;
    for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x) {
        const long long k = e / nrhs;
        const int t = (int) (e - k * nrhs);
        const int m = map[k];
        const long long o = (long long) m * nrhs + t;
        if (scatter) d[o] = scale[m] * s[e]; else d[e] = scale[m] * s[o];
    }
}

// slogdet(B) -> slogdet(A): sign *= parity of the row permutation, logabs += -(sum log dr + sum log dc)
__global__ void __launch_bounds__(64)
k_match_slogdet(double *sign, double *logabs, long long batch, double parity, double shift)
{
    const long long b = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    if (sign[b] != 0.0) sign[b] *= parity;
    logabs[b] += shift;
}

hipError_t launch_match_values(const MatchView &M, const double *src, double *dst, long long nnz, long long batch, hipStream_t st)
{
    const long long total = nnz * batch;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_match_values, dim3(match_grid(total, 256)), dim3(256), 0, st, src, dst, M.erow, M.ecol, M.dr, M.dc, nnz, total);
    CS3_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_match_rows(const double *src, double *dst, const int *map, const double *scale, long long n, int nrhs,
                             long long batch, bool scatter, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    dim3 grid(match_grid(n * (long long) nrhs, 256), (unsigned) batch);
    hipLaunchKernelGGL(k_match_rows, grid, dim3(256), 0, st, src, dst, map, scale, n, nrhs, scatter ? 1 : 0, n * (long long) nrhs);
    CS3_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_match_slogdet(double *sign, double *logabs, long long batch, double parity, double shift, hipStream_t st)
{
    hipLaunchKernelGGL(k_match_slogdet, dim3((unsigned) ((batch + 63) / 64)), dim3(64), 0, st, sign, logabs, batch, parity, shift);
    CS3_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace cs3
