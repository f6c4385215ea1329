// Complex selected inversion (include/csparse3_amd.h, "complex selected inversion"): Z = A^-1 of a complex matrix read out
// of the real selected inverse ZR that cs3_selinv_dev left on the handle of the real-equivalent form.  The handle
// factorises the real form of M = diag(s) A, so per matrix of the batch
//
//     Minv(i, j) = (ZR(2i, 2j), ZR(2i + 1, 2j))        the first column of the 2 x 2 block; the twin column is not read
//     Z(i, j)    = Minv(i, j) * s_j                     A^-1 = M^-1 diag(s)
//
//   k_cselinv_entries    Zz[e] = Z(Ai[e], j) for entry e of column j; trans: Z(j, Ai[e]), rotated by s of the ROW of the entry
//   k_cselinv_diag       d[i] = Z(i, i)
//   k_cselinv_thevenin   T[e] = ((Z(i, i) + Z(j, j)) - Z(i, j)) - Z(j, i), i = Ai[e]: eight reads of ZR, four rotations and the
//                        three additions in one lane
//
// All three are gathers: every output is written exactly once by the lane that owns it -- no memset, no atomics, nothing
// allocated, nothing waited for.  The maps hold the zpool offsets of a pair (real part, imaginary part) as one 16-byte
// entry, the index table the pair (row, column) of an entry as one 8-byte entry: consecutive lanes load consecutive map
// entries and store consecutive results; the reads of zpool (and of s) are scattered by nature.
//
// Arithmetic: the product is (ar*br - ai*bi, ar*bi + ai*br), every product rounded before the sum (fp contraction is off),
// and it is made also when s = (1, +0).  A host restates every result bit for bit with the same expressions.
//
// Shape: 256 threads, grid-stride over a flat 64-bit index under CSELINV_GRID_CAP workgroups, one complex number per
// lane; the flat index is split by division in every pass, as in cplxplan.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // a * b - c * d stays three roundings: what a host restates

namespace cs3 {

namespace {

__device__ inline double2 csel_mul(double2 a, double2 b)
{
    double2 w;
    w.x = (a.x * b.x) - (a.y * b.y);
    w.y = (a.x * b.y) + (a.y * b.x);
    return w;
}

// (ZR at off.x, ZR at off.y) * s
__device__ inline double2 csel_z(const double *__restrict__ z, longlong2 off, double2 s)
{
    return csel_mul(make_double2(z[off.x], z[off.y]), s);
}

#define CSELINV_GRID_STRIDE(idx, total)                                                                  \
    for (long long idx = (long long) blockIdx.x * CSELINV_BLOCK + threadIdx.x; idx < (total);            \
         idx += (long long) gridDim.x * CSELINV_BLOCK)

// one lane per (matrix, entry); `map` is the entry map, or with trans the map of the transposed positions
__global__ void __launch_bounds__(CSELINV_BLOCK)
k_cselinv_entries(const double *__restrict__ zpool, long long z_stride, const longlong2 *__restrict__ map,
                  const int2 *__restrict__ ij, int trans, const double2 *__restrict__ S, long long n, long long nnz, long long total,
                  double2 *__restrict__ out)
{
    CSELINV_GRID_STRIDE(idx, total) {
        const long long b = idx / nnz, e = idx - b * nnz;
        const int2 c = ij[e];
        out[idx] = csel_z(zpool + b * z_stride, map[e], S[b * n + (trans ? c.x : c.y)]);
    }
}

// one lane per (matrix, bus)
__global__ void __launch_bounds__(CSELINV_BLOCK)
k_cselinv_diag(const double *__restrict__ zpool, long long z_stride, const longlong2 *__restrict__ dmap,
               const double2 *__restrict__ S, long long n, long long total, double2 *__restrict__ out)
{
    CSELINV_GRID_STRIDE(r, total) {
        const long long b = r / n, i = r - b * n;
        out[r] = csel_z(zpool + b * z_stride, dmap[i], S[r]);
    }
}

// one lane per (matrix, entry)
__global__ void __launch_bounds__(CSELINV_BLOCK)
k_cselinv_thevenin(const double *__restrict__ zpool, long long z_stride, CselinvMaps M, const double2 *__restrict__ S, long long n,
                   long long nnz, long long total, double2 *__restrict__ out)
{
    const longlong2 *__restrict__ entry = reinterpret_cast<const longlong2 *>(M.entry);
    const longlong2 *__restrict__ entry_t = reinterpret_cast<const longlong2 *>(M.entry_t);
    const longlong2 *__restrict__ diag = reinterpret_cast<const longlong2 *>(M.diag);
    const int2 *__restrict__ ij = reinterpret_cast<const int2 *>(M.ij);
    CSELINV_GRID_STRIDE(idx, total) {
        const long long b = idx / nnz, e = idx - b * nnz;
        const int2 c = ij[e];                                       // (i, j)
        const double *z = zpool + b * z_stride;
        const double2 si = S[b * n + c.x], sj = S[b * n + c.y];
        const double2 zii = csel_z(z, diag[c.x], si), zjj = csel_z(z, diag[c.y], sj);
        const double2 zij = csel_z(z, entry[e], sj), zji = csel_z(z, entry_t[e], si);
        double2 t;
        t.x = ((zii.x + zjj.x) - zij.x) - zji.x;
        t.y = ((zii.y + zjj.y) - zij.y) - zji.y;
        out[idx] = t;
    }
}

unsigned csel_blocks(long long total)
{
    return (unsigned) std::min<long long>((total + CSELINV_BLOCK - 1) / CSELINV_BLOCK, CSELINV_GRID_CAP);
}

}  // namespace

hipError_t launch_cselinv_entries(const double *zpool, long long z_stride, const CselinvMaps &M, bool trans, const double *s,
                                  long long n, long long nnz, long long batch, double *out, hipStream_t st)
{
    const long long total = batch * nnz;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cselinv_entries, dim3(csel_blocks(total)), dim3(CSELINV_BLOCK), 0, st, zpool, z_stride,
                       reinterpret_cast<const longlong2 *>(trans ? M.entry_t : M.entry), reinterpret_cast<const int2 *>(M.ij),
                       trans ? 1 : 0, reinterpret_cast<const double2 *>(s), n, nnz, total, reinterpret_cast<double2 *>(out));
    return hipGetLastError();
}

hipError_t launch_cselinv_diag(const double *zpool, long long z_stride, const CselinvMaps &M, const double *s, long long n,
                               long long batch, double *out, hipStream_t st)
{
    const long long total = batch * n;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cselinv_diag, dim3(csel_blocks(total)), dim3(CSELINV_BLOCK), 0, st, zpool, z_stride,
                       reinterpret_cast<const longlong2 *>(M.diag), reinterpret_cast<const double2 *>(s), n, total,
                       reinterpret_cast<double2 *>(out));
    return hipGetLastError();
}

hipError_t launch_cselinv_thevenin(const double *zpool, long long z_stride, const CselinvMaps &M, const double *s, long long n,
                                   long long nnz, long long batch, double *out, hipStream_t st)
{
    const long long total = batch * nnz;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cselinv_thevenin, dim3(csel_blocks(total)), dim3(CSELINV_BLOCK), 0, st, zpool, z_stride, M,
                       reinterpret_cast<const double2 *>(s), n, nnz, total, reinterpret_cast<double2 *>(out));
    return hipGetLastError();
}

}  // namespace cs3
