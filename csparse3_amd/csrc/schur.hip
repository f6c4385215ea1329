// Device side of a Schur handle (cs3_analyze_schur): the front of the Schur variables is assembled by k_big_gather like
// any big front and then NOT eliminated.  One kernel moves the assembled front -- the Schur complement
// S = A22 - A21 A11^-1 A12 -- into the handle's own buffer and leaves the identity in its place, so that the unchanged
// sweeps run through the front as through factors [L11 0; L21 I] [U11 U12; 0 I].
#include <hip/hip_runtime.h>

#include "cs3_device.hpp"

namespace cs3 {

#define CS3_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

constexpr int ST = 32;             // tile order: 32 x 8 threads, four entries each

// Workgroup (ti, tj, b) owns tile (ti, tj) of the column-major front F [ns, ns] of matrix b: it reads the tile (coalesced
// down the columns), writes it to the row-major S through an LDS tile whose rows are padded by one double (coalesced along
// the rows of S, conflict-free in the LDS), and overwrites it with the identity.  Nobody else touches the tile, so the
// launch needs no order between workgroups.
// Cholesky: the gather fills the lower triangle only.  The workgroups of the lower tiles (ti >= tj) also write the mirror
// image S(j, i) = F(i, j) straight from their registers and the identity into the mirrored tile of F; the others leave.
// The last tiles are predicated on i, j < ns: nothing is read or written past the two buffers.
template <int KIND>
__global__ void __launch_bounds__(256)
k_schur_take(double *__restrict__ pool_all, long long pool_stride, long long lpan, int ns, double *__restrict__ S_all)
{
    __shared__ double tile[ST][ST + 1];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (KIND == CS3_CHOLESKY && ti < tj) return;
    double *F = pool_all + (long long) blockIdx.z * pool_stride + lpan;
    double *S = S_all + (long long) blockIdx.z * ns * ns;
    const int tx = threadIdx.x & (ST - 1), ty = threadIdx.x / ST;      // 32 x 8
    const int i0 = ti * ST, j0 = tj * ST;
    {
        const int i = i0 + tx;
#pragma unroll
        for (int u = 0; u < ST / 8; ++u) {
            const int jj = ty + 8 * u, j = j0 + jj;
            const bool in = i < ns && j < ns;
            const long long at = (long long) i + (long long) j * ns;
            const double v = in ? F[at] : 0.0;
            tile[jj][tx] = v;
            if (in) F[at] = (i == j) ? 1.0 : 0.0;
            if (KIND == CS3_CHOLESKY && in && i > j) S[(long long) j * ns + i] = v;
        }
    }
    __syncthreads();
    {
        const int j = j0 + tx;
#pragma unroll
        for (int u = 0; u < ST / 8; ++u) {
            const int ii = ty + 8 * u, i = i0 + ii;
            if (i >= ns || j >= ns) continue;
            if (KIND != CS3_CHOLESKY || i >= j) S[(long long) i * ns + j] = tile[tx][ii];
            // the mirrored tile of F (rows j0.., columns i0..): entry (j, i), coalesced along j
            if (KIND == CS3_CHOLESKY && ti != tj) F[(long long) j + (long long) i * ns] = 0.0;
        }
    }
}

hipError_t launch_schur_take(const DeviceFactor &D, hipStream_t st)
{
    const int ns = D.schur_ns;
    if (ns < 1 || !D.schur) return hipErrorInvalidValue;
    const unsigned nt = (unsigned) ((ns + ST - 1) / ST);
    const dim3 grid(nt, nt, (unsigned) D.batch);
    if (D.kind == CS3_LU)
        hipLaunchKernelGGL((k_schur_take<CS3_LU>), grid, dim3(256), 0, st, D.pool_pm, D.pm_stride, D.schur_lpan, ns, D.schur);
    else
        hipLaunchKernelGGL((k_schur_take<CS3_CHOLESKY>), grid, dim3(256), 0, st, D.pool_pm, D.pm_stride, D.schur_lpan, ns, D.schur);
    CS3_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace cs3
