// Bilinear forms on the selected inverse (include/csparse3_amd.h, "bilinear forms on the selected inverse"): for m sparse row
// pairs (c_i, b_i) whose index pairs lie on the pattern of L + U,
//
//     t_i = c_i' A^-1 b_i = sum over the entries a of c_i and b of b_i of (c_a * Z(a, b)) * b_b
//
// read out of the zpool that cs3_selinv_dev left on the handle, and the normalised residuals of a state estimate on top:
//
//   k_quad_forms            all of t in one launch; the plan's position table holds the zpool offset of every term, a-major
//   k_quad_normres_part     omega_i = 1/w_i - t_i, rn_i, and per workgroup (max rn, its row, sum w r^2, critical rows)
//   k_quad_normres_close    the partials of one matrix into its summary
//
// k_quad_forms runs the rows in three classes by their term count nt (the plan sorts them; QuadShape says which workgroups
// run which class, so the branch is uniform over a workgroup):
//   lane       nt <= QUAD_LANE_TERMS   one lane per row.  The loads are dependent gathers (position, then Z): the lane loads
//                                      QUAD_CHUNK positions, then their QUAD_CHUNK entries of Z, then adds.
//   wave       nt <= QUAD_WAVE_TERMS   one wave per row, four rows per workgroup, four terms of a lane in flight.
//   workgroup  beyond                  one workgroup per row.
//
// Summation order (a host restates every result bit for bit; fp contraction is off, so a term is two rounded products):
//   lane       s = 0; s += term u for u = 0, 1, ..., nt - 1.
//   wave       lane l: s_l = 0; s_l += term u for u = l, l + 64, ...; then the tree s_l += s_(l + off) for l < off,
//              off = 32, 16, 8, 4, 2, 1; t = s_0.  (A lane without terms carries +0.)
//   workgroup  thread j of 256: s_j += term u for u = j, j + 256, ...; the tree inside each of the four waves; then
//              t = ((S_0 + S_1) + S_2) + S_3 over the waves' sums, through LDS.
// The reductions of the normalised residuals use the same tree and the same order of the waves: k_quad_normres_part owns
// rows 256 g .. 256 g + 255 (thread j row 256 g + j; a row past m carries +0 and loses every comparison),
// k_quad_normres_close gives thread j the partials j, j + 256, ... in that order, then the tree and the waves.  The
// largest rn is taken under a total order (a NaN above every number, then the larger value, then the lower row), so
// its result does not depend on the order of the comparisons.
//
// Every output is written once by the lane that owns it: no memset, no atomics, the same bits on every run.  blockIdx.y is
// the matrix of the batch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // (c * z) * b and w * (r * r) stay rounded products: what a host restates

namespace cs3 {

namespace {

static_assert(QUAD_BLOCK == 256 && QUAD_LANE_TERMS % QUAD_CHUNK == 0, "four waves per workgroup; whole chunks in the lane class");

__device__ inline double quad_wave_tree(double s)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off, 64);
    return s;                                               // (lane 0 holds the sum)
}

// the sum of the four waves' lane-0 values in wave order, valid in thread 0; every thread of the workgroup calls it
__device__ inline double quad_block_sum(double s, double *lds)
{
    s = quad_wave_tree(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    const double total = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    __syncthreads();
    return total;
}

// terms u = first, first + step, ... of one row, four in flight, added in that order
__device__ inline double quad_strided(const QuadRow &R, int nt, int first, int step, const long long *__restrict__ pos,
                                      const double *__restrict__ z, const double *__restrict__ cx, const double *__restrict__ bx)
{
    double s = 0.0;
    const long long *__restrict__ P = pos + R.term0;
    int u = first;
    for (; u + 3 * step < nt; u += 4 * step) {
        long long p[4];
        double zz[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) p[v] = P[u + v * step];
#pragma unroll
        for (int v = 0; v < 4; ++v) zz[v] = z[p[v]];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int w = u + v * step, a = w / R.nb, b = w - a * R.nb;
            s += (cx[R.c0 + a] * zz[v]) * bx[R.b0 + b];
        }
    }
    for (; u < nt; u += step) {
        const int a = u / R.nb, b = u - a * R.nb;
        s += (cx[R.c0 + a] * z[P[u]]) * bx[R.b0 + b];
    }
    return s;
}

__global__ void __launch_bounds__(QUAD_BLOCK)
k_quad_forms(const double *__restrict__ zpool, long long z_stride, const QuadRow *__restrict__ rows, const long long *__restrict__ pos,
             QuadShape G, const double *__restrict__ cx_all, long long cx_stride, const double *__restrict__ bx_all, long long bx_stride,
             long long m, double *__restrict__ t_all)
{
    __shared__ double lds[4];
    const long long mat = blockIdx.y;
    const double *__restrict__ z = zpool + mat * z_stride;
    const double *__restrict__ cx = cx_all + mat * cx_stride;
    const double *__restrict__ bx = bx_all + mat * bx_stride;
    double *__restrict__ t = t_all + mat * m;
    const unsigned blk = blockIdx.x;

    if (blk < G.blk_wave) {                                 // ---- lane class
        const long long k = (long long) blk * QUAD_BLOCK + threadIdx.x;
        if (k >= G.n_lane) return;
        const QuadRow R = rows[k];
        const int nt = R.nc * R.nb;
        const long long *__restrict__ P = pos + R.term0;
        double s = 0.0;
        int a = 0, b = 0;
        for (int u0 = 0; u0 < nt; u0 += QUAD_CHUNK) {
            long long p[QUAD_CHUNK];
            double zz[QUAD_CHUNK];
#pragma unroll
            for (int v = 0; v < QUAD_CHUNK; ++v) p[v] = (u0 + v < nt) ? P[u0 + v] : -1;
#pragma unroll
            for (int v = 0; v < QUAD_CHUNK; ++v) zz[v] = (p[v] >= 0) ? z[p[v]] : 0.0;
#pragma unroll
            for (int v = 0; v < QUAD_CHUNK; ++v) {
                if (u0 + v < nt) {
                    s += (cx[R.c0 + a] * zz[v]) * bx[R.b0 + b];
                    if (++b == R.nb) { b = 0; ++a; }
                }
            }
        }
        t[R.row] = s;
    } else if (blk < G.blk_wg) {                            // ---- wave class
        const long long k = G.n_lane + (long long) (blk - G.blk_wave) * 4 + (threadIdx.x >> 6);
        if (k >= G.n_lane + G.n_wave) return;               // (a whole wave leaves; nothing below synchronises the workgroup)
        const QuadRow R = rows[k];
        const double s = quad_wave_tree(quad_strided(R, R.nc * R.nb, threadIdx.x & 63, 64, pos, z, cx, bx));
        if ((threadIdx.x & 63) == 0) t[R.row] = s;
    } else {                                                // ---- workgroup class
        const QuadRow R = rows[G.n_lane + G.n_wave + (blk - G.blk_wg)];
        const double s = quad_block_sum(quad_strided(R, R.nc * R.nb, threadIdx.x, QUAD_BLOCK, pos, z, cx, bx), lds);
        if (threadIdx.x == 0) t[R.row] = s;
    }
}

// One candidate for the largest normalised residual.  a beats b: a NaN above every number, then the larger value, then
// the lower row -- a total order, so the maximum is the same whatever the order of the comparisons.
struct QuadBest { double v; double row; };

__device__ inline QuadBest quad_better(QuadBest a, QuadBest b)
{
    const bool an = a.v != a.v, bn = b.v != b.v;
    bool take_a;
    if (an != bn) take_a = an;
    else if (an || a.v == b.v) take_a = a.row < b.row;
    else take_a = a.v > b.v;
    return take_a ? a : b;
}

// (max, sum J, sum critical) of the workgroup's 256 candidates in thread 0
__device__ inline void quad_reduce(QuadBest &best, double &J, double &crit, double *lds)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        QuadBest o;
        o.v = __shfl_down(best.v, off, 64);
        o.row = __shfl_down(best.row, off, 64);
        best = quad_better(best, o);
        J = J + __shfl_down(J, off, 64);
        crit = crit + __shfl_down(crit, off, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { lds[4 * wv] = best.v; lds[4 * wv + 1] = best.row; lds[4 * wv + 2] = J; lds[4 * wv + 3] = crit; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; ++v) {
            best = quad_better(best, QuadBest{lds[4 * v], lds[4 * v + 1]});
            J = J + lds[4 * v + 2];
            crit = crit + lds[4 * v + 3];
        }
    }
}

constexpr double QUAD_NO_ROW = 9007199254740992.0;          // 2^53: the row of a candidate that stands for no row

__global__ void __launch_bounds__(QUAD_BLOCK)
k_quad_normres_part(const double *__restrict__ t_all, const double *__restrict__ w_all, const double *__restrict__ r_all, double crit_tol,
                    long long m, long long nparts, double *__restrict__ omega_all, double *__restrict__ rn_all,
                    double *__restrict__ parts)
{
    __shared__ double lds[16];
    const long long mat = blockIdx.y, i = (long long) blockIdx.x * QUAD_BLOCK + threadIdx.x;
    QuadBest best{-1.0, QUAD_NO_ROW};
    double J = 0.0, crit = 0.0;
    if (i < m) {
        const double t = t_all[mat * m + i], w = w_all[mat * m + i], r = r_all[mat * m + i];
        const double omega = 1.0 / w - t;
        const bool critical = 1.0 - w * t <= crit_tol;
        const double rn = critical ? 0.0 : fabs(r) / sqrt(omega);
        if (omega_all) omega_all[mat * m + i] = omega;
        if (rn_all) rn_all[mat * m + i] = rn;
        best = QuadBest{rn, (double) i};
        J = w * (r * r);
        crit = critical ? 1.0 : 0.0;
    }
    quad_reduce(best, J, crit, lds);
    if (threadIdx.x == 0) {
        double *out = parts + 4 * (mat * nparts + blockIdx.x);
        out[0] = best.v; out[1] = best.row; out[2] = J; out[3] = crit;
    }
}

__global__ void __launch_bounds__(QUAD_BLOCK)
k_quad_normres_close(const double *__restrict__ parts, long long nparts, double *__restrict__ summary)
{
    __shared__ double lds[16];
    const long long mat = blockIdx.x;
    QuadBest best{-1.0, QUAD_NO_ROW};
    double J = 0.0, crit = 0.0;
    for (long long g = threadIdx.x; g < nparts; g += QUAD_BLOCK) {
        const double *in = parts + 4 * (mat * nparts + g);
        best = quad_better(best, QuadBest{in[0], in[1]});
        J = J + in[2];
        crit = crit + in[3];
    }
    quad_reduce(best, J, crit, lds);
    if (threadIdx.x == 0) {
        double *out = summary + 4 * mat;
        out[0] = best.v; out[1] = best.row; out[2] = J; out[3] = crit;
    }
}

}  // namespace

hipError_t launch_quad_forms(const double *zpool, long long z_stride, const QuadRow *rows, const long long *pos, const QuadShape &G,
                             const double *cx, long long cx_stride, const double *bx, long long bx_stride, long long m,
                             long long batch, double *t, hipStream_t st)
{
    if (G.blocks == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(k_quad_forms, dim3(G.blocks, (unsigned) batch), dim3(QUAD_BLOCK), 0, st, zpool, z_stride, rows, pos, G, cx,
                       cx_stride, bx, bx_stride, m, t);
    return hipGetLastError();
}

hipError_t launch_quad_normres(const double *t, const double *w, const double *r, double crit_tol, long long m, long long batch,
                               double *omega, double *rn, double *parts, double *summary, hipStream_t st)
{
    if (m == 0 || batch == 0) return hipSuccess;
    const long long nparts = (m + QUAD_BLOCK - 1) / QUAD_BLOCK;
    hipLaunchKernelGGL(k_quad_normres_part, dim3((unsigned) nparts, (unsigned) batch), dim3(QUAD_BLOCK), 0, st, t, w, r, crit_tol, m,
                       nparts, omega, rn, parts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_quad_normres_close, dim3((unsigned) batch), dim3(QUAD_BLOCK), 0, st, parts, nparts, summary);
    return hipGetLastError();
}

}  // namespace cs3
