// Complex sparse right-hand sides, Y = C op(A)^-1 B on a handle that holds the real-equivalent form of a complex matrix
// (cs3_cplx_sens_*), and the complex Schur complement read out of the real one (cs3_cplx_schur_get*).  The two kernels of
// sens.hip with the plan's pack and unpack (cplxplan.hip) folded in, around the handle's unchanged many-RHS solves:
//
//     T [2n, w] = pack_inner(columns c0 .. c0 + t of the solved-for operand, densified)         k_csens_scatter
//     T = M^-1 T (inner N) or M^-T T (inner T, H), M = the real form of diag(s) A                the handle's solve, in place
//     out[g, j] = sum_e v_e * unpack_inner(T[2 i_e, j], T[2 i_e + 1, j])                         k_csens_combine
//
// One complex solved-for column is ONE real column of the tile: side left with p rows of C costs p solves, where the real
// sens path on the real form would need the real and the imaginary row of every row of C, 2p.  apps.cpp drives it per tile
// and picks `inner` and the conjugations (include/csparse3_amd.h, "complex sparse right-hand sides").
//
// Arithmetic is that of cplxplan.hip: a complex product is four rounded products, then the two sums; a conjugate is a sign
// flip; every sum runs in storage order, component by component; no atomics.  A host restates every result bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/csparse3_amd.h"
#include "cs3_device.hpp"

#pragma clang fp contract(off)          // a * b - c * d stays three roundings: what a host restates

namespace cs3 {

namespace {

constexpr int SC_NT = SENS_SCATTER_THREADS, SC_ROWS = CSENS_SCATTER_ROWS;
constexpr int CB_J = SENS_COMBINE_LANES;        // 64 tile columns: a wave reads 512 contiguous bytes of each row of a pair
constexpr int CB_G = SENS_COMBINE_COLS;         // 32 columns of the other operand per workgroup = the transposing block edge
constexpr int CB_NT = 256;
constexpr int CB_LD = CSENS_BLOCK_LD;           // LDS row of the transposing store: the reads along g spread over the banks
constexpr int GATHER_NT = 256, GATHER_GRID_CAP = 2048;
static_assert(2 * SC_ROWS == SENS_SCATTER_ROWS, "a scatter workgroup owns whole pairs of real rows");
static_assert(CB_G == SENS_TBLOCK && CB_NT == 4 * CB_J && CB_G % 4 == 0 && CB_NT % CB_G == 0, "the lane maps of k_csens_combine");

__device__ inline double2 cmul(double2 a, double2 b)
{
    double2 w;
    w.x = (a.x * b.x) - (a.y * b.y);
    w.y = (a.x * b.y) + (a.y * b.x);
    return w;
}

__device__ inline double2 cconj(double2 a) { a.y = -a.y; return a; }

// what cs3_cplx_pack_dev does to one number of row i
__device__ inline double2 pack_inner(const CsensGlue &g, long long i, double2 v)
{
    if (g.conj) v = cconj(v);
    if (g.inner == CS3_CPLX_N) return cmul(reinterpret_cast<const double2 *>(g.s)[i], v);
    return g.inner == CS3_CPLX_T ? cconj(v) : v;
}

// what cs3_cplx_unpack_dev does to one number of row i
__device__ inline double2 unpack_inner(const CsensGlue &g, long long i, double2 y)
{
    if (g.inner == CS3_CPLX_H) y = cmul(cconj(reinterpret_cast<const double2 *>(g.s)[i]), y);
    else if (g.inner == CS3_CPLX_T) y = cmul(reinterpret_cast<const double2 *>(g.s)[i], cconj(y));
    return g.conj ? cconj(y) : y;
}

}  // namespace

// The tile's right-hand sides: T [2n, w] real, row-major.  Column j < t holds pack_inner of column c0 + j of the operand
// (an identity operand: of e_{c0 + j}), columns t .. w - 1 are the zero padding up to the solve width.  A workgroup owns
// SC_ROWS complex rows -- 2 SC_ROWS real rows, never half a pair --, a thread its columns j, j + SC_NT, ...: it zeroes both
// rows of every pair, then walks the entries of its columns in storage order and adds Re u to row 2i, Im u to row 2i + 1,
// to addresses it zeroed itself: program order is all the ordering needed, duplicates add in storage order.
__global__ void __launch_bounds__(SC_NT)
k_csens_scatter(double *__restrict__ T, long long n, int w, CsensOperand op, long long c0, int t, CsensGlue g)
{
    const long long i0 = (long long) blockIdx.x * SC_ROWS, i1 = std::min(n, i0 + SC_ROWS);
    const double2 *x = reinterpret_cast<const double2 *>(op.x);
    for (int j = threadIdx.x; j < w; j += SC_NT) {
        for (long long r = 2 * i0; r < 2 * i1; ++r) T[r * w + j] = 0.0;
        if (j >= t) continue;
        if (!op.p) {
            const long long i = c0 + j;
            if (i >= i0 && i < i1) {
                const double2 u = pack_inner(g, i, make_double2(1.0, 0.0));
                T[2 * i * w + j] = u.x;
                T[(2 * i + 1) * w + j] = u.y;
            }
            continue;
        }
        for (int e = op.p[c0 + j]; e < op.p[c0 + j + 1]; ++e) {
            const long long i = op.i[e];
            if (i >= i0 && i < i1) {
                const double2 u = pack_inner(g, i, x[e]);
                T[2 * i * w + j] += u.x;
                T[(2 * i + 1) * w + j] += u.y;
            }
        }
    }
}

// out[g, j] = sum_e v_e * unpack_inner(T[2 i_e, j], T[2 i_e + 1, j]) over the entries e of column g of `op` (an identity
// operand: the unpacked (T[2g, j], T[2g + 1, j])), for the tile columns j < t.  A workgroup owns CB_G columns g and CB_J
// tile columns j; lanes run along j, so both reads of a pair are contiguous, and wave v takes g = v, v + 4, ...  The first
// product starts the sum; later products add component by component.
// TRANSPOSED = false: Y[g * ldy + c0 + j], contiguous along j.  TRANSPOSED = true: Y[(c0 + j) * ldy + g]: the block goes
// through LDS and leaves with lanes along g, CB_G contiguous complex numbers per row of Y.
template <bool TRANSPOSED>
__global__ void __launch_bounds__(CB_NT)
k_csens_combine(const double *__restrict__ T, int w, int t, CsensOperand op, long long ng, long long c0, long long ldy, CsensGlue gl_,
                double2 *__restrict__ Y)
{
    __shared__ double2 blk[TRANSPOSED ? CB_G * CB_LD : 1];
    const int tid = threadIdx.x, lane = tid % CB_J, wave = tid / CB_J;
    const int j = blockIdx.y * CB_J + lane;
    const long long g0 = (long long) blockIdx.x * CB_G;
    const double2 *x = reinterpret_cast<const double2 *>(op.x);
    for (int gl = wave; gl < CB_G; gl += CB_NT / CB_J) {
        const long long g = g0 + gl;
        double2 acc = make_double2(0.0, 0.0);
        if (g < ng && j < t) {
            if (!op.p) {
                acc = unpack_inner(gl_, g, make_double2(T[2 * g * w + j], T[(2 * g + 1) * w + j]));
            } else {
                const int e0 = op.p[g], e1 = op.p[g + 1];
                for (int e = e0; e < e1; ++e) {
                    const long long i = op.i[e];
                    const double2 prod = cmul(x[e], unpack_inner(gl_, i, make_double2(T[2 * i * w + j], T[(2 * i + 1) * w + j])));
                    if (e == e0) acc = prod;
                    else { acc.x = acc.x + prod.x; acc.y = acc.y + prod.y; }
                }
            }
            if (!TRANSPOSED) Y[g * ldy + c0 + j] = acc;
        }
        if (TRANSPOSED) blk[gl * CB_LD + lane] = acc;
    }
    if (TRANSPOSED) {
        __syncthreads();
        const int gl = tid % CB_G;
        const long long g = g0 + gl;
        for (int jl = tid / CB_G; jl < CB_J; jl += CB_NT / CB_G) {
            const int jj = blockIdx.y * CB_J + jl;
            if (g < ng && jj < t) Y[(c0 + jj) * ldy + g] = blk[gl * CB_LD + jl];
        }
    }
}

// S[b][i, j] = (SR[b][2i, 2j], SR[b][2i + 1, 2j]): the first column of every 2 x 2 block of the real Schur complement.  One
// lane per complex number, written once, grid-stride.
__global__ void __launch_bounds__(GATHER_NT)
k_cplx_schur_gather(const double *__restrict__ SR, long long ns, long long total, double2 *__restrict__ S)
{
    for (long long idx = (long long) blockIdx.x * GATHER_NT + threadIdx.x; idx < total; idx += (long long) gridDim.x * GATHER_NT) {
        const long long b = idx / (ns * ns), r = idx - b * ns * ns, i = r / ns, j = r - i * ns;
        const double *blk = SR + b * 4 * ns * ns + 2 * i * 2 * ns + 2 * j;
        S[idx] = make_double2(blk[0], blk[2 * ns]);
    }
}

#define CS3_CSENS_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_csens_scatter(double *T, long long n, int w, const CsensOperand &op, long long c0, int t, const CsensGlue &g,
                                hipStream_t st)
{
    if (n == 0 || w == 0) return hipSuccess;
    if (t > w || w > SENS_MAX_TILE) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_csens_scatter, dim3((unsigned) ((n + SC_ROWS - 1) / SC_ROWS)), dim3(SC_NT), 0, st, T, n, w, op, c0, t, g);
    CS3_CSENS_CHECK();
    return hipSuccess;
}

hipError_t launch_csens_combine(const double *T, int w, int t, const CsensOperand &op, long long ng, long long c0, long long ldy,
                                bool transposed, const CsensGlue &g, double *Y, hipStream_t st)
{
    if (ng == 0 || t == 0) return hipSuccess;
    if (t > w || w > SENS_MAX_TILE) return hipErrorInvalidValue;
    const dim3 grid((unsigned) ((ng + CB_G - 1) / CB_G), (unsigned) ((t + CB_J - 1) / CB_J));
    double2 *y = reinterpret_cast<double2 *>(Y);
    if (transposed) hipLaunchKernelGGL(k_csens_combine<true>, grid, dim3(CB_NT), 0, st, T, w, t, op, ng, c0, ldy, g, y);
    else hipLaunchKernelGGL(k_csens_combine<false>, grid, dim3(CB_NT), 0, st, T, w, t, op, ng, c0, ldy, g, y);
    CS3_CSENS_CHECK();
    return hipSuccess;
}

hipError_t launch_cplx_schur_gather(const double *SR, long long batch, long long ns, double *S, hipStream_t st)
{
    const long long total = batch * ns * ns;
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned) std::min<long long>((total + GATHER_NT - 1) / GATHER_NT, GATHER_GRID_CAP);
    hipLaunchKernelGGL(k_cplx_schur_gather, dim3(blocks), dim3(GATHER_NT), 0, st, SR, ns, total, reinterpret_cast<double2 *>(S));
    CS3_CSENS_CHECK();
    return hipSuccess;
}

}  // namespace cs3
