// Sparse right-hand sides, Y = C op(A)^-1 B on the factors a handle holds (cs3_sens_*): the two kernels around the handle's
// own many-RHS solves.
//
//     T = (columns c0 .. c0 + t of the solved-for operand, densified)      k_sens_scatter
//     T = op(A)^-1 T  (side left: op(A)^-T T)                              the handle's solve, in place
//     out[g, j] = sum_e v_e T[i_e, j]   over the entries of column g of the OTHER operand      k_sens_combine
//
// apps.cpp drives it per tile of at most 1024 solved-for columns.  Side right solves for columns of B and combines with the
// rows of C (out = Y[g, c0 + j]); side left solves for rows of C and combines with the columns of B (out = Y[c0 + j, g],
// stored through LDS so that both the reads of T and the stores to Y are contiguous).
//
// Every sum runs in storage order with the product rounded before the add, and there are no atomics: results are bitwise
// reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // v * T is rounded, then added: the sums cs3_matvec_dev documents

namespace cs3 {

namespace {

constexpr int SC_NT = SENS_SCATTER_THREADS, SC_ROWS = SENS_SCATTER_ROWS;
constexpr int CB_J = SENS_COMBINE_LANES;        // 64 tile columns: a wave reads 512 contiguous bytes of a row of T
constexpr int CB_G = SENS_COMBINE_COLS;         // 32 columns of the other operand per workgroup = the transposing block edge
constexpr int CB_NT = 256;
constexpr int CB_LD = CB_J + 1;                 // LDS row of the transposing store: the reads along g spread over the banks
static_assert(CB_G == SENS_TBLOCK && CB_NT == 4 * CB_J && CB_G % 4 == 0 && CB_NT % CB_G == 0, "the lane maps of k_sens_combine");

}  // namespace

// The tile's right-hand sides: T [n, w] row-major.  Column j < t holds column c0 + j of the operand (an identity operand:
// e_{c0 + j}), columns t .. w - 1 are the zero padding up to the solve width.  A workgroup owns SC_ROWS rows, a thread its
// columns j, j + SC_NT, ...: it first zeroes them (consecutive lanes, consecutive addresses), then walks the entries of
// its columns in storage order and adds those that fall into the workgroup's rows -- to addresses it zeroed itself, so
// program order is all the ordering needed, and duplicates add in storage order without atomics.
__global__ void __launch_bounds__(SC_NT)
k_sens_scatter(double *__restrict__ T, long long n, int w, SensOperand op, long long c0, int t)
{
    const long long i0 = (long long) blockIdx.x * SC_ROWS, i1 = std::min(n, i0 + SC_ROWS);
    for (int j = threadIdx.x; j < w; j += SC_NT) {
        for (long long i = i0; i < i1; ++i) T[i * w + j] = 0.0;
        if (j >= t) continue;
        if (!op.p) {
            const long long i = c0 + j;
            if (i >= i0 && i < i1) T[i * w + j] = 1.0;
            continue;
        }
        for (int e = op.p[c0 + j]; e < op.p[c0 + j + 1]; ++e) {
            const long long i = op.i[e];
            if (i >= i0 && i < i1) T[i * w + j] += op.x[e];
        }
    }
}

// out[g, j] = sum_e v_e T[i_e, j] over the entries e of column g of `op` (an identity operand: T[g, j]), for the tile
// columns j < t.  A workgroup owns CB_G columns g and CB_J tile columns j; lanes run along j, so every read of a row of T
// is contiguous, and wave v takes g = v, v + 4, ...  The first product starts the sum (a unit value hands T's bits over).
// TRANSPOSED = false: Y[g * ldy + c0 + j], contiguous along j.  TRANSPOSED = true: Y[(c0 + j) * ldy + g]: the block goes
// through LDS and leaves with lanes along g, CB_G contiguous doubles per row of Y.
template <bool TRANSPOSED>
__global__ void __launch_bounds__(CB_NT)
k_sens_combine(const double *__restrict__ T, int w, int t, SensOperand op, long long ng, long long c0, long long ldy,
               double *__restrict__ Y)
{
    __shared__ double blk[TRANSPOSED ? CB_G * CB_LD : 1];
    const int tid = threadIdx.x, lane = tid % CB_J, wave = tid / CB_J;
    const int j = blockIdx.y * CB_J + lane;
    const long long g0 = (long long) blockIdx.x * CB_G;
    for (int gl = wave; gl < CB_G; gl += CB_NT / CB_J) {
        const long long g = g0 + gl;
        double acc = 0.0;
        if (g < ng && j < t) {
            if (!op.p) {
                acc = T[g * w + j];
            } else {
                const int e0 = op.p[g], e1 = op.p[g + 1];
                for (int e = e0; e < e1; ++e) {
                    const double prod = op.x[e] * T[(long long) op.i[e] * w + j];
                    acc = (e == e0) ? prod : acc + prod;
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

#define CS3_SENS_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_sens_scatter(double *T, long long n, int w, const SensOperand &op, long long c0, int t, hipStream_t st)
{
    if (n == 0 || w == 0) return hipSuccess;
    if (t > w || w > SENS_MAX_TILE) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sens_scatter, dim3((unsigned) ((n + SC_ROWS - 1) / SC_ROWS)), dim3(SC_NT), 0, st, T, n, w, op, c0, t);
    CS3_SENS_CHECK();
    return hipSuccess;
}

hipError_t launch_sens_combine(const double *T, int w, int t, const SensOperand &op, long long ng, long long c0, long long ldy,
                               bool transposed, double *Y, hipStream_t st)
{
    if (ng == 0 || t == 0) return hipSuccess;
    if (t > w || w > SENS_MAX_TILE) return hipErrorInvalidValue;
    const dim3 grid((unsigned) ((ng + CB_G - 1) / CB_G), (unsigned) ((t + CB_J - 1) / CB_J));
    if (transposed) hipLaunchKernelGGL(k_sens_combine<true>, grid, dim3(CB_NT), 0, st, T, w, t, op, ng, c0, ldy, Y);
    else hipLaunchKernelGGL(k_sens_combine<false>, grid, dim3(CB_NT), 0, st, T, w, t, op, ng, c0, ldy, Y);
    CS3_SENS_CHECK();
    return hipSuccess;
}

}  // namespace cs3
