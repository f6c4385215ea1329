// Condition estimates and log-determinants on the factors a handle holds (cs3_condest*, cs3_slogdet*).
//
// The 1-norm estimate is LAPACK's dlacn2 (ITMAX = 5), one state machine per matrix of the batch.  api.cpp drives it in
// SLOTS: prepare(kind) writes the input of every matrix that the slot serves (zeros for the others), the handle's own
// solve of that kind runs on the work buffer, consume(kind) applies one step of dlacn2 to the served matrices (partial
// reductions over fixed chunks of the vector, then one transition per matrix) and counts what every matrix wants next.
// The kernels here are only those vector steps.
//
// Reductions run in a fixed order (per-thread strided loops, xor butterflies inside a wave, waves and chunks in index
// order), there are no float atomics, and the only integer atomics are the two "wants" counters: results are bitwise
// reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // LAPACK's roundings: 2 * (sum / 3n) and 1 + i / (n - 1) stay separate operations

namespace cs3 {

namespace {

constexpr int EST_NT = 1024;            // one workgroup per matrix (log-determinants)
constexpr int EST_WAVES = EST_NT / 64;
constexpr int PART_NT = 256;            // one workgroup per chunk of EST_CHUNK entries (the partial reductions)
static_assert(PART_NT == EST_NORM_COLS, "k_est_colsums: one column per thread");

// What a state consumes: 1 = x = A^-1 b (F), 2 = x = A^-T b (T), 0 = nothing (DONE).  Steps 1, 3, 5 are F; 2, 4 are T.
__device__ __forceinline__ int step_kind(int step) { return step == 0 ? 0 : (step & 1) ? 1 : 2; }

// first index of the largest value: (m, i) takes (om, oi) when om is larger, or equal with a smaller index
__device__ __forceinline__ void argmax_merge(double &m, int &i, double om, int oi)
{
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}

// the (sum, first argmax, flags) of a wave, every lane ending with the same values (xor butterfly, fixed order)
__device__ __forceinline__ void wave_merge(double &sum, double &mx, int &mi, int &flags)
{
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        argmax_merge(mx, mi, __shfl_xor(mx, off), __shfl_xor(mi, off));
        flags |= __shfl_xor(flags, off);
    }
}

// the current sign vector of matrix b, or the other half of the double buffer
__device__ __forceinline__ const signed char *sign_half(const signed char *S, long long n, long long batch, long long b, int half)
{
    return S + ((long long) half * batch + b) * n;
}

}  // namespace

// Stage 1 of ||A_b||_1: one thread per column sums |A_b(:, j)| in storage order (csc_norm's inner loop, bit for bit), the
// workgroup keeps the largest sum of its 256 columns.  Grid (norm_chunks(n), batch).
__global__ void __launch_bounds__(PART_NT)
k_est_colsums(const int *__restrict__ Cp, const int *__restrict__ Cmap, const double *__restrict__ Ax_all, long long n,
              long long nnz_a, EstPart *__restrict__ parts)
{
    __shared__ double part[PART_NT / 64];
    const long long b = blockIdx.y, j = (long long) blockIdx.x * PART_NT + threadIdx.x;
    const int tid = threadIdx.x;
    const double *ax = Ax_all + b * nnz_a;
    double m = 0.0;
    if (j < n) {
        for (int p = Cp[j]; p < Cp[j + 1]; ++p) m += fabs(ax[Cmap[p]]);
    }
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(m, off); m = (o > m) ? o : m; }   // a max is exact in
    if ((tid & 63) == 0) part[tid >> 6] = m;                                                              // any order; a NaN
    __syncthreads();                                                                                      // sum never wins `>`
    if (tid == 0) {
        for (int w = 0; w < PART_NT / 64; ++w) m = (part[w] > m) ? part[w] : m;
        parts[b * gridDim.x + blockIdx.x].max = m;
    }
}

// Stage 2: ||A_b||_1 = the largest chunk maximum, and the initial state (step 1 = J1, est 0).  One wave per matrix.
__global__ void __launch_bounds__(64)
k_est_init(const EstPart *__restrict__ parts, long long nparts, EstState *__restrict__ state)
{
    const long long b = blockIdx.x;
    double m = 0.0;
    for (long long i = threadIdx.x; i < nparts; i += 64) { const double v = parts[b * nparts + i].max; m = (v > m) ? v : m; }
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(m, off); m = (o > m) ? o : m; }
    if (threadIdx.x == 0) {
        EstState s;
        s.est = 0.0; s.anorm = m; s.step = 1; s.j = 0; s.iter = 0; s.sbuf = 0;
        state[b] = s;
    }
}

// The input of this slot's solve: for a served matrix what its state asks for (J1: 1/n, J2 and J4: s, J3: e_j,
// J5: alt_i = (-1)^i (1 + i/(n-1))), zeros for every other matrix so that nothing stale travels through the solve.
// Clears the counters that the following consume fills.  Grid (chunks of the vector, batch).
__global__ void __launch_bounds__(256)
k_est_prepare(const EstState *__restrict__ state, const signed char *__restrict__ S, double *__restrict__ X, long long n,
              long long batch, int kmask, unsigned *__restrict__ cnt)
{
    const long long b = blockIdx.y;
    const EstState st = state[b];
    const int step = (step_kind(st.step) & kmask) ? st.step : 0;
    double *x = X + b * n;
    const signed char *s = sign_half(S, n, batch, b, st.sbuf);
    const double inv_n = 1.0 / (double) n, nm1 = (double) (n - 1);
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        double v = 0.0;
        if (step == 1) v = inv_n;
        else if (step == 2 || step == 4) v = (double) s[i];
        else if (step == 3) v = (i == st.j) ? 1.0 : 0.0;
        else if (step == 5) { const double a = 1.0 + (double) i / nm1; v = (i & 1) ? -a : a; }
        x[i] = v;
    }
    if (b == 0 && blockIdx.x == 0 && threadIdx.x == 0) { cnt[0] = 0u; cnt[1] = 0u; }
}

// Stage 1 of a dlacn2 step, over one chunk of the solution x of a served matrix: sum |x_i|, first argmax |x_i|, flags
// (1: a non-finite entry; 2, at J3: sign(x_i) != s_i).  At J1 and J3 it also writes sign(x) into the other half of the
// sign buffer; stage 2 adopts that half when the step takes the new signs.  Grid (chunks, batch).
__global__ void __launch_bounds__(PART_NT)
k_est_partial(const EstState *__restrict__ state, signed char *__restrict__ S, const double *__restrict__ X, long long n,
              long long batch, int kmask, EstPart *__restrict__ parts)
{
    __shared__ double w_sum[PART_NT / 64], w_max[PART_NT / 64];
    __shared__ int w_idx[PART_NT / 64], w_flags[PART_NT / 64];
    const long long b = blockIdx.y, c0 = (long long) blockIdx.x * EST_CHUNK, c1 = std::min(n, c0 + EST_CHUNK);
    const EstState st = state[b];
    if (!(step_kind(st.step) & kmask)) return;           // (uniform over the workgroup)
    const int tid = threadIdx.x;
    const double *x = X + b * n;
    const signed char *s = sign_half(S, n, batch, b, st.sbuf);
    signed char *s_new = S + ((long long) (st.sbuf ^ 1) * batch + b) * n;
    const bool signs = st.step == 1 || st.step == 3;
    double sum = 0.0, mx = -1.0;
    int mi = (int) n, flags = 0;
    for (long long i = c0 + tid; i < c1; i += PART_NT) {
        const double v = x[i], a = fabs(v);
        const signed char sg = (v >= 0.0) ? 1 : -1;
        if (!(a <= DBL_MAX)) flags |= 1;
        sum += a;
        if (a > mx) { mx = a; mi = (int) i; }
        if (st.step == 3 && sg != s[i]) flags |= 2;
        if (signs) s_new[i] = sg;
    }
    wave_merge(sum, mx, mi, flags);
    if ((tid & 63) == 0) { w_sum[tid >> 6] = sum; w_max[tid >> 6] = mx; w_idx[tid >> 6] = mi; w_flags[tid >> 6] = flags; }
    __syncthreads();
    if (tid == 0) {
        sum = 0.0; mx = -1.0; mi = (int) n; flags = 0;
        for (int w = 0; w < PART_NT / 64; ++w) { sum += w_sum[w]; argmax_merge(mx, mi, w_max[w], w_idx[w]); flags |= w_flags[w]; }
        EstPart p;
        p.sum = sum; p.max = mx; p.idx = mi; p.flags = flags;
        parts[b * gridDim.x + blockIdx.x] = p;
    }
}

// Stage 2: the chunks combined in index order and one dlacn2 transition per served matrix; then every matrix counts what
// it wants next: cnt[0] += wants F, cnt[1] += wants T.  A non-finite entry in x: est = +inf, DONE.  One wave per matrix.
__global__ void __launch_bounds__(64)
k_est_finish(EstState *__restrict__ state, const double *__restrict__ X, long long n, long long nparts, int kmask,
             const EstPart *__restrict__ parts, unsigned *__restrict__ cnt)
{
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    EstState st = state[b];
    if (step_kind(st.step) & kmask) {
        double sum = 0.0, mx = -1.0;
        int mi = (int) n, flags = 0;
        for (long long i = lane; i < nparts; i += 64) {
            const EstPart p = parts[b * nparts + i];
            sum += p.sum; argmax_merge(mx, mi, p.max, p.idx); flags |= p.flags;
        }
        wave_merge(sum, mx, mi, flags);
        if (lane == 0) {
            const double *x = X + b * n;
            if (flags & 1) {
                st.est = HUGE_VAL; st.step = 0;
            } else if (st.step == 1) {                   // J1: x = A^-1 (1/n) 1
                if (n == 1) { st.est = fabs(x[0]); st.step = 0; }
                else { st.est = sum; st.sbuf ^= 1; st.step = 2; }
            } else if (st.step == 2) {                   // J2: x = A^-T s
                st.j = mi; st.iter = 2; st.step = 3;
            } else if (st.step == 3) {                   // J3: x = A^-1 e_j
                const double estold = st.est;
                st.est = sum;
                if (!(flags & 2) || st.est <= estold) st.step = 5;      // repeated sign vector, or no growth: final stage
                else { st.sbuf ^= 1; st.step = 4; }
            } else if (st.step == 4) {                   // J4: x = A^-T s
                const int jlast = st.j;
                st.j = mi;
                if (x[jlast] != mx && st.iter < 5) { st.iter += 1; st.step = 3; }
                else st.step = 5;
            } else {                                     // J5: x = A^-1 alt
                const double t = 2.0 * (sum / (double) (3 * n));
                if (t > st.est) st.est = t;
                st.step = 0;
            }
            state[b] = st;
        }
    }
    if (lane == 0) {
        const int k = step_kind(st.step);
        if (k) atomicAdd(&cnt[k - 1], 1u);
    }
}

__global__ void __launch_bounds__(256)
k_est_finalize(const EstState *__restrict__ state, long long batch, double *__restrict__ cond, double *__restrict__ inv_norm)
{
    for (long long b = (long long) blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (long long) gridDim.x * blockDim.x) {
        const EstState s = state[b];
        cond[b] = s.anorm * s.est;
        if (inv_norm) inv_norm[b] = s.est;
    }
}

// sign and log|det| from the pivots: diag[j] = virtual pool offset of pivot j's diagonal, read through the same
// per-matrix / interleaved decode as k_extract.  LU: det A = prod u_jj; Cholesky: sign +1, 2 sum log l_jj.  A zero pivot
// gives (0, -inf) as numpy.linalg.slogdet does; a NaN propagates into log|det|.  One workgroup per matrix.
__global__ void __launch_bounds__(EST_NT)
k_slogdet(const double *__restrict__ pool_il, const double *__restrict__ pool_pm, long long il_len, long long pm_stride,
          const long long *__restrict__ diag, long long n, int cholesky, double *__restrict__ sign_out,
          double *__restrict__ logabs_out)
{
    __shared__ double w_acc[EST_WAVES];
    __shared__ int w_neg[EST_WAVES], w_zero[EST_WAVES];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *vil = pool_il + (b >> 6) * 64 * il_len + (b & 63);
    const double *vpm = pool_pm + b * pm_stride;
    double acc = 0.0;
    int neg = 0, zero = 0;
    for (long long i = tid; i < n; i += EST_NT) {
        const long long o = diag[i];
        const double v = (o < il_len) ? vil[o * 64] : vpm[o];
        neg ^= (v < 0.0) ? 1 : 0;
        zero |= (v == 0.0) ? 1 : 0;
        acc += log(fabs(v));
    }
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off);
        neg ^= __shfl_xor(neg, off);
        zero |= __shfl_xor(zero, off);
    }
    if (lane == 0) { w_acc[wv] = acc; w_neg[wv] = neg; w_zero[wv] = zero; }
    __syncthreads();
    if (tid == 0) {
        acc = 0.0; neg = 0; zero = 0;
        for (int w = 0; w < EST_WAVES; ++w) { acc += w_acc[w]; neg ^= w_neg[w]; zero |= w_zero[w]; }
        if (zero) { sign_out[b] = 0.0; logabs_out[b] = -HUGE_VAL; }
        else if (cholesky) { sign_out[b] = 1.0; logabs_out[b] = 2.0 * acc; }
        else { sign_out[b] = neg ? -1.0 : 1.0; logabs_out[b] = acc; }
    }
}

#define CS3_EST_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

static unsigned grid_x(long long work, int block, long long cap)
{
    return (unsigned) std::max<long long>(1, std::min<long long>((work + block - 1) / block, cap));
}

hipError_t launch_est_start(const int *Cp, const int *Cmap, const double *Ax, long long n, long long nnz_a, long long batch,
                            EstPart *parts, EstState *state, hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    const long long np = norm_chunks(n);
    hipLaunchKernelGGL(k_est_colsums, dim3((unsigned) np, (unsigned) batch), dim3(PART_NT), 0, st, Cp, Cmap, Ax, n, nnz_a, parts);
    CS3_EST_CHECK();
    hipLaunchKernelGGL(k_est_init, dim3((unsigned) batch), dim3(64), 0, st, parts, np, state);
    CS3_EST_CHECK();
    return hipSuccess;
}

hipError_t launch_est_prepare(const EstState *state, const signed char *S, double *X, long long n, long long batch, int kmask,
                              unsigned *cnt, hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(k_est_prepare, dim3(grid_x(n, 256, 256), (unsigned) batch), dim3(256), 0, st, state, S, X, n, batch, kmask,
                       cnt);
    CS3_EST_CHECK();
    return hipSuccess;
}

hipError_t launch_est_consume(EstState *state, signed char *S, const double *X, long long n, long long batch, int kmask,
                              EstPart *parts, unsigned *cnt, hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    const long long np = est_chunks(n);
    hipLaunchKernelGGL(k_est_partial, dim3((unsigned) np, (unsigned) batch), dim3(PART_NT), 0, st, state, S, X, n, batch, kmask,
                       parts);
    CS3_EST_CHECK();
    hipLaunchKernelGGL(k_est_finish, dim3((unsigned) batch), dim3(64), 0, st, state, X, n, np, kmask, parts, cnt);
    CS3_EST_CHECK();
    return hipSuccess;
}

hipError_t launch_est_finalize(const EstState *state, long long batch, double *cond, double *inv_norm, hipStream_t st)
{
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(k_est_finalize, dim3(grid_x(batch, 256, 1024)), dim3(256), 0, st, state, batch, cond, inv_norm);
    CS3_EST_CHECK();
    return hipSuccess;
}

hipError_t launch_slogdet(const DeviceFactor &D, const long long *diag, double *sign, double *logabs, hipStream_t st)
{
    if (D.batch == 0) return hipSuccess;
    hipLaunchKernelGGL(k_slogdet, dim3((unsigned) D.batch), dim3(EST_NT), 0, st, D.pool_il, D.pool_pm, D.il_len, D.pm_stride,
                       diag, D.n, D.kind == CS3_CHOLESKY ? 1 : 0, sign, logabs);
    CS3_EST_CHECK();
    return hipSuccess;
}

}  // namespace cs3
