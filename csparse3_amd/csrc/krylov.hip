// The vector layer of restarted GMRES on the factors a handle holds (cs3_gmres*): norms, multi-dots, basis updates and
// the small Hessenberg problems of batch * k systems at once.  api.cpp drives it: per iteration one solve and one product
// of the handle serve every system, the kernels here do the rest.
//
// Every vector is [batch][n, k] row-major; system s = b * k + t is column t of matrix b and is served by ONE thread
// column: a workgroup is TX x (256 / TX) threads, TX = min(pow2ceil(k), 64), tx = right-hand side inside a tile of 64,
// ty strides over the rows of a chunk of KRY_CHUNK rows, so loads stay contiguous along [row][t].  Grid: one workgroup
// per (matrix, tile of right-hand sides, chunk), flattened into x.
//
// Reductions run in a fixed order: a per-thread strided loop over the rows of a chunk, xor butterflies inside a wave, the
// four waves in index order, then the chunks in index order by the kernel that consumes them.  No float atomics; the only
// integer atomic is the count of active systems.  Results are bitwise reproducible and do not depend on the grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "cs3_device.hpp"

namespace cs3 {

namespace {

constexpr int KRY_NT = 256;
constexpr int KRY_NI = 8;               // basis vectors per pass over w in the multi-dot

struct Tile {                           // what a thread of the streaming kernels serves
    long long s;                        // its system
    long long base;                     // offset of (row 0, its column) in a vector
    long long r0, r1, c;                // rows of its chunk, the chunk
    int tx, ty, ny;                     // ny = 256 / TX
    bool valid;                         // its column exists (t < k)
};

__device__ __forceinline__ Tile tile_of(long long n, long long k, long long chunks, int log2tx)
{
    const long long ktiles = (k + KRY_RHS_TILE - 1) / KRY_RHS_TILE;
    const long long bid = blockIdx.x;
    Tile T;
    T.c = bid % chunks;
    const long long kt = (bid / chunks) % ktiles, b = bid / (chunks * ktiles);
    T.tx = threadIdx.x & ((1 << log2tx) - 1);
    T.ty = threadIdx.x >> log2tx;
    T.ny = KRY_NT >> log2tx;
    const long long t = kt * KRY_RHS_TILE + T.tx;
    T.valid = t < k;
    T.s = b * k + (T.valid ? t : 0);
    T.base = b * n * k + (T.valid ? t : 0);
    T.r0 = T.c * KRY_CHUNK;
    T.r1 = std::min(n, T.r0 + KRY_CHUNK);
    return T;
}

// The sum of `a` over the threads of the workgroup that share tx, in a fixed order; the result is valid in the threads
// tid < TX.  red: 4 * 64 doubles of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ double sum_over_ty(double a, int log2tx, double *red)
{
    const int tid = threadIdx.x, lane = tid & 63, tx_count = 1 << log2tx;
    for (int off = 32; off >= tx_count; off >>= 1) a += __shfl_xor(a, off);
    if (lane < tx_count) red[(tid >> 6) * 64 + lane] = a;
    __syncthreads();
    double sum = 0.0;
    if (tid < tx_count) sum = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
    __syncthreads();
    return sum;
}

__device__ __forceinline__ double sum_chunks(const double *p, long long chunks)
{
    double sum = 0.0;
    for (long long c = 0; c < chunks; ++c) sum += p[c];
    return sum;
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= DBL_MAX; }

}  // namespace

// Stage 1 of the norms at the start of a cycle: the partial sums of r^2 (and of b^2, first cycle) over one chunk.  Clears
// the counters of the coming cycle.
__global__ void __launch_bounds__(KRY_NT)
k_kry_norms(KryWork K, const double *__restrict__ B, int log2tx)
{
    __shared__ double red[4 * 64];
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    if (blockIdx.x == 0 && (int) threadIdx.x < K.restart + 2) K.cnt[threadIdx.x] = 0u;
    const long long nsys = K.batch * K.k;
    double r2 = 0.0, b2 = 0.0;
    if (T.valid) {
        for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
            const double r = K.W[T.base + row * K.k];
            r2 += r * r;
            if (B) { const double b = B[T.base + row * K.k]; b2 += b * b; }
        }
    }
    r2 = sum_over_ty(r2, log2tx, red);
    if (B) b2 = sum_over_ty(b2, log2tx, red);
    if ((int) threadIdx.x < (1 << log2tx) && T.valid) {
        K.nparts[T.s * K.chunks + T.c] = r2;
        if (B) K.nparts[(nsys + T.s) * K.chunks + T.c] = b2;
    }
}

// Stage 2 and the state of every system for the coming cycle.  One thread per system.
__global__ void __launch_bounds__(64)
k_kry_begin(KryWork K, int first, double rtol, int max_iters)
{
    const long long nsys = K.batch * K.k, s = (long long) blockIdx.x * 64 + threadIdx.x;
    if (s >= nsys) return;
    KrySys S = K.sys[s];
    if (first) {
        S.status = KRY_RUN; S.iters = 0; S.est = 0.0; S.relres = 0.0;
        S.bnorm = sqrt(sum_chunks(K.nparts + (nsys + s) * K.chunks, K.chunks));
    }
    S.active = 0; S.part = 0; S.inv = 0.0; S.ncols = 0;
    if (S.status == KRY_RUN) {
        const double rn = sqrt(sum_chunks(K.nparts + s * K.chunks, K.chunks));
        if (S.bnorm == 0.0) {                            // x = 0: ncols -1 has k_kry_scale zero the column
            S.status = KRY_DONE; S.relres = 0.0; S.ncols = -1;
        } else if (!is_finite(rn) || !is_finite(S.bnorm)) {
            S.status = KRY_BAD; S.relres = NAN;
        } else {
            S.relres = rn / S.bnorm;
            if (S.relres <= rtol || S.iters >= max_iters) {
                S.status = KRY_DONE;
            } else {
                S.active = 1; S.part = 1; S.inv = 1.0 / rn;
                K.g[s * (K.restart + 1)] = rn;
                atomicAdd(&K.cnt[0], 1u);
            }
        }
    }
    K.sys[s] = S;
}

// dst = Z = w * inv for an active system, exact zeros for every other (a frozen system contributes nothing further,
// whatever its w holds).  X (the start of the first cycle only): the columns of zero right-hand sides become zero.
__global__ void __launch_bounds__(KRY_NT)
k_kry_scale(KryWork K, double *__restrict__ dst, double *__restrict__ X, int log2tx)
{
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    if (!T.valid) return;
    const KrySys S = K.sys[T.s];
    for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
        const long long at = T.base + row * K.k;
        const double v = S.active ? K.W[at] * S.inv : 0.0;
        dst[at] = v;
        K.Z[at] = v;
        if (X && S.ncols < 0) X[at] = 0.0;
    }
}

// The multi-dot h_i = v_i . w for i <= j over one chunk, KRY_NI basis vectors per pass over w.
__global__ void __launch_bounds__(KRY_NT)
k_kry_dot(KryWork K, int j, int pass, int log2tx)
{
    __shared__ double red[4 * 64];
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    const long long nsys = K.batch * K.k, total = K.batch * K.n * K.k;
    double *out = K.parts + ((long long) pass * nsys + T.s) * K.restart * K.chunks + T.c;
    for (int i0 = 0; i0 <= j; i0 += KRY_NI) {
        double acc[KRY_NI];
#pragma unroll
        for (int q = 0; q < KRY_NI; ++q) acc[q] = 0.0;
        if (T.valid) {
            for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
                const long long at = T.base + row * K.k;
                const double w = K.W[at];
#pragma unroll
                for (int q = 0; q < KRY_NI; ++q)
                    if (i0 + q <= j) acc[q] += K.V[(long long) (i0 + q) * total + at] * w;
            }
        }
#pragma unroll
        for (int q = 0; q < KRY_NI; ++q) {
            const double sum = sum_over_ty(acc[q], log2tx, red);
            if (i0 + q <= j && (int) threadIdx.x < (1 << log2tx) && T.valid) out[(long long) (i0 + q) * K.chunks] = sum;
        }
    }
}

// w -= sum_i h_i v_i over one chunk, the h_i summed over the chunks first (chunk 0 records them for the Hessenberg
// column).  NORM: the partial sums of the new ||w||^2 as well.
template <bool NORM>
__global__ void __launch_bounds__(KRY_NT)
k_kry_update(KryWork K, int j, int pass, int log2tx)
{
    __shared__ double red[4 * 64];
    __shared__ double h[KRY_MAX_RESTART][KRY_RHS_TILE];
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    const long long nsys = K.batch * K.k, total = K.batch * K.n * K.k;
    if (T.valid) {
        for (int i = T.ty; i <= j; i += T.ny) {
            const double sum = sum_chunks(K.parts + (((long long) pass * nsys + T.s) * K.restart + i) * K.chunks, K.chunks);
            h[i][T.tx] = sum;
            if (T.c == 0) K.hsum[((long long) pass * nsys + T.s) * K.restart + i] = sum;
        }
    }
    __syncthreads();
    double nrm = 0.0;
    if (T.valid) {
        for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
            const long long at = T.base + row * K.k;
            double w = K.W[at];
            for (int i = 0; i <= j; ++i) w -= h[i][T.tx] * K.V[(long long) i * total + at];
            K.W[at] = w;
            if (NORM) nrm += w * w;
        }
    }
    if (NORM) {
        nrm = sum_over_ty(nrm, log2tx, red);
        if ((int) threadIdx.x < (1 << log2tx) && T.valid) K.nparts[T.s * K.chunks + T.c] = nrm;
    }
}

// Column j of the Hessenberg matrix of every active system: both Gram-Schmidt passes added, the old rotations applied, the
// new one formed, g updated, and the decision: frozen (converged by the recurrence, lucky breakdown, out of iterations),
// bad (a non-finite entry) or active with inv = 1 / h_{j+1,j}.  One thread per system.
__global__ void __launch_bounds__(64)
k_kry_hess(KryWork K, int j, double rtol, int max_iters)
{
    const long long nsys = K.batch * K.k, s = (long long) blockIdx.x * 64 + threadIdx.x;
    if (s >= nsys) return;
    KrySys S = K.sys[s];
    if (!S.active) return;
    const int m = K.restart;
    double *Rc = K.R + (s * m + j) * m, *cs = K.cs + s * m, *sn = K.sn + s * m, *g = K.g + s * (m + 1);
    bool bad = false;
    for (int i = 0; i <= j; ++i) {
        const double hi = K.hsum[s * m + i] + K.hsum[(nsys + s) * m + i];
        Rc[i] = hi;
        bad = bad || !is_finite(hi);
    }
    const double hn = sqrt(sum_chunks(K.nparts + s * K.chunks, K.chunks));
    bad = bad || !is_finite(hn);
    double prev = Rc[0], denom = 0.0;
    if (!bad) {
        for (int i = 0; i < j; ++i) {
            const double next = Rc[i + 1];
            Rc[i] = cs[i] * prev + sn[i] * next;
            prev = cs[i] * next - sn[i] * prev;
        }
        denom = hypot(prev, hn);
        bad = !is_finite(denom) || denom == 0.0;
    }
    if (bad) {                                           // frozen alone: X keeps what the last completed cycle left
        S.status = KRY_BAD; S.relres = NAN; S.active = 0; S.part = 0; S.inv = 0.0;
        K.sys[s] = S;
        return;
    }
    const double c = prev / denom, sj = hn / denom, gj = g[j];
    Rc[j] = denom; cs[j] = c; sn[j] = sj;
    g[j + 1] = -sj * gj;
    g[j] = c * gj;
    S.iters += 1;
    S.ncols = j + 1;
    const double est = fabs(g[j + 1]);
    S.est = est / S.bnorm;
    if (est <= rtol * S.bnorm || hn == 0.0 || S.iters >= max_iters) {
        S.active = 0; S.inv = 0.0;
    } else {
        S.inv = 1.0 / hn;
        atomicAdd(&K.cnt[1 + j], 1u);
    }
    K.sys[s] = S;
}

// y from R y = g for every system that took part (zeros behind its last column).  One thread per system.
__global__ void __launch_bounds__(64)
k_kry_backsub(KryWork K)
{
    const long long nsys = K.batch * K.k, s = (long long) blockIdx.x * 64 + threadIdx.x;
    if (s >= nsys) return;
    const KrySys S = K.sys[s];
    const int m = K.restart, nc = (S.part && S.ncols > 0) ? S.ncols : 0;
    const double *R = K.R + s * m * m, *g = K.g + s * (m + 1);
    double *y = K.y + s * m;
    for (int i = nc; i < m; ++i) y[i] = 0.0;
    for (int i = nc - 1; i >= 0; --i) {
        double v = g[i];
        for (int l = i + 1; l < nc; ++l) v -= R[l * m + i] * y[l];
        y[i] = v / R[i * m + i];
    }
}

// Z = u = sum_{i < cols} y_i v_i for a system that took part, zeros for every other.
__global__ void __launch_bounds__(KRY_NT)
k_kry_combine(KryWork K, int cols, int log2tx)
{
    __shared__ double y[KRY_MAX_RESTART][KRY_RHS_TILE];
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    const long long total = K.batch * K.n * K.k;
    int nc = 0;
    if (T.valid) {
        const KrySys S = K.sys[T.s];
        nc = (S.part && S.ncols > 0) ? std::min(S.ncols, cols) : 0;
        for (int i = T.ty; i < cols; i += T.ny) y[i][T.tx] = K.y[T.s * K.restart + i];
    }
    __syncthreads();
    if (!T.valid) return;
    for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
        const long long at = T.base + row * K.k;
        double u = 0.0;
        for (int i = 0; i < nc; ++i) u += y[i][T.tx] * K.V[(long long) i * total + at];
        K.Z[at] = u;
    }
}

// X += Z for the systems that took part
__global__ void __launch_bounds__(KRY_NT)
k_kry_axpy(KryWork K, double *__restrict__ X, int log2tx)
{
    const Tile T = tile_of(K.n, K.k, K.chunks, log2tx);
    if (!T.valid) return;
    const KrySys S = K.sys[T.s];
    if (!(S.part && S.ncols > 0)) return;
    for (long long row = T.r0 + T.ty; row < T.r1; row += T.ny) {
        const long long at = T.base + row * K.k;
        X[at] += K.Z[at];
    }
}

#define CS3_KRY_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

namespace {

struct Shape { unsigned grid, sys_grid; int log2tx; bool ok; };

Shape shape_of(const KryWork &K)
{
    Shape s{};
    while ((1 << s.log2tx) < KRY_RHS_TILE && (1LL << s.log2tx) < K.k) ++s.log2tx;
    const long long ktiles = (K.k + KRY_RHS_TILE - 1) / KRY_RHS_TILE, blocks = K.batch * ktiles * K.chunks;
    const long long sys_blocks = (K.batch * K.k + 63) / 64;
    s.ok = K.n > 0 && K.batch > 0 && K.k > 0 && blocks <= 0x7fffffffLL && K.restart >= 1 && K.restart <= KRY_MAX_RESTART;
    s.grid = (unsigned) blocks;
    s.sys_grid = (unsigned) sys_blocks;
    return s;
}

}  // namespace

hipError_t launch_kry_start(const KryWork &K, const double *B, double *X, bool first, double rtol, int max_iters, hipStream_t st)
{
    const Shape s = shape_of(K);
    if (!s.ok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kry_norms, dim3(s.grid), dim3(KRY_NT), 0, st, K, first ? B : nullptr, s.log2tx);
    CS3_KRY_CHECK();
    hipLaunchKernelGGL(k_kry_begin, dim3(s.sys_grid), dim3(64), 0, st, K, first ? 1 : 0, rtol, max_iters);
    CS3_KRY_CHECK();
    hipLaunchKernelGGL(k_kry_scale, dim3(s.grid), dim3(KRY_NT), 0, st, K, K.V, first ? X : nullptr, s.log2tx);
    CS3_KRY_CHECK();
    return hipSuccess;
}

hipError_t launch_kry_step(const KryWork &K, int j, double rtol, int max_iters, hipStream_t st)
{
    const Shape s = shape_of(K);
    if (!s.ok || j < 0 || j >= K.restart) return hipErrorInvalidValue;
    const long long total = K.batch * K.n * K.k;
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(k_kry_dot, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, pass, s.log2tx);
        CS3_KRY_CHECK();
        if (pass == 0) hipLaunchKernelGGL(k_kry_update<false>, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, pass, s.log2tx);
        else hipLaunchKernelGGL(k_kry_update<true>, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, pass, s.log2tx);
        CS3_KRY_CHECK();
    }
    hipLaunchKernelGGL(k_kry_hess, dim3(s.sys_grid), dim3(64), 0, st, K, j, rtol, max_iters);
    CS3_KRY_CHECK();
    hipLaunchKernelGGL(k_kry_scale, dim3(s.grid), dim3(KRY_NT), 0, st, K, K.V + (long long) (j + 1) * total, (double *) nullptr,
                       s.log2tx);
    CS3_KRY_CHECK();
    return hipSuccess;
}

// diagnostics (tools/bench_gmres.py): one kernel of iteration j alone, on whatever the work memory holds
hipError_t launch_kry_probe(const KryWork &K, int which, int j, hipStream_t st)
{
    const Shape s = shape_of(K);
    if (!s.ok || j < 0 || j >= K.restart || which < 0 || which > 2) return hipErrorInvalidValue;
    if (which == 0) hipLaunchKernelGGL(k_kry_dot, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, 0, s.log2tx);
    else if (which == 1) hipLaunchKernelGGL(k_kry_update<false>, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, 0, s.log2tx);
    else hipLaunchKernelGGL(k_kry_update<true>, dim3(s.grid), dim3(KRY_NT), 0, st, K, j, 1, s.log2tx);
    CS3_KRY_CHECK();
    return hipSuccess;
}

hipError_t launch_kry_combine(const KryWork &K, int cols, hipStream_t st)
{
    const Shape s = shape_of(K);
    if (!s.ok || cols < 0 || cols > K.restart) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kry_backsub, dim3(s.sys_grid), dim3(64), 0, st, K);
    CS3_KRY_CHECK();
    hipLaunchKernelGGL(k_kry_combine, dim3(s.grid), dim3(KRY_NT), 0, st, K, cols, s.log2tx);
    CS3_KRY_CHECK();
    return hipSuccess;
}

hipError_t launch_kry_axpy(const KryWork &K, double *X, hipStream_t st)
{
    const Shape s = shape_of(K);
    if (!s.ok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kry_axpy, dim3(s.grid), dim3(KRY_NT), 0, st, K, X, s.log2tx);
    CS3_KRY_CHECK();
    return hipSuccess;
}

}  // namespace cs3
