// Selected inversion (cs3_selinv_*): Z = (Q' A Q)^-1 on the pattern of L + U from the factors a handle holds, one dense
// r x r block Zfront per front in a second pool, by the Takahashi recurrences, parents before children.  For a front with
// pivots P (w of them) and update rows C (c = r - w), with X = L21 L11^-1 and Y = U11^-1 U12:
//
//     Z_CC = the parent's Zfront at (rel[i], rel[j])        Z_CP = -Z_CC X        Z_PC = -Y Z_CC
//     Z_PP = U11^-1 L11^-1 - Y Z_CP
//
// Cholesky runs the same recurrences with U = L' (L11 is not unit then); Z comes out symmetric up to rounding.
//
//   k_selinv_lds<KIND, 64>    fronts of order <= 32: one wave per front, four fronts per workgroup
//   k_selinv_lds<KIND, 256>   fronts of order <= 136: one workgroup per front
//       the r x r image [L11\U11, U12; L21, Z_CC] sits in LDS; Y, U11^-1 and then [U11^-1 L11^-1; X] are formed in place,
//       the three products by v_mfma_f64_16x16x4 (selinv_tile)
//   k_selinv_big_prep / k_selinv_big_product<1> / <2>      larger fronts, three launches, many workgroups per front:
//       X, Y and U11^-1 L11^-1 by slices of 16 vectors in chunks of 64 pivots (tri_slice) and the gather of Z_CC;
//       Z_CP and Z_PC; Z_PP.  They read the factors in the pool and write Zfront and a work buffer: nothing is in place.
//   k_selinv_gather           out[e] = zpool[map[e]]
//
// Every entry of Z is written once by the lane that owns it and every sum has a fixed order: the same bits on every run.
// There are no atomics.  blockIdx.y is the matrix of the batch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_devfn.hpp"

namespace cs3 {

namespace {

constexpr int WAVE_IMAGE = (SELINV_WAVE_R | 1) * SELINV_WAVE_R;     // doubles of one wave's image (leading dimension r | 1)
constexpr int XS_LD = SELINV_DIAG + 1;                              // LDS rows of tri_slice: the reads along a column spread over the banks
static_assert(SELINV_LDS_R <= 256 && SELINV_WAVE_R <= 64, "a thread owns one row of the image");
static_assert(((SELINV_LDS_R | 1) * SELINV_LDS_R) * 8 <= 160 * 1024, "the image of the largest LDS front");
static_assert(SELINV_SLICE * 16 == 256 && SELINV_DIAG == 64, "the thread map of tri_slice");

// One 16 x 16 tile of  acc - P Q  (P: ni x nk, Q: nk x nj), computed transposed as schur_tiles does (A operand = Q, B operand
// = -P): the lane ends up with entry (i0 + (lane & 15), j0 + (lane >> 4) + 4 v) in acc[v] and passes them in the same places.
// p(i, k) and q(k, j) are only called inside [0, ni) x [0, nk) x [0, nj): rows and columns past the edge repeat the last one
// (they reach outputs nobody takes), pivots past nk contribute zero.
template <class P, class Q>
__device__ __forceinline__ cs3_double4 selinv_tile(cs3_double4 acc, int i0, int j0, int ni, int nj, int nk, P p, Q q)
{
    const int lane = threadIdx.x & 63, mi = lane & 15, mq = lane >> 4;
    const int i = min(i0 + mi, ni - 1), j = min(j0 + mi, nj - 1);
    for (int k0 = 0; k0 < nk; k0 += 4) {                        // (wave-uniform)
        const int k = k0 + mq;
        const bool kin = k < nk;
        const int kc = kin ? k : 0;
        const double a = q(kc, j), b = p(i, kc);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kin ? a : 0.0, kin ? -b : 0.0, acc, 0, 0, 0);
    }
    return acc;
}

// out(i, j, value) for the entries of the tile that exist
template <class Out>
__device__ __forceinline__ void selinv_tile_store(const cs3_double4 &acc, int i0, int j0, int ni, int nj, Out out)
{
    const int lane = threadIdx.x & 63, i = i0 + (lane & 15);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int j = j0 + (lane >> 4) + 4 * v;
        if (i < ni && j < nj) out(i, j, acc[v]);
    }
}

template <int NT>
__device__ __forceinline__ void group_sync()
{
    if (NT > 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();
}

// One front whose image F (column-major, leading dimension ld = r | 1) fits the LDS, by a group of NT threads (t: the
// thread's index in it) that is `nwaves` waves.  A thread owns row t of the image in the two in-place sweeps.
template <int KIND, int NT>
__device__ __forceinline__ void selinv_front_lds(const SelFront &d, const double *__restrict__ pool, double *zpool,
                                                 const int *__restrict__ rel_idx, double *F, int t, int wave, int nwaves)
{
    const int r = d.r, w = d.w, c = r - w, ld = r | 1;
    const double *__restrict__ L = pool + d.lpan;
    const double *__restrict__ U = pool + d.upan;
    const int *__restrict__ rel = rel_idx + d.rel;
    const double *ZP = zpool + d.zpar;
    double *Z = zpool + d.z;
    // the image: LU  [L11\U11, U12; L21, Z_CC];  Cholesky the same with U = L' mirrored from the panel
    for (int e = t; e < r * w; e += NT) {
        const int i = e % r, k = e / r;
        if (KIND == CS3_LU) F[i + k * ld] = L[e];
        else if (i >= k) { const double v = L[e]; F[i + k * ld] = v; F[k + i * ld] = v; }
    }
    if (KIND == CS3_LU)
        for (int e = t; e < w * c; e += NT) {
            const int k = e % w, j = e / w;
            F[k + (w + j) * ld] = U[k * d.u_sk + j * d.u_sj];
        }
    for (int e = t; e < c * c; e += NT) {
        const int i = e % c, j = e / c;
        F[(w + i) + (w + j) * ld] = ZP[rel[i] + (long long) rel[j] * d.rpar];
    }
    group_sync<NT>();
    // Y = U11^-1 U12 in place, a thread per column (U11 is only read)
    for (int j = w + t; j < r; j += NT) {
        double *y = F + j * ld;
        for (int k = w - 1; k >= 0; --k) {
            double s = y[k];
            for (int m = k + 1; m < w; ++m) s -= F[k + m * ld] * y[m];
            y[k] = s / F[k + k * ld];
        }
    }
    group_sync<NT>();
    // V = U11^-1 in place, row t by thread t, column by column: V(t, j) = (delta_tj - sum_{t <= k < j} V(t, k) U(k, j)) / U(j, j).
    // Step j reads column j of U and writes column j of V behind the barrier.
    for (int j = 0; j < w; ++j) {
        double v = 0.0;
        if (t <= j) {
            double s = (t == j) ? 1.0 : 0.0;
            for (int k = t; k < j; ++k) s -= F[t + k * ld] * F[k + j * ld];
            v = s / F[j + j * ld];
        }
        group_sync<NT>();
        if (t <= j) F[t + j * ld] = v;
    }
    group_sync<NT>();
    // [U11^-1 L11^-1; X] = [V; L21] L11^-1 in place, row t by thread t, columns from the right:
    //   T(t, j) = (S(t, j) - sum_{k > j} T(t, k) L(k, j)) / L(j, j),  S = V on and above the diagonal, 0 below it, L21 under the block.
    // Step j reads column j of L11 (Cholesky: 1 / L(j, j) is V(j, j), still in place) and overwrites it behind the barrier.
    for (int j = w - 1; j >= 0; --j) {
        double s = 0.0;
        if (t < r) {
            s = (t <= j || t >= w) ? F[t + j * ld] : 0.0;
            for (int k = j + 1; k < w; ++k) s -= F[t + k * ld] * F[k + j * ld];
            if (KIND == CS3_CHOLESKY) s *= F[j + j * ld];
        }
        group_sync<NT>();
        if (t < r) F[t + j * ld] = s;
    }
    group_sync<NT>();
    // Z_CC as gathered, Z_CP = -Z_CC X, Z_PC = -Y Z_CC: 16 x 16 tiles dealt to the waves
    for (int e = t; e < c * c; e += NT) {
        const int i = e % c, j = e / c;
        Z[(w + i) + (long long) (w + j) * r] = F[(w + i) + (w + j) * ld];
    }
    const int tc = (c + SELINV_TILE - 1) / SELINV_TILE, tw = (w + SELINV_TILE - 1) / SELINV_TILE;
    const cs3_double4 zero = {0.0, 0.0, 0.0, 0.0};
    for (int tile = wave; tile < 2 * tc * tw; tile += nwaves) {          // (wave-uniform)
        const int half = tile / (tc * tw), tt = tile % (tc * tw);
        if (half == 0) {
            const int i0 = (tt % tc) * SELINV_TILE, j0 = (tt / tc) * SELINV_TILE;
            const cs3_double4 acc = selinv_tile(zero, i0, j0, c, w, c,
                                                [&](int i, int k) { return F[(w + i) + (w + k) * ld]; },
                                                [&](int k, int j) { return F[(w + k) + j * ld]; });
            selinv_tile_store(acc, i0, j0, c, w, [&](int i, int j, double v) { Z[(w + i) + (long long) j * r] = v; });
        } else {
            const int i0 = (tt % tw) * SELINV_TILE, j0 = (tt / tw) * SELINV_TILE;
            const cs3_double4 acc = selinv_tile(zero, i0, j0, w, c, c,
                                                [&](int i, int k) { return F[i + (w + k) * ld]; },
                                                [&](int k, int j) { return F[(w + k) + (w + j) * ld]; });
            selinv_tile_store(acc, i0, j0, w, c, [&](int i, int j, double v) { Z[i + (long long) (w + j) * r] = v; });
        }
    }
    __threadfence();                                            // Z_CP is read back from Zfront below, by other lanes
    group_sync<NT>();
    // Z_PP = U11^-1 L11^-1 - Y Z_CP
    const int lane = threadIdx.x & 63;
    for (int tile = wave; tile < tw * tw; tile += nwaves) {
        const int i0 = (tile % tw) * SELINV_TILE, j0 = (tile / tw) * SELINV_TILE;
        cs3_double4 acc;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = F[min(i0 + (lane & 15), w - 1) + min(j0 + (lane >> 4) + 4 * v, w - 1) * ld];
        acc = selinv_tile(acc, i0, j0, w, w, c,
                          [&](int i, int k) { return F[i + (w + k) * ld]; },
                          [&](int k, int j) { return Z[(w + k) + (long long) j * r]; });
        selinv_tile_store(acc, i0, j0, w, w, [&](int i, int j, double v) { Z[i + (long long) j * r] = v; });
    }
}

template <int KIND, int NT>
__global__ void __launch_bounds__(256)
k_selinv_lds(SelinvView V, int first, int count)
{
    extern __shared__ double selinv_lds[];
    const int wv = threadIdx.x >> 6;
    const int front = (NT == 64) ? blockIdx.x * 4 + wv : blockIdx.x;
    if (front >= count) return;                                 // (a whole wave, and NT == 64 has no block barrier)
    const SelFront d = V.fronts[first + front];
    const double *pool = V.pool + (long long) blockIdx.y * V.pool_stride;
    double *zpool = V.zpool + (long long) blockIdx.y * V.z_stride;
    if (NT == 64) selinv_front_lds<KIND, 64>(d, pool, zpool, V.rel_idx, selinv_lds + wv * WAVE_IMAGE, threadIdx.x & 63, 0, 1);
    else selinv_front_lds<KIND, 256>(d, pool, zpool, V.rel_idx, selinv_lds, threadIdx.x, wv, 4);
}

// ---- fronts beyond the LDS ----------------------------------------------------------------------------------------------
// The factors of a big front as the solves read them: L11 (diagonal 1 for LU), U11 and U12 (Cholesky: L' mirrored).
template <int KIND>
struct BigFactors {
    const double *__restrict__ L, *__restrict__ U;
    int r, w, u_sk, u_sj;
    __device__ __forceinline__ double l11(int i, int j) const { return (KIND == CS3_LU && i == j) ? 1.0 : L[i + (long long) j * r]; }      // i >= j
    __device__ __forceinline__ double l21(int i, int j) const { return L[(w + i) + (long long) j * r]; }
    __device__ __forceinline__ double u11(int i, int j) const { return (KIND == CS3_LU) ? L[i + (long long) j * r] : L[j + (long long) i * r]; }   // i <= j
    __device__ __forceinline__ double u12(int i, int j) const
    {
        return (KIND == CS3_LU) ? U[(long long) i * u_sk + (long long) j * u_sj] : L[(w + j) + (long long) i * r];
    }
};

// SELINV_SLICE vectors x with  sum_k x_k M(k, j) = b_j  for a triangular M of order w whose column j holds rows k >= j:
//   x_j = (b_j - sum_{k > j} x_k M(k, j)) / M(j, j),  j descending,
// by one workgroup of 256 threads, thread (v, t) = (tid / 16, tid % 16): chunks of 64 columns from the right; a chunk first
// takes the finished chunks' part of the sum (thread (v, t): columns t, t + 16, t + 32, t + 48 of the chunk, k ascending),
// then is solved against its diagonal block in LDS (mb), one column per step.  m(k, j) is the matrix, b(v, j) the right-hand
// sides, xl(v, k) / xs(v, j, value) read and write the solution (the same memory: what a chunk stores the later ones load).
// nv <= 16 vectors exist; the others repeat the last one and store nothing.
template <class M, class B, class XL, class XS>
__device__ __forceinline__ void tri_slice(int w, int nv, M m, B b, XL xl, XS xs, double *xb, double *mb)
{
    const int tid = threadIdx.x, v = tid >> 4, t = tid & 15;
    const int vc = min(v, nv - 1);
    for (int j0 = ((w - 1) / SELINV_DIAG) * SELINV_DIAG; j0 >= 0; j0 -= SELINV_DIAG) {
        const int jw = min(SELINV_DIAG, w - j0);
        for (int e = tid; e < SELINV_DIAG * SELINV_DIAG; e += 256) {
            const int a = e / SELINV_DIAG, bb = e % SELINV_DIAG;        // mb[a][bb] = M(j0 + a, j0 + bb), the triangle a >= bb
            mb[a * XS_LD + bb] = (a < jw && bb <= a) ? m(j0 + a, j0 + bb) : 0.0;
        }
        double acc[4];
        int jc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { jc[q] = min(j0 + t + 16 * q, w - 1); acc[q] = b(vc, jc[q]); }
        for (int k = j0 + SELINV_DIAG; k < w; ++k) {
            const double x = xl(vc, k);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] -= x * m(k, jc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) xb[v * XS_LD + t + 16 * q] = acc[q];
        __syncthreads();
        for (int jl = jw - 1; jl >= 0; --jl) {                  // (uniform over the workgroup)
            const double x = xb[v * XS_LD + jl] / mb[jl * XS_LD + jl];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = t + 16 * q;
                if (cl < jl) xb[v * XS_LD + cl] -= x * mb[jl * XS_LD + cl];
            }
            if (t == (jl & 15) && v < nv) xs(v, j0 + jl, x);
            __syncthreads();
        }
        __threadfence();                                        // the next chunk loads what other lanes stored here
        __syncthreads();
    }
}

// First launch of a group of big fronts (blockIdx.z = front): workgroup b of a front is, in this order, a slice of rows
// of X = L21 L11^-1, a slice of columns of Y = U11^-1 U12, a slice of columns of U11^-1 L11^-1 (L11 t = e_j, then U11 z = t, in
// the front's Z_PP), or a part of the gather of Z_CC from the parent.
template <int KIND>
__global__ void __launch_bounds__(256)
k_selinv_big_prep(SelinvView V, int first)
{
    __shared__ double xb[SELINV_SLICE * XS_LD], mb[SELINV_DIAG * XS_LD];
    const SelFront d = V.fronts[first + blockIdx.z];
    const int r = d.r, w = d.w, c = r - w;
    const double *pool = V.pool + (long long) blockIdx.y * V.pool_stride;
    double *zpool = V.zpool + (long long) blockIdx.y * V.z_stride;
    double *X = V.work + (long long) blockIdx.y * V.work_stride + d.wk, *Y = X + (long long) c * w;
    double *Z = zpool + d.z;
    const BigFactors<KIND> f{pool + d.lpan, pool + d.upan, r, w, d.u_sk, d.u_sj};
    const int nsc = (c + SELINV_SLICE - 1) / SELINV_SLICE, nsw = (w + SELINV_SLICE - 1) / SELINV_SLICE;
    int blk = blockIdx.x;
    if (blk < nsc) {
        const int i0 = blk * SELINV_SLICE;
        tri_slice(w, min(SELINV_SLICE, c - i0),
                  [&](int k, int j) { return f.l11(k, j); },
                  [&](int v, int j) { return f.l21(i0 + v, j); },
                  [&](int v, int k) { return X[(i0 + v) + (long long) k * c]; },
                  [&](int v, int j, double x) { X[(i0 + v) + (long long) j * c] = x; }, xb, mb);
        return;
    }
    blk -= nsc;
    if (blk < nsc) {
        const int j0 = blk * SELINV_SLICE;
        tri_slice(w, min(SELINV_SLICE, c - j0),
                  [&](int k, int j) { return f.u11(j, k); },
                  [&](int v, int j) { return f.u12(j, j0 + v); },
                  [&](int v, int k) { return Y[k + (long long) (j0 + v) * w]; },
                  [&](int v, int j, double x) { Y[j + (long long) (j0 + v) * w] = x; }, xb, mb);
        return;
    }
    blk -= nsc;
    if (blk < nsw) {
        const int j0 = blk * SELINV_SLICE, last = w - 1;
        // L11 t = e_j runs forwards: the same recurrence on the reversed indices
        tri_slice(w, min(SELINV_SLICE, w - j0),
                  [&](int k, int j) { return f.l11(last - j, last - k); },
                  [&](int v, int j) { return (last - j == j0 + v) ? 1.0 : 0.0; },
                  [&](int v, int k) { return Z[(last - k) + (long long) (j0 + v) * r]; },
                  [&](int v, int j, double x) { Z[(last - j) + (long long) (j0 + v) * r] = x; }, xb, mb);
        tri_slice(w, min(SELINV_SLICE, w - j0),
                  [&](int k, int j) { return f.u11(j, k); },
                  [&](int v, int j) { return Z[j + (long long) (j0 + v) * r]; },
                  [&](int v, int k) { return Z[k + (long long) (j0 + v) * r]; },
                  [&](int v, int j, double x) { Z[j + (long long) (j0 + v) * r] = x; }, xb, mb);
        return;
    }
    blk -= nsw;
    const int *__restrict__ rel = V.rel_idx + d.rel;
    const double *ZP = zpool + d.zpar;
    const long long stride = 256ll * (gridDim.x - (2 * nsc + nsw));
    for (long long e = 256ll * blk + threadIdx.x; e < (long long) c * c; e += stride) {
        const int i = (int) (e % c), j = (int) (e / c);
        Z[(w + i) + (long long) (w + j) * r] = ZP[rel[i] + (long long) rel[j] * d.rpar];
    }
}

// PHASE 1: Z_CP = -Z_CC X and Z_PC = -Y Z_CC; PHASE 2: Z_PP = (U11^-1 L11^-1, in place) - Y Z_CP.  One 16 x 16 tile per wave.
template <int PHASE>
__global__ void __launch_bounds__(256)
k_selinv_big_product(SelinvView V, int first)
{
    const SelFront d = V.fronts[first + blockIdx.z];
    const int r = d.r, w = d.w, c = r - w;
    const double *X = V.work + (long long) blockIdx.y * V.work_stride + d.wk, *Y = X + (long long) c * w;
    double *Z = V.zpool + (long long) blockIdx.y * V.z_stride + d.z;
    const int tc = (c + SELINV_TILE - 1) / SELINV_TILE, tw = (w + SELINV_TILE - 1) / SELINV_TILE;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c == 0) return;
    if (PHASE == 1) {
        if (tile >= 2 * tc * tw) return;
        const int half = tile / (tc * tw), tt = tile % (tc * tw);
        const cs3_double4 zero = {0.0, 0.0, 0.0, 0.0};
        if (half == 0) {
            const int i0 = (tt % tc) * SELINV_TILE, j0 = (tt / tc) * SELINV_TILE;
            const cs3_double4 acc = selinv_tile(zero, i0, j0, c, w, c,
                                                [&](int i, int k) { return Z[(w + i) + (long long) (w + k) * r]; },
                                                [&](int k, int j) { return X[k + (long long) j * c]; });
            selinv_tile_store(acc, i0, j0, c, w, [&](int i, int j, double v) { Z[(w + i) + (long long) j * r] = v; });
        } else {
            const int i0 = (tt % tw) * SELINV_TILE, j0 = (tt / tw) * SELINV_TILE;
            const cs3_double4 acc = selinv_tile(zero, i0, j0, w, c, c,
                                                [&](int i, int k) { return Y[i + (long long) k * w]; },
                                                [&](int k, int j) { return Z[(w + k) + (long long) (w + j) * r]; });
            selinv_tile_store(acc, i0, j0, w, c, [&](int i, int j, double v) { Z[i + (long long) (w + j) * r] = v; });
        }
    } else {
        if (tile >= tw * tw) return;
        const int i0 = (tile % tw) * SELINV_TILE, j0 = (tile / tw) * SELINV_TILE;
        cs3_double4 acc;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = Z[min(i0 + (lane & 15), w - 1) + (long long) min(j0 + (lane >> 4) + 4 * v, w - 1) * r];
        acc = selinv_tile(acc, i0, j0, w, w, c,
                          [&](int i, int k) { return Y[i + (long long) k * w]; },
                          [&](int k, int j) { return Z[(w + k) + (long long) j * r]; });
        selinv_tile_store(acc, i0, j0, w, w, [&](int i, int j, double v) { Z[i + (long long) j * r] = v; });
    }
}

__global__ void __launch_bounds__(256)
k_selinv_gather(const double *__restrict__ zpool, long long z_stride, const long long *__restrict__ map, double *__restrict__ out,
                long long count)
{
    const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
    if (e < count) out[(long long) blockIdx.y * count + e] = zpool[(long long) blockIdx.y * z_stride + map[e]];
}

}  // namespace

#define CS3_SELINV_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t prepare_selinv_kernels()
{
    const void *fns[] = {(const void *) k_selinv_lds<CS3_LU, 256>, (const void *) k_selinv_lds<CS3_CHOLESKY, 256>};
    for (const void *f : fns) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_selinv_group(int kind, const SelinvView &V, const SelinvGroup &g, hipStream_t st)
{
    if (g.count == 0 || V.batch == 0) return hipSuccess;
    const unsigned by = (unsigned) V.batch;
    return with_kind(kind, [&](auto K) -> hipError_t {
        constexpr int KIND = decltype(K)::value;
        if (g.cls == SELINV_WAVE) {
            if (g.max_r > SELINV_WAVE_R) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_selinv_lds<KIND, 64>), dim3((unsigned) ((g.count + 3) / 4), by), dim3(256),
                               4 * WAVE_IMAGE * sizeof(double), st, V, g.first, g.count);
        } else if (g.cls == SELINV_LDS) {
            if (g.max_r > SELINV_LDS_R) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_selinv_lds<KIND, 256>), dim3((unsigned) g.count, by), dim3(256),
                               (size_t) (g.max_r | 1) * g.max_r * sizeof(double), st, V, g.first, g.count);
        } else {
            if (g.count > 65535) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_selinv_big_prep<KIND>), dim3(g.grid_prep, by, (unsigned) g.count), dim3(256), 0, st, V, g.first);
            CS3_SELINV_CHECK();
            hipLaunchKernelGGL((k_selinv_big_product<1>), dim3(g.grid_cross, by, (unsigned) g.count), dim3(256), 0, st, V, g.first);
            CS3_SELINV_CHECK();
            hipLaunchKernelGGL((k_selinv_big_product<2>), dim3(g.grid_pivot, by, (unsigned) g.count), dim3(256), 0, st, V, g.first);
        }
        CS3_SELINV_CHECK();
        return hipSuccess;
    });
}

hipError_t launch_selinv_gather(const double *zpool, long long z_stride, const long long *map, double *out, long long count,
                                long long batch, hipStream_t st)
{
    if (count == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(k_selinv_gather, dim3((unsigned) ((count + 255) / 256), (unsigned) batch), dim3(256), 0, st, zpool, z_stride,
                       map, out, count);
    CS3_SELINV_CHECK();
    return hipSuccess;
}

}  // namespace cs3
