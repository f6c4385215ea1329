// Many low-rank-modified systems (A + dA_c) x = b on the factors a handle holds (cs3_updates_*): the vector steps of the
// Sherman-Morrison-Woodbury formula around the handle's own solves.
//
//     Z = A^-1 E_R          the columns of A^-1 of the touched rows, one TILE of at most 1024 of them at a time
//     S_c = I + D_c Z[C_c, R_c],   y_c = S_c^-1 D_c x0[C_c],   x_c = x0 - Z[:, R_c] y_c
//
// apps.cpp drives it per tile: k_upd_units writes the unit right-hand sides, the handle's many-RHS solve turns them into
// the tile of Z in place, k_upd_capacitance forms and solves the small systems of the tile's cases, k_upd_apply writes
// their columns of X.  The tables the kernels read (UpdTables) are built once per plan on the host.
//
// Every sum runs in a fixed order and there are no atomics: results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cs3_device.hpp"

namespace cs3 {

namespace {

constexpr int RK = UPD_MAX_RANK;        // 16: rows and columns of one case
constexpr int SLD = RK + 1;             // leading dimension of S in LDS: column 16 is the right-hand side
constexpr int UNIT_NT = 256, UNIT_ROWS = 16;
constexpr int APPLY_STAGE = 8;          // rows of Z in LDS at a time: 8 x 1024 x 8 B = 64 KB at the full tile width
constexpr int APPLY_ROWS = 128;         // rows per workgroup: the 160 B of y / positions a lane loads are paid once per 128 rows
constexpr int APPLY_NT_MIN = 512;       // threads of the smallest workgroup (lanes beyond the tile's cases only move Z)
constexpr int APPLY_PF = 8;             // 16-byte loads per thread and stage at 512 threads and the full width
static_assert(APPLY_STAGE * UPD_MAX_TILE / 2 <= APPLY_PF * APPLY_NT_MIN, "a stage must fit the prefetch registers of the smallest block");

__device__ __forceinline__ void upd_fetch(const double *__restrict__ src, long long len, int tid, int nt, double2 (&pf)[APPLY_PF],
                                          double &pf_tail)
{
    const double2 *src2 = reinterpret_cast<const double2 *>(src);
#pragma unroll
    for (int m = 0; m < APPLY_PF; ++m) {
        const long long e = tid + (long long) m * nt;
        pf[m] = (e < len / 2) ? src2[e] : make_double2(0.0, 0.0);
    }
    if ((len & 1) && tid == 0) pf_tail = src[len - 1];
}

__device__ __forceinline__ void upd_stash(double *dst, long long len, int tid, int nt, const double2 (&pf)[APPLY_PF], double pf_tail)
{
    double2 *dst2 = reinterpret_cast<double2 *>(dst);
#pragma unroll
    for (int m = 0; m < APPLY_PF; ++m) {
        const long long e = tid + (long long) m * nt;
        if (e < len / 2) dst2[e] = pf[m];
    }
    if ((len & 1) && tid == 0) dst[len - 1] = pf_tail;
}

}  // namespace

// The tile's right-hand sides: Z [n, t] row-major, column j = e_{unit_row[j]} (a negative row: a zero column, the padding
// up to the solve width).  A thread keeps the rows of its columns and walks UNIT_ROWS rows: stores only, coalesced.
__global__ void __launch_bounds__(UNIT_NT)
k_upd_units(double *__restrict__ Z, long long n, int t, const int *__restrict__ unit_row)
{
    const long long i0 = (long long) blockIdx.x * UNIT_ROWS, i1 = std::min(n, i0 + UNIT_ROWS);
    for (int j = threadIdx.x; j < t; j += UNIT_NT) {
        const long long rj = unit_row[j];
        for (long long i = i0; i < i1; ++i) Z[i * t + j] = (rj == i) ? 1.0 : 0.0;
    }
}

// One case per wave.  (A lane per case would hold D, G and S -- 3 x 256 doubles -- in runtime-indexed registers, i.e. in
// scratch; a wave with the three blocks in 6.3 KB of LDS has 4 entries of each per lane and a handful of VGPRs.  The
// kernel moves a few hundred bytes per case and is far from any limit either way.)
//   D (r x s): the case's values, duplicates of one (i, j) added in triplet order
//   G (s x r): Z[col_a, zcol_k], gathered
//   S = I + D G and the right-hand side D x0[C], sums over ascending a
//   elimination with partial pivoting (largest |.|, ties to the lowest row), rpiv = min |pivot| / max(1, max |S|)
// y_c is written zero-padded to 16; flag = an exactly zero pivot, or rpiv <= sing_tol when sing_tol > 0, or a NaN among
// the pivot candidates (a NaN value of the case makes its whole row of S NaN, so step 0 meets it): rpiv = NaN then.
__global__ void __launch_bounds__(64)
k_upd_capacitance(const UpdCase *__restrict__ cases, const int *__restrict__ cp, const unsigned char *__restrict__ tpos,
                  const double *__restrict__ cx, const double *__restrict__ Z, int t, const double *__restrict__ x0,
                  int c0, double sing_tol, double *__restrict__ Y, double *__restrict__ rpiv, int *__restrict__ flag)
{
    __shared__ double Dm[RK * RK], Gm[RK * RK], Sm[RK * SLD], xc[RK];
    const int c = c0 + blockIdx.x, lane = threadIdx.x;
    const UpdCase *uc = cases + c;
    const int r = uc->r, s = uc->s;
    if (r == 0) {                                        // an empty case: x_c = x0
        if (lane < RK) Y[(long long) c * RK + lane] = 0.0;
        if (lane == 0) { rpiv[c] = 1.0; flag[c] = 0; }
        return;
    }
    // D: lane owns entries lane + 64 m and takes its triplets in their order
    {
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = cp[c]; p < cp[c + 1]; ++p) {
            const int e = tpos[p];
            const double v = cx[p];
#pragma unroll
            for (int m = 0; m < 4; ++m) if (e == lane + 64 * m) d[m] += v;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) Dm[lane + 64 * m] = d[m];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int e = lane + 64 * m, a = e >> 4, k = e & 15;
        Gm[e] = (a < s && k < r) ? Z[(long long) uc->col[a] * t + uc->zcol[k]] : 0.0;
    }
    if (lane < RK) xc[lane] = (lane < s) ? x0[uc->col[lane]] : 0.0;
    __syncthreads();
    // S (entry (i, k) at i * SLD + k) and the right-hand side in column 16; max |S|
    double smax = 0.0;
    for (int e = lane; e < RK * SLD; e += 64) {
        const int i = e / SLD, k = e - i * SLD;
        double acc = 0.0;
        if (i < r && k < r) {
            acc = (i == k) ? 1.0 : 0.0;
            for (int a = 0; a < s; ++a) acc += Dm[i * RK + a] * Gm[a * RK + k];
            smax = fmax(smax, fabs(acc));
        } else if (i < r && k == RK) {
            for (int a = 0; a < s; ++a) acc += Dm[i * RK + a] * xc[a];
        }
        Sm[e] = acc;
    }
    for (int off = 32; off > 0; off >>= 1) smax = fmax(smax, __shfl_xor(smax, off));
    __syncthreads();
    double pmin = HUGE_VAL;
    bool zero = false;
    for (int k = 0; k < r; ++k) {
        // pivot search over rows k .. r-1 of column k: every lane ends with the same (value, row).  A NaN counts as larger
        // than every number (plain comparisons would let a lane keep its own NaN and refuse its neighbour's, and the lanes
        // would part ways); among numbers the order is the usual one
        double pv = (lane >= k && lane < r) ? fabs(Sm[lane * SLD + k]) : -1.0;
        int pi = lane;
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(pv, off);
            const int oi = __shfl_xor(pi, off);
            const bool on = ov != ov, pn = pv != pv;
            if (on ? (!pn || oi < pi) : (!pn && (ov > pv || (ov == pv && oi < pi)))) { pv = ov; pi = oi; }
        }
        if (!(pv > 0.0)) { pmin = pv; zero = true; break; }      // an exactly zero (or NaN) column: singular; uniform
        pmin = (pv < pmin) ? pv : pmin;
        if (pi != k && lane >= k && lane <= RK) {
            const double a = Sm[k * SLD + lane], b = Sm[pi * SLD + lane];
            Sm[k * SLD + lane] = b; Sm[pi * SLD + lane] = a;
        }
        __syncthreads();
        const double piv = Sm[k * SLD + k];
        const int w = RK - k;                            // columns k+1 .. 16 of the rows below
        for (int e = lane; e < (r - k - 1) * w; e += 64) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            Sm[i * SLD + j] -= (Sm[i * SLD + k] / piv) * Sm[k * SLD + j];
        }
        __syncthreads();
    }
    double y = 0.0;
    if (!zero) {                                         // back substitution by columns, on column 16
        for (int k = r - 1; k >= 0; --k) {
            const double yk = Sm[k * SLD + RK] / Sm[k * SLD + k];
            if (lane == k) y = yk;
            __syncthreads();
            if (lane < k) Sm[lane * SLD + RK] -= Sm[lane * SLD + k] * yk;
            __syncthreads();
        }
    }
    const double rp = pmin / fmax(1.0, smax);            // (a NaN pivot travels into rpiv)
    if (lane < RK) Y[(long long) c * RK + lane] = (lane < r) ? y : 0.0;
    if (lane == 0) {
        rpiv[c] = rp;
        flag[c] = (zero || (sing_tol > 0.0 && rp <= sing_tol)) ? 1 : 0;
    }
}

// X[i, c] = x0[i] - sum_j Z[i, zcol(c, j)] y_c[j] for the cases c0 .. c0 + nc - 1 of one tile, NaN for a flagged case.
// A workgroup owns APPLY_ROWS rows; lanes are cases (consecutive lanes, consecutive addresses of X), y_c and the packed
// column positions sit in registers for the whole row block.  Z travels through LDS in stages of APPLY_STAGE rows -- one
// contiguous piece of Z, read with 16-byte loads by all threads (those without a case included) -- and the loads of the
// next stage are in flight in registers while the current one is consumed: Z is read once, X written once, both
// coalesced.  The gathered 8-byte LDS reads of a row are data dependent (a case's columns sit wherever the plan placed
// them; consecutive cases mostly read nearby columns), so no padding or swizzle removes their bank conflicts; at r reads
// per entry of X written they stay far below the LDS rate.
__global__ void __launch_bounds__(1024)
k_upd_apply(const double *__restrict__ Z, int t, const double *__restrict__ x0, long long n, const UpdCase *__restrict__ cases,
            const double *__restrict__ Y, const int *__restrict__ flag, int c0, int nc, int rmax, long long ldx,
            double *__restrict__ X)
{
    extern __shared__ double zl[];                       // [APPLY_STAGE][t]
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long i0 = (long long) blockIdx.x * APPLY_ROWS, i1 = std::min(n, i0 + APPLY_ROWS);
    const bool mine = tid < nc;
    double y[RK];
    unsigned zc[RK / 2];                                 // two 16-bit column positions per word
    int r = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < RK; ++j) y[j] = 0.0;
#pragma unroll
    for (int j = 0; j < RK / 2; ++j) zc[j] = 0u;
    if (mine) {
        const UpdCase *uc = cases + c0 + tid;
        r = uc->r;
        bad = flag[c0 + tid] != 0;
#pragma unroll
        for (int j = 0; j < RK; ++j) y[j] = Y[(long long) (c0 + tid) * RK + j];
#pragma unroll
        for (int j = 0; j < RK / 2; ++j) zc[j] = (unsigned) uc->zcol[2 * j] | ((unsigned) uc->zcol[2 * j + 1] << 16);
    }
    // the loads of a stage: len doubles from an address that is 16-byte aligned (every stage starts a multiple of the even
    // APPLY_STAGE rows into Z); an odd tail entry travels through thread 0
    double2 pf[APPLY_PF];
    double pf_tail = 0.0;
    if (i0 < i1) upd_fetch(Z + i0 * t, (std::min(i1, i0 + APPLY_STAGE) - i0) * t, tid, nt, pf, pf_tail);
    for (long long ia = i0; ia < i1; ia += APPLY_STAGE) {
        __syncthreads();                                 // the previous stage has been consumed
        upd_stash(zl, (std::min(i1, ia + APPLY_STAGE) - ia) * t, tid, nt, pf, pf_tail);
        __syncthreads();
        if (ia + APPLY_STAGE < i1)
            upd_fetch(Z + (ia + APPLY_STAGE) * t, (std::min(i1, ia + 2 * APPLY_STAGE) - ia - APPLY_STAGE) * t, tid, nt, pf, pf_tail);
        const int rows = (int) (std::min(i1, ia + APPLY_STAGE) - ia);
        if (mine) {
            for (int q = 0; q < rows; ++q) {
                const double *zr = zl + q * t;
                double acc = x0[ia + q];
#pragma unroll
                for (int j = 0; j < RK; ++j) {
                    if (j >= rmax) break;                // (uniform: the largest rank of the tile)
                    const unsigned pos = (j & 1) ? (zc[j >> 1] >> 16) : (zc[j >> 1] & 0xffffu);
                    if (j < r) acc -= zr[pos] * y[j];
                }
                X[(ia + q) * ldx + c0 + tid] = bad ? __builtin_nan("") : acc;
            }
        }
    }
}

#define CS3_UPD_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t prepare_updates_kernels()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_upd_apply), hipFuncAttributeMaxDynamicSharedMemorySize,
                               APPLY_STAGE * UPD_MAX_TILE * (int) sizeof(double));
}

hipError_t launch_upd_units(double *Z, long long n, int t, const int *unit_row, hipStream_t st)
{
    if (n == 0 || t == 0) return hipSuccess;
    hipLaunchKernelGGL(k_upd_units, dim3((unsigned) ((n + UNIT_ROWS - 1) / UNIT_ROWS)), dim3(UNIT_NT), 0, st, Z, n, t, unit_row);
    CS3_UPD_CHECK();
    return hipSuccess;
}

hipError_t launch_upd_capacitance(const UpdTables &T, const double *cx, const double *Z, int t, const double *x0, int c0, int nc,
                                  double sing_tol, double *rpiv, hipStream_t st)
{
    if (nc == 0) return hipSuccess;
    hipLaunchKernelGGL(k_upd_capacitance, dim3((unsigned) nc), dim3(64), 0, st, T.cases, T.cp, T.tpos, cx, Z, t, x0, c0, sing_tol,
                       T.y, rpiv, T.flag);
    CS3_UPD_CHECK();
    return hipSuccess;
}

hipError_t launch_upd_apply(const UpdTables &T, const double *Z, int t, const double *x0, long long n, int c0, int nc, int rmax,
                            long long ldx, double *X, hipStream_t st)
{
    if (n == 0 || nc == 0) return hipSuccess;
    if (t > UPD_MAX_TILE || nc > UPD_MAX_TILE_CASES) return hipErrorInvalidValue;
    const int nt = std::max(APPLY_NT_MIN, (nc + 63) / 64 * 64);
    const size_t lds = (size_t) APPLY_STAGE * t * sizeof(double);
    hipLaunchKernelGGL(k_upd_apply, dim3((unsigned) ((n + APPLY_ROWS - 1) / APPLY_ROWS)), dim3(nt), lds, st, Z, t, x0, n, T.cases,
                       T.y, T.flag, c0, nc, rmax, ldx, X);
    CS3_UPD_CHECK();
    return hipSuccess;
}

}  // namespace cs3
