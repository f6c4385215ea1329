// Many low-rank-modified COMPLEX systems (A + dA_c) v = i on a handle that holds the real-equivalent form of a complex
// matrix (cs3_cplx_updates_*): the vector steps of the Sherman-Morrison-Woodbury formula in complex arithmetic, around the
// handle's unchanged solves.
//
//     Z [2n, t] = M^-1 pack_N(E_R)      ONE real column per touched complex row: (Re, Im) of A^-1 e_row in rows 2i, 2i + 1
//     S_c = I + D_c Z[C_c, R_c],   y_c = S_c^-1 D_c x0[C_c],   x_c = x0 - Z[:, R_c] y_c          (complex)
//
// M is the real form of diag(s) A, and pack_N(e_row) = (Re s_row, Im s_row) in the pair of that row: M^-1 of it is
// A^-1 e_row with no rotation of dA_c anywhere.  apps.cpp drives it per tile as it drives updates.hip: k_cupd_units writes
// the right-hand sides, the handle's many-RHS solve turns them into the tile of Z in place, k_cupd_capacitance forms and
// solves the small systems, k_cupd_apply writes their columns of X.  Plan, cases and tiles are those of updates.hip.
//
// Arithmetic is that of cplxplan.hip on separate real and imaginary parts: a product is four rounded products, then the
// two sums; a quotient is cdiv below; every sum runs in a fixed order, component by component; no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // a * b - c * d stays three roundings: what a host restates

namespace cs3 {

namespace {

constexpr int RK = UPD_MAX_RANK;        // 16: rows and columns of one case
constexpr int SLD = RK + 1;             // leading dimension of S in LDS: column 16 is the right-hand side
constexpr int UNIT_NT = CUPD_UNIT_THREADS, UNIT_ROWS = CUPD_UNIT_ROWS;
constexpr int APPLY_STAGE = CUPD_APPLY_STAGE, APPLY_ROWS = CUPD_APPLY_ROWS, APPLY_NT_MIN = CUPD_APPLY_NT_MIN;
constexpr int APPLY_PF = 4;             // 16-byte loads per thread and stage at 1024 threads and the full width
static_assert(APPLY_STAGE * UPD_MAX_TILE <= APPLY_PF * APPLY_NT_MIN, "a stage must fit the prefetch registers of the smallest block");
static_assert(APPLY_ROWS % APPLY_STAGE == 0, "a row block is whole stages");

__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    double2 w;
    w.x = (a.x * b.x) - (a.y * b.y);
    w.y = (a.x * b.y) + (a.y * b.x);
    return w;
}

// a / b = a conj(b) / |b|^2, the textbook formula: one sum of two squares, two sums of two products, two quotients
__device__ __forceinline__ double2 cdiv(double2 a, double2 b)
{
    const double den = (b.x * b.x) + (b.y * b.y);
    double2 w;
    w.x = ((a.x * b.x) + (a.y * b.y)) / den;
    w.y = ((a.y * b.x) - (a.x * b.y)) / den;
    return w;
}

__device__ __forceinline__ double cabs1(double2 a) { return fabs(a.x) + fabs(a.y); }

// a stage is an even number of doubles (whole pairs of rows) at a 16-byte aligned address: no tail
__device__ __forceinline__ void cupd_fetch(const double *__restrict__ src, long long len, int tid, int nt, double2 (&pf)[APPLY_PF])
{
    const double2 *src2 = reinterpret_cast<const double2 *>(src);
#pragma unroll
    for (int m = 0; m < APPLY_PF; ++m) {
        const unsigned e = (unsigned) tid + (unsigned) m * (unsigned) nt;      // (a stage has at most 4096 such loads)
        pf[m] = (e < (unsigned) (len / 2)) ? src2[e] : make_double2(0.0, 0.0);
    }
}

// The stage leaves the registers INTERLEAVED: zl[q][c] = (Z[2q, c], Z[2q + 1, c]) as one 16-byte entry, so that a lane
// gathers a complex number with one LDS read.  Double d of the piece is row d / t (real rows of the stage), column d % t.
__device__ __forceinline__ void cupd_stash(double *dst, long long len, int t, int tid, int nt, const double2 (&pf)[APPLY_PF])
{
#pragma unroll
    for (int m = 0; m < APPLY_PF; ++m) {
        const unsigned e = (unsigned) tid + (unsigned) m * (unsigned) nt;
        if (e < (unsigned) (len / 2)) {
            const unsigned d = 2u * e, ut = (unsigned) t;
            unsigned rr = d / ut, c = d - rr * ut;
            dst[2u * ((rr >> 1) * ut + c) + (rr & 1u)] = pf[m].x;
            if (++c == ut) { c = 0; ++rr; }
            dst[2u * ((rr >> 1) * ut + c) + (rr & 1u)] = pf[m].y;
        }
    }
}

}  // namespace

// The tile's right-hand sides: Z [2n, t] real, row-major.  Column j is zero but for the pair of complex row unit_row[j],
// which holds pack_N((1, +0)) = s_row * (1, +0), the product cs3_cplx_pack_dev would form for e_row (a negative row: a zero
// column, the padding up to the solve width).  A workgroup owns UNIT_ROWS complex rows -- never half a pair --, a thread
// keeps the rows of its columns: stores only, coalesced.
__global__ void __launch_bounds__(UNIT_NT)
k_cupd_units(double *__restrict__ Z, long long n, int t, const int *__restrict__ unit_row, const double2 *__restrict__ s)
{
    const long long i0 = (long long) blockIdx.x * UNIT_ROWS, i1 = std::min(n, i0 + UNIT_ROWS);
    for (int j = threadIdx.x; j < t; j += UNIT_NT) {
        const long long rj = unit_row[j];
        for (long long i = i0; i < i1; ++i) {
            double2 u = make_double2(0.0, 0.0);
            if (rj == i) u = cmul(s[i], make_double2(1.0, 0.0));
            Z[2 * i * t + j] = u.x;
            Z[(2 * i + 1) * t + j] = u.y;
        }
    }
}

// One case per wave, as k_upd_capacitance, with D, G, S and the right-hand side column as split real / imaginary planes
// in LDS.
//   D (r x s): the case's values, duplicates of one (i, j) added in triplet order, component by component
//   G (s x r): (Z[2 col_a, zcol_k], Z[2 col_a + 1, zcol_k]), gathered; x0[C] likewise
//   S = I + D G and the right-hand side D x0[C], sums over ascending a, every product a cmul
//   elimination with partial pivoting by cabs1 = |Re| + |Im| (ties to the lowest row, a NaN above every number),
//   multipliers and the back substitution through cdiv;  rpiv = min cabs1(pivot) / max(1, max cabs1(S))
// y_c is written zero-padded to 16 complex; flag = an exactly zero pivot column, or rpiv <= sing_tol when sing_tol > 0, or
// a NaN among the pivot candidates (a NaN value of the case makes its whole row of S NaN, so step 0 meets it): rpiv = NaN.
__global__ void __launch_bounds__(64)
k_cupd_capacitance(const UpdCase *__restrict__ cases, const int *__restrict__ cp, const unsigned char *__restrict__ tpos,
                   const double2 *__restrict__ cz, const double *__restrict__ Z, int t, const double2 *__restrict__ x0,
                   int c0, double sing_tol, double2 *__restrict__ Y, double *__restrict__ rpiv, int *__restrict__ flag)
{
    __shared__ double Dr[RK * RK], Di[RK * RK], Gr[RK * RK], Gi[RK * RK], Sr[RK * SLD], Si[RK * SLD], xr[RK], xi[RK];
    const int c = c0 + blockIdx.x, lane = threadIdx.x;
    const UpdCase *uc = cases + c;
    const int r = uc->r, s = uc->s;
    if (r == 0) {                                        // an empty case: x_c = x0
        if (lane < RK) Y[(long long) c * RK + lane] = make_double2(0.0, 0.0);
        if (lane == 0) { rpiv[c] = 1.0; flag[c] = 0; }
        return;
    }
    // D: lane owns entries lane + 64 m and takes its triplets in their order
    {
        double dr[4] = {0.0, 0.0, 0.0, 0.0}, di[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = cp[c]; p < cp[c + 1]; ++p) {
            const int e = tpos[p];
            const double2 v = cz[p];
#pragma unroll
            for (int m = 0; m < 4; ++m) if (e == lane + 64 * m) { dr[m] += v.x; di[m] += v.y; }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) { Dr[lane + 64 * m] = dr[m]; Di[lane + 64 * m] = di[m]; }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int e = lane + 64 * m, a = e >> 4, k = e & 15;
        const bool in = a < s && k < r;
        const long long at = in ? 2LL * uc->col[a] * t + uc->zcol[k] : 0;
        Gr[e] = in ? Z[at] : 0.0;
        Gi[e] = in ? Z[at + t] : 0.0;
    }
    if (lane < RK) {
        const double2 v = (lane < s) ? x0[uc->col[lane]] : make_double2(0.0, 0.0);
        xr[lane] = v.x; xi[lane] = v.y;
    }
    __syncthreads();
    // S (entry (i, k) at i * SLD + k) and the right-hand side in column 16; max cabs1(S)
    double smax = 0.0;
    for (int e = lane; e < RK * SLD; e += 64) {
        const int i = e / SLD, k = e - i * SLD;
        double2 acc = make_double2(0.0, 0.0);
        if (i < r && k < r) {
            acc.x = (i == k) ? 1.0 : 0.0;
            for (int a = 0; a < s; ++a) {
                const double2 pr = cmul(make_double2(Dr[i * RK + a], Di[i * RK + a]), make_double2(Gr[a * RK + k], Gi[a * RK + k]));
                acc.x += pr.x; acc.y += pr.y;
            }
            smax = fmax(smax, cabs1(acc));
        } else if (i < r && k == RK) {
            for (int a = 0; a < s; ++a) {
                const double2 pr = cmul(make_double2(Dr[i * RK + a], Di[i * RK + a]), make_double2(xr[a], xi[a]));
                acc.x += pr.x; acc.y += pr.y;
            }
        }
        Sr[e] = acc.x; Si[e] = acc.y;
    }
    for (int off = 32; off > 0; off >>= 1) smax = fmax(smax, __shfl_xor(smax, off));
    __syncthreads();
    double pmin = HUGE_VAL;
    bool zero = false;
    for (int k = 0; k < r; ++k) {
        // pivot search over rows k .. r-1 of column k: the butterfly carries (cabs1, row) and every lane ends with the same
        // pair.  A NaN counts as larger than every number, ties go to the lowest row, so the exit below is wave-uniform
        double pv = (lane >= k && lane < r) ? cabs1(make_double2(Sr[lane * SLD + k], Si[lane * SLD + k])) : -1.0;
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
            const double ar = Sr[k * SLD + lane], ai = Si[k * SLD + lane], br = Sr[pi * SLD + lane], bi = Si[pi * SLD + lane];
            Sr[k * SLD + lane] = br; Si[k * SLD + lane] = bi;
            Sr[pi * SLD + lane] = ar; Si[pi * SLD + lane] = ai;
        }
        __syncthreads();
        const double2 piv = make_double2(Sr[k * SLD + k], Si[k * SLD + k]);
        const int w = RK - k;                            // columns k+1 .. 16 of the rows below
        for (int e = lane; e < (r - k - 1) * w; e += 64) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            const double2 l = cdiv(make_double2(Sr[i * SLD + k], Si[i * SLD + k]), piv);
            const double2 pr = cmul(l, make_double2(Sr[k * SLD + j], Si[k * SLD + j]));
            Sr[i * SLD + j] -= pr.x; Si[i * SLD + j] -= pr.y;
        }
        __syncthreads();
    }
    double2 y = make_double2(0.0, 0.0);
    if (!zero) {                                         // back substitution by columns, on column 16
        for (int k = r - 1; k >= 0; --k) {
            const double2 yk = cdiv(make_double2(Sr[k * SLD + RK], Si[k * SLD + RK]), make_double2(Sr[k * SLD + k], Si[k * SLD + k]));
            if (lane == k) y = yk;
            __syncthreads();
            if (lane < k) {
                const double2 pr = cmul(make_double2(Sr[lane * SLD + k], Si[lane * SLD + k]), yk);
                Sr[lane * SLD + RK] -= pr.x; Si[lane * SLD + RK] -= pr.y;
            }
            __syncthreads();
        }
    }
    const double rp = pmin / fmax(1.0, smax);            // (a NaN pivot travels into rpiv)
    if (lane < RK) Y[(long long) c * RK + lane] = (lane < r) ? y : make_double2(0.0, 0.0);
    if (lane == 0) {
        rpiv[c] = rp;
        flag[c] = (zero || (sing_tol > 0.0 && rp <= sing_tol)) ? 1 : 0;
    }
}

// X[i, c] = x0[i] - sum_j Z[i, zcol(c, j)] y_c[j] (complex) for the cases c0 .. c0 + nc - 1 of one tile, (NaN, NaN) for a
// flagged case.  A workgroup owns APPLY_ROWS complex rows; lanes are cases (consecutive lanes, consecutive 16-byte entries
// of X), y_c -- 16 complex, 64 VGPRs, held whole -- and the packed column positions sit in registers for the whole row
// block.  Z travels through LDS in stages of APPLY_STAGE row PAIRS -- one contiguous piece of Z, read with 16-byte loads by
// all threads, those without a case included -- and the loads of the next stage are in flight in registers while the
// current one is consumed: Z is read once, X written once, both coalesced.  A lane gathers (zr[pos], zi[pos]) from the two
// rows of a pair and accumulates in ascending j.  The workgroup is 1024 threads whatever the tile, so a stage is 4 loads
// per thread and y fits beside them below the 128 VGPRs such a workgroup may use.
__global__ void __launch_bounds__(1024)
k_cupd_apply(const double *__restrict__ Z, int t, const double2 *__restrict__ x0, long long n, const UpdCase *__restrict__ cases,
             const double2 *__restrict__ Y, const int *__restrict__ flag, int c0, int nc, int rmax, long long ldx,
             double2 *__restrict__ X)
{
    extern __shared__ double zl[];                       // [APPLY_STAGE][t] pairs (Re, Im)
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long i0 = (long long) blockIdx.x * APPLY_ROWS, i1 = std::min(n, i0 + APPLY_ROWS);
    const bool mine = tid < nc;
    double2 y[RK];
    unsigned zc[RK / 2];                                 // two 16-bit column positions per word
    int r = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < RK; ++j) y[j] = make_double2(0.0, 0.0);
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
    double2 pf[APPLY_PF];
    if (i0 < i1) cupd_fetch(Z + 2 * i0 * t, 2 * (std::min(i1, i0 + APPLY_STAGE) - i0) * t, tid, nt, pf);
    for (long long ia = i0; ia < i1; ia += APPLY_STAGE) {
        __syncthreads();                                 // the previous stage has been consumed
        cupd_stash(zl, 2 * (std::min(i1, ia + APPLY_STAGE) - ia) * t, t, tid, nt, pf);
        __syncthreads();
        if (ia + APPLY_STAGE < i1)
            cupd_fetch(Z + 2 * (ia + APPLY_STAGE) * t, 2 * (std::min(i1, ia + 2 * APPLY_STAGE) - ia - APPLY_STAGE) * t, tid, nt, pf);
        const int rows = (int) (std::min(i1, ia + APPLY_STAGE) - ia);
        if (mine) {
#pragma unroll 1
            for (int q = 0; q < rows; ++q) {
                const double2 *zq = reinterpret_cast<const double2 *>(zl) + q * t;
                double2 acc = x0[ia + q];
#pragma unroll
                for (int j = 0; j < RK; ++j) {
                    const unsigned pos = (j & 1) ? (zc[j >> 1] >> 16) : (zc[j >> 1] & 0xffffu);
                    if (j < rmax && j < r) {             // (j < rmax is uniform: the largest rank of the tile)
                        const double2 pr = cmul(zq[pos], y[j]);
                        acc.x -= pr.x; acc.y -= pr.y;
                    }
                }
                X[(ia + q) * ldx + c0 + tid] = bad ? make_double2(__builtin_nan(""), __builtin_nan("")) : acc;
            }
        }
    }
}

#define CS3_CUPD_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t prepare_cupd_kernels()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_cupd_apply), hipFuncAttributeMaxDynamicSharedMemorySize,
                               2 * APPLY_STAGE * UPD_MAX_TILE * (int) sizeof(double));
}

hipError_t launch_cupd_units(double *Z, long long n, int t, const int *unit_row, const double *s, hipStream_t st)
{
    if (n == 0 || t == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cupd_units, dim3((unsigned) ((n + UNIT_ROWS - 1) / UNIT_ROWS)), dim3(UNIT_NT), 0, st, Z, n, t, unit_row,
                       reinterpret_cast<const double2 *>(s));
    CS3_CUPD_CHECK();
    return hipSuccess;
}

hipError_t launch_cupd_capacitance(const UpdTables &T, const double *cz, const double *Z, int t, const double *x0, int c0, int nc,
                                   double sing_tol, double *rpiv, hipStream_t st)
{
    if (nc == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cupd_capacitance, dim3((unsigned) nc), dim3(64), 0, st, T.cases, T.cp, T.tpos,
                       reinterpret_cast<const double2 *>(cz), Z, t, reinterpret_cast<const double2 *>(x0), c0, sing_tol,
                       reinterpret_cast<double2 *>(T.y), rpiv, T.flag);
    CS3_CUPD_CHECK();
    return hipSuccess;
}

hipError_t launch_cupd_apply(const UpdTables &T, const double *Z, int t, const double *x0, long long n, int c0, int nc, int rmax,
                             long long ldx, double *X, hipStream_t st)
{
    if (n == 0 || nc == 0) return hipSuccess;
    if (t > UPD_MAX_TILE || nc > UPD_MAX_TILE_CASES) return hipErrorInvalidValue;
    const int nt = std::max(APPLY_NT_MIN, (nc + 63) / 64 * 64);
    const size_t lds = (size_t) 2 * APPLY_STAGE * t * sizeof(double);
    hipLaunchKernelGGL(k_cupd_apply, dim3((unsigned) ((n + APPLY_ROWS - 1) / APPLY_ROWS)), dim3(nt), lds, st, Z, t,
                       reinterpret_cast<const double2 *>(x0), n, T.cases, reinterpret_cast<const double2 *>(T.y), T.flag, c0, nc, rmax,
                       ldx, reinterpret_cast<double2 *>(X));
    CS3_CUPD_CHECK();
    return hipSuccess;
}

}  // namespace cs3
