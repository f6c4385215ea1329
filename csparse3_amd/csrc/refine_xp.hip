// Extra-precise refinement on the factors a handle holds (cs3_refine_xp*, cs3_residual_xp*): the kernels around the
// handle's own solves.
//
//     r  = b - op(A) (x + xt)   accumulated in doubled precision, rounded once      k_residual_xp
//     dx = op(A)^-1 r                                                                the handle's solve, in place
//     nd = max |dx_i|, nx = max |x_i| per system                                     k_xp_maxima
//     stop / apply per system                                                        k_xp_control
//     (x, xt) += dx in doubled precision, for the systems that apply                 k_xp_update
//
// api.cpp drives the passes and reads one word per pass.  The closing pass runs k_residual_xp on x alone with the ratio
// switch (|r_i| / s_i instead of r_i) and k_xp_maxima over it: berr and max |x_i|.
//
// The sums run in a fixed order per thread, the only atomics are maxima on the bit patterns of non-negative doubles (exact,
// whatever the order): results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs3_device.hpp"

#pragma clang fp contract(off)          // every product and sum below is rounded on its own; the FMAs are written out

namespace cs3 {

namespace {

// Knuth's TwoSum: s = fl(a + b), e = the exact error of that sum (six operations, no branch)
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// larger of two non-negative doubles, a NaN wins (its bit pattern, sign clear, is above +inf's for atomicMax too)
__device__ __forceinline__ double max_nan(double m, double a) { return (a > m || a != a) ? a : m; }

}  // namespace

// One thread per (row, right-hand side) of one matrix (blockIdx.y), a grid-stride loop over the n * nrhs outputs.  The
// view is the handle's row view (trans: its column view), so the entries of a row come in cs3_residual_dev's order.
template <bool TAIL, bool RATIO>
__global__ void __launch_bounds__(XP_BLOCK)
k_residual_xp(const int *__restrict__ Rp, const int *__restrict__ Rj, const int *__restrict__ Rmap,
              const double *__restrict__ Ax_all, const double *__restrict__ B_all, const double *__restrict__ X_all,
              const double *__restrict__ XT_all, double *__restrict__ R_all, double *__restrict__ S_all,
              long long n, int nrhs, long long nnz_a)
{
    const long long total = n * nrhs, base = (long long) blockIdx.y * total;
    const double *Ax = Ax_all + (long long) blockIdx.y * nnz_a;
    const double *B = B_all + base, *X = X_all + base;
    const double *XT = TAIL ? XT_all + base : nullptr;
    double *R = R_all + base;
    double *S = S_all ? S_all + base : nullptr;
    for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x) {
        const long long i = e / nrhs;
        const int t = (int) (e - i * nrhs);
        const double b = B[e];
        double sh = b, sl = 0.0, den = fabs(b);
        for (int p = Rp[i]; p < Rp[i + 1]; ++p) {
            const double a = Ax[Rmap[p]];
            const long long xj = (long long) Rj[p] * nrhs + t;
            const double x = X[xj];
            const double ph = a * x;
            const double pl = __builtin_fma(a, x, -ph);
            double err;
            two_sum(sh, -ph, sh, err);
            double c = err - pl;
            if (TAIL) c = c - a * XT[xj];
            sl = sl + c;
            den = den + fabs(a) * fabs(x);
        }
        const double r = sh + sl;
        if (RATIO) R[e] = (r == 0.0 && den == 0.0) ? 0.0 : fabs(r) / den;
        else R[e] = r;
        if (S) S[e] = den;
    }
}

// Per system the maxima of |D| and |X| over its column.  A workgroup covers a tile of w = min(nrhs, XP_BLOCK) columns
// (blockIdx.z) and XP_BLOCK / w rows per pass: lanes run along the columns, so the loads are contiguous.  A thread keeps
// its column throughout; the workgroup's threads of one column meet in LDS, and one atomicMax per column and workgroup
// reaches memory.
__global__ void __launch_bounds__(XP_BLOCK)
k_xp_maxima(const double *__restrict__ D_all, const double *__restrict__ X_all, XpSys *__restrict__ sys, long long n, int nrhs)
{
    __shared__ double sd[XP_BLOCK], sx[XP_BLOCK];
    const int w = std::min(nrhs, XP_BLOCK), rows = XP_BLOCK / w;
    const int tid = threadIdx.x, lane_t = tid % w, lane_r = tid / w;
    const int t = (int) blockIdx.z * w + lane_t;
    const bool live = lane_r < rows && t < nrhs;
    const long long base = (long long) blockIdx.y * n * nrhs;
    double md = 0.0, mx = 0.0;
    if (live) {
        for (long long i = (long long) blockIdx.x * rows + lane_r; i < n; i += (long long) gridDim.x * rows) {
            const long long e = base + i * nrhs + t;
            md = max_nan(md, fabs(D_all[e]));
            mx = max_nan(mx, fabs(X_all[e]));
        }
    }
    sd[tid] = md; sx[tid] = mx;
    __syncthreads();
    if (tid < w && t < nrhs) {
        for (int r = 1; r < rows; ++r) { md = max_nan(md, sd[r * w + tid]); mx = max_nan(mx, sx[r * w + tid]); }
        XpSys &s = sys[(long long) blockIdx.y * nrhs + t];
        atomicMax(&s.nd_bits, (unsigned long long) __double_as_longlong(md));
        atomicMax(&s.nx_bits, (unsigned long long) __double_as_longlong(mx));
    }
}

// One thread per system: what this pass's correction is worth.
__global__ void __launch_bounds__(XP_BLOCK)
k_xp_control(XpSys *__restrict__ sys, long long nsys, unsigned *__restrict__ active)
{
    const long long g = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nsys) return;
    XpSys s = sys[g];
    const double nd = __longlong_as_double((long long) s.nd_bits), nx = __longlong_as_double((long long) s.nx_bits);
    s.nd_bits = 0; s.nx_bits = 0;
    s.apply = 0;
    if (!s.stopped) {
        if (!isfinite(nd) || !isfinite(nx)) {
            s.flag = XP_NONFINITE; s.stopped = 1;
        } else {
            bool stall = false;
            if (s.iters > 0) {                       // nd_prev > 0: a zero correction has converged
                const double q = nd / s.nd_prev;
                s.rate = q > s.rate ? q : s.rate;
                stall = nd > XP_STALL_RATIO * s.nd_prev;
            }
            if (stall) {
                s.flag = XP_STALLED; s.stopped = 1;
            } else {
                s.apply = 1; s.iters += 1; s.nd_prev = nd;
                if (nd <= XP_EPS * nx) { s.flag = XP_CONVERGED; s.stopped = 1; }
            }
        }
        if (!s.stopped) atomicAdd(active, 1u);
    }
    sys[g] = s;
}

// One thread per entry; the entries of a system that does not apply are neither read nor written.
__global__ void __launch_bounds__(XP_BLOCK)
k_xp_update(double *__restrict__ X_all, double *__restrict__ XT_all, const double *__restrict__ D_all,
            const XpSys *__restrict__ sys, long long n, int nrhs)
{
    const long long total = n * nrhs, base = (long long) blockIdx.y * total;
    const XpSys *msys = sys + (long long) blockIdx.y * nrhs;
    for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x) {
        const int t = (int) (e % nrhs);
        if (!msys[t].apply) continue;
        double s, err, x, xt;
        two_sum(X_all[base + e], D_all[base + e], s, err);
        const double tl = XT_all[base + e] + err;
        two_sum(s, tl, x, xt);
        X_all[base + e] = x;
        XT_all[base + e] = xt;
    }
}

hipError_t launch_residual_xp(const int *Rp, const int *Rj, const int *Rmap, const double *Ax, const double *B, const double *X,
                              const double *XT, double *R, double *S, long long n, int nrhs, long long nnz_a, long long batch,
                              bool ratio, hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    dim3 grid((unsigned) std::min<long long>((n * nrhs + XP_BLOCK - 1) / XP_BLOCK, XP_GRID_CAP), (unsigned) batch);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(XP_BLOCK), 0, st, Rp, Rj, Rmap, Ax, B, X, XT, R, S, n, nrhs, nnz_a); };
    if (ratio) { if (XT) go(k_residual_xp<true, true>); else go(k_residual_xp<false, true>); }
    else { if (XT) go(k_residual_xp<true, false>); else go(k_residual_xp<false, false>); }
    return hipGetLastError();
}

hipError_t launch_xp_maxima(const double *D, const double *X, XpSys *sys, long long n, int nrhs, long long batch, hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    const int w = std::min(nrhs, XP_BLOCK), rows = XP_BLOCK / w;
    dim3 grid((unsigned) std::min<long long>((n + rows - 1) / rows, XP_MAXIMA_GRID_CAP), (unsigned) batch, (unsigned) ((nrhs + w - 1) / w));
    hipLaunchKernelGGL(k_xp_maxima, grid, dim3(XP_BLOCK), 0, st, D, X, sys, n, nrhs);
    return hipGetLastError();
}

hipError_t launch_xp_control(XpSys *sys, long long nsys, unsigned *active, hipStream_t st)
{
    if (nsys == 0) return hipSuccess;
    hipLaunchKernelGGL(k_xp_control, dim3((unsigned) ((nsys + XP_BLOCK - 1) / XP_BLOCK)), dim3(XP_BLOCK), 0, st, sys, nsys, active);
    return hipGetLastError();
}

hipError_t launch_xp_update(double *X, double *XT, const double *D, const XpSys *sys, long long n, int nrhs, long long batch,
                            hipStream_t st)
{
    if (n == 0 || batch == 0) return hipSuccess;
    dim3 grid((unsigned) std::min<long long>((n * nrhs + XP_BLOCK - 1) / XP_BLOCK, XP_GRID_CAP), (unsigned) batch);
    hipLaunchKernelGGL(k_xp_update, grid, dim3(XP_BLOCK), 0, st, X, XT, D, sys, n, nrhs);
    return hipGetLastError();
}

}  // namespace cs3
