// Complex plans, numeric phase (include/csparse3_amd.h, "complex matrices"): the device glue between a complex CSC matrix
// and a handle that factorises its real-equivalent form.  Five kernels, all in gather form: every output is written
// exactly once by the lane that owns it -- no memset, no atomics, nothing allocated, nothing waited for.
//
//   k_cplx_rotation   s_i = conj(d_i) / max(|Re d_i|, |Im d_i|) per matrix and row, d_i the stored diagonal
//   k_cplx_values     w = s_i z for every entry, written as the 2 x 2 block [[Re w, -Im w], [Im w, Re w]]
//   k_cplx_pack       Z [batch][n, k] complex -> Y [batch][2n, k] real
//   k_cplx_unpack     the inverse, stored or added to Z
//   k_cplx_residual   R = B - op(A) X on the complex CSC, the caller's values
//
// Arithmetic: a complex product is (ar*br - ai*bi, ar*bi + ai*br), every product rounded before the sum (fp contraction
// is off), a conjugate is a sign flip.  A host restates every result bit for bit with the same expressions.
//
// Shape: 256 threads, grid-stride over a flat 64-bit index under CPLX_GRID_CAP workgroups, one complex number per lane,
// moved as one 16-byte load or store.  The flat index is split by division in every pass: a second pass only happens beyond
// CPLX_GRID_CAP * CPLX_BLOCK numbers, where the divisions are a small part of the traffic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_cplx.hpp"

#pragma clang fp contract(off)          // a * b - c * d stays three roundings: what a host restates

namespace cs3 {

constexpr int CPLX_BLOCK = 256;
constexpr int CPLX_GRID_CAP = 2048;

struct CplxTables {
    const int *Ap, *Ai, *ecol, *dptr, *dpos, *rptr, *rpos;
};

__device__ inline double2 cplx_mul(double2 a, double2 b)
{
    double2 w;
    w.x = (a.x * b.x) - (a.y * b.y);
    w.y = (a.x * b.y) + (a.y * b.x);
    return w;
}

__device__ inline double2 cplx_conj(double2 a) { a.y = -a.y; return a; }

#define CPLX_GRID_STRIDE(idx, total)                                                                     \
    for (long long idx = (long long) blockIdx.x * CPLX_BLOCK + threadIdx.x; idx < (total);               \
         idx += (long long) gridDim.x * CPLX_BLOCK)

// one lane per (matrix, row)
__global__ void __launch_bounds__(CPLX_BLOCK)
k_cplx_rotation(CplxTables T, long long n, long long nnz, long long total, const double2 *__restrict__ Az, double2 *__restrict__ S)
{
    CPLX_GRID_STRIDE(r, total) {
        const long long b = r / n, i = r - b * n;
        const int p0 = T.dptr[i], p1 = T.dptr[i + 1];
        double2 s = make_double2(1.0, 0.0);
        if (p0 < p1) {
            const double2 *az = Az + b * nnz;
            double2 d = az[T.dpos[p0]];
            for (int p = p0 + 1; p < p1; ++p) { const double2 v = az[T.dpos[p]]; d.x += v.x; d.y += v.y; }
            const double ar = fabs(d.x), ai = fabs(d.y);
            const double m = ar > ai ? ar : ai;
            if (ar < __builtin_inf() && ai < __builtin_inf() && m > 0.0) s = make_double2(d.x / m, -d.y / m);   // (a NaN fails a comparison)
        }
        S[r] = s;
    }
}

// one lane per (matrix, entry)
__global__ void __launch_bounds__(CPLX_BLOCK)
k_cplx_values(CplxTables T, long long n, long long nnz, long long total, const double2 *__restrict__ Az,
              const double2 *__restrict__ S, double2 *__restrict__ Rx)
{
    CPLX_GRID_STRIDE(idx, total) {
        const long long b = idx / nnz, e = idx - b * nnz;
        const int j = T.ecol[e];
        const double2 w = cplx_mul(S[b * n + T.Ai[e]], Az[idx]);
        double2 *out = Rx + b * 2 * nnz + e;                        // (in units of two doubles: Rp[2j] + 2t = 2 Ap[j] + 2e)
        out[T.Ap[j]] = w;                                           // column 2j:     rows 2i, 2i + 1
        out[T.Ap[j + 1]] = make_double2(-w.y, w.x);                 // column 2j + 1: rows 2i, 2i + 1
    }
}

// one lane per (matrix, row, right-hand side), the right-hand side fastest
__global__ void __launch_bounds__(CPLX_BLOCK)
k_cplx_pack(int op, long long k, long long total, const double2 *__restrict__ Z, const double2 *__restrict__ S, double *__restrict__ Y)
{
    CPLX_GRID_STRIDE(idx, total) {
        const long long r = idx / k, c = idx - r * k;
        double2 u = Z[idx];
        if (op == CS3_CPLX_N) u = cplx_mul(S[r], u);
        else if (op == CS3_CPLX_T) u = cplx_conj(u);
        Y[2 * r * k + c] = u.x;
        Y[(2 * r + 1) * k + c] = u.y;
    }
}

__global__ void __launch_bounds__(CPLX_BLOCK)
k_cplx_unpack(int op, int accumulate, long long k, long long total, const double *__restrict__ Y, const double2 *__restrict__ S,
              double2 *__restrict__ Z)
{
    CPLX_GRID_STRIDE(idx, total) {
        const long long r = idx / k, c = idx - r * k;
        double2 y = make_double2(Y[2 * r * k + c], Y[(2 * r + 1) * k + c]);
        if (op == CS3_CPLX_H) y = cplx_mul(cplx_conj(S[r]), y);
        else if (op == CS3_CPLX_T) y = cplx_mul(S[r], cplx_conj(y));
        if (accumulate) { const double2 z = Z[idx]; y.x = z.x + y.x; y.y = z.y + y.y; }
        Z[idx] = y;
    }
}

// one lane per (matrix, row of the result, right-hand side), the right-hand side fastest
__global__ void __launch_bounds__(CPLX_BLOCK)
k_cplx_residual(CplxTables T, int op, long long n, long long nnz, long long k, long long total, const double2 *__restrict__ Az,
                const double2 *__restrict__ B, const double2 *__restrict__ X, double2 *__restrict__ R)
{
    CPLX_GRID_STRIDE(idx, total) {
        const long long r = idx / k, c = idx - r * k;
        const long long b = r / n, i = r - b * n;
        const double2 *az = Az + b * nnz, *x = X + b * n * k + c;
        double2 acc = B[idx];
        if (op == CS3_CPLX_N) {
            for (int p = T.rptr[i]; p < T.rptr[i + 1]; ++p) {
                const int e = T.rpos[p];
                const double2 t = cplx_mul(az[e], x[(long long) T.ecol[e] * k]);
                acc.x -= t.x; acc.y -= t.y;
            }
        } else {
            for (int e = T.Ap[i]; e < T.Ap[i + 1]; ++e) {
                double2 a = az[e];
                if (op == CS3_CPLX_H) a = cplx_conj(a);
                const double2 t = cplx_mul(a, x[(long long) T.Ai[e] * k]);
                acc.x -= t.x; acc.y -= t.y;
            }
        }
        R[idx] = acc;
    }
}

}  // namespace cs3

using namespace cs3;

namespace {

int cx_bad(const char *who, const std::string &msg) { set_error(std::string(who) + ": " + msg); return CS3_ERR_ARG; }

unsigned cx_blocks(long long total) { return (unsigned) std::min<long long>((total + CPLX_BLOCK - 1) / CPLX_BLOCK, CPLX_GRID_CAP); }

bool cx_misaligned(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

CplxTables cx_tables(cs3_cplx_s *p)
{
    return CplxTables{p->d_Ap.get(), p->d_Ai.get(), p->d_ecol.get(), p->d_dptr.get(), p->d_dpos.get(), p->d_rptr.get(), p->d_rpos.get()};
}

int cx_upload(cs3_cplx_s *p, const char *who)
{
    if (p->uploaded) return CS3_OK;
    if (no_device(who)) return CS3_ERR_HIP;
    CS3_HIP(p->d_Ap.upload(p->Ap));
    CS3_HIP(p->d_Ai.upload(p->Ai));
    CS3_HIP(p->d_ecol.upload(p->ecol));
    CS3_HIP(p->d_dptr.upload(p->dptr));
    CS3_HIP(p->d_dpos.upload(p->dpos));
    CS3_HIP(p->d_rptr.upload(p->rptr));
    CS3_HIP(p->d_rpos.upload(p->rpos));
    std::vector<double> one((size_t) (2 * p->batch * p->n), 0.0);               // s = (1, +0) until a values call says otherwise
    for (size_t r = 0; r < one.size(); r += 2) one[r] = 1.0;
    CS3_HIP(p->d_s.upload(one));
    p->uploaded = true;
    return CS3_OK;
}

int cx_op(const char *who, int64_t op, int64_t k)
{
    if (op != CS3_CPLX_N && op != CS3_CPLX_T && op != CS3_CPLX_H) return cx_bad(who, "op must be 0 (N), 1 (T) or 2 (H)");
    if (k < 0) return cx_bad(who, "k must be >= 0");
    return CS3_OK;
}

int cx_values(cs3_cplx_s *p, const double *Az, double *Rx, hipStream_t st)
{
    const double2 *az = reinterpret_cast<const double2 *>(Az);
    double2 *s = reinterpret_cast<double2 *>(p->d_s.get());
    const long long rows = (long long) p->batch * p->n, total = (long long) p->batch * p->nnz;
    if (p->rotate == CS3_CPLX_ROTATE_DIAG && rows > 0) {
        hipLaunchKernelGGL(k_cplx_rotation, dim3(cx_blocks(rows)), dim3(CPLX_BLOCK), 0, st, cx_tables(p), (long long) p->n,
                           (long long) p->nnz, rows, az, s);
        CS3_HIP(hipGetLastError());
    }
    if (total > 0) {
        hipLaunchKernelGGL(k_cplx_values, dim3(cx_blocks(total)), dim3(CPLX_BLOCK), 0, st, cx_tables(p), (long long) p->n,
                           (long long) p->nnz, total, az, s, reinterpret_cast<double2 *>(Rx));
        CS3_HIP(hipGetLastError());
    }
    return CS3_OK;
}

int cx_pack(cs3_cplx_s *p, int64_t op, const double *Z, double *Y, int64_t k, hipStream_t st)
{
    const long long total = (long long) p->batch * p->n * k;
    if (total == 0) return CS3_OK;
    hipLaunchKernelGGL(k_cplx_pack, dim3(cx_blocks(total)), dim3(CPLX_BLOCK), 0, st, (int) op, (long long) k, total,
                       reinterpret_cast<const double2 *>(Z), reinterpret_cast<const double2 *>(p->d_s.get()), Y);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int cx_unpack(cs3_cplx_s *p, int64_t op, const double *Y, double *Z, int64_t k, int64_t accumulate, hipStream_t st)
{
    const long long total = (long long) p->batch * p->n * k;
    if (total == 0) return CS3_OK;
    hipLaunchKernelGGL(k_cplx_unpack, dim3(cx_blocks(total)), dim3(CPLX_BLOCK), 0, st, (int) op, accumulate ? 1 : 0, (long long) k,
                       total, Y, reinterpret_cast<const double2 *>(p->d_s.get()), reinterpret_cast<double2 *>(Z));
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int cx_residual(cs3_cplx_s *p, int64_t op, const double *Az, const double *B, const double *X, double *R, int64_t k, hipStream_t st)
{
    const long long total = (long long) p->batch * p->n * k;
    if (total == 0) return CS3_OK;
    hipLaunchKernelGGL(k_cplx_residual, dim3(cx_blocks(total)), dim3(CPLX_BLOCK), 0, st, cx_tables(p), (int) op, (long long) p->n,
                       (long long) p->nnz, (long long) k, total, reinterpret_cast<const double2 *>(Az),
                       reinterpret_cast<const double2 *>(B), reinterpret_cast<const double2 *>(X), reinterpret_cast<double2 *>(R));
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

}  // namespace

extern "C" {

int cs3_cplx_limits(cs3_cplx_limits_t *out)
{
    if (!out) return cx_bad("cs3_cplx_limits", "null output");
    out->block = CPLX_BLOCK;
    out->grid_cap = CPLX_GRID_CAP;
    return CS3_OK;
}

int cs3_cplx_upload(cs3_cplx p)
{
    if (!p) return cx_bad("cs3_cplx_upload", "null plan");
    return cx_upload(p, "cs3_cplx_upload");
}

int cs3_cplx_workspace_dev(cs3_cplx p, int64_t slot, int64_t count, double **out)
{
    const char *who = "cs3_cplx_workspace_dev";
    if (!p || !out) return cx_bad(who, "null argument");
    if (slot < 0 || slot >= 3 || count < 0) return cx_bad(who, "slot must be 0, 1 or 2 and count >= 0");
    if (no_device(who)) return CS3_ERR_HIP;
    DevBuf<double> &w = p->ws[slot];
    if (!w.get() || (size_t) count > w.count()) {
        CS3_HIP(hipDeviceSynchronize());                            // work in flight may still read the block that goes
        CS3_HIP(w.alloc((size_t) count));
    }
    *out = w.get();
    return CS3_OK;
}

int cs3_cplx_values_dev(cs3_cplx p, const double *Az_dev, double *Rx_dev, void *stream)
{
    const char *who = "cs3_cplx_values_dev";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_upload(p, who)) return rc;                      // (CS3_ERR_HIP without a device)
    if (p->batch * p->nnz > 0 && (!Az_dev || !Rx_dev)) return cx_bad(who, "null value array");
    if (cx_misaligned(Az_dev, 16) || cx_misaligned(Rx_dev, 16)) return cx_bad(who, "value arrays must be aligned to 16 bytes");
    return cx_values(p, Az_dev, Rx_dev, (hipStream_t) stream);
}

int cs3_cplx_pack_dev(cs3_cplx p, int64_t op, const double *Z_dev, double *Y_dev, int64_t k, void *stream)
{
    const char *who = "cs3_cplx_pack_dev";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    if (p->batch * p->n * k > 0 && (!Z_dev || !Y_dev)) return cx_bad(who, "null array");
    if (cx_misaligned(Z_dev, 16) || cx_misaligned(Y_dev, 8)) return cx_bad(who, "Z must be aligned to 16 bytes, Y to 8");
    return cx_pack(p, op, Z_dev, Y_dev, k, (hipStream_t) stream);
}

int cs3_cplx_unpack_dev(cs3_cplx p, int64_t op, const double *Y_dev, double *Z_dev, int64_t k, int64_t accumulate, void *stream)
{
    const char *who = "cs3_cplx_unpack_dev";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    if (p->batch * p->n * k > 0 && (!Z_dev || !Y_dev)) return cx_bad(who, "null array");
    if (cx_misaligned(Z_dev, 16) || cx_misaligned(Y_dev, 8)) return cx_bad(who, "Z must be aligned to 16 bytes, Y to 8");
    return cx_unpack(p, op, Y_dev, Z_dev, k, accumulate, (hipStream_t) stream);
}

int cs3_cplx_residual_dev(cs3_cplx p, int64_t op, const double *Az_dev, const double *B_dev, const double *X_dev, double *R_dev,
                          int64_t k, void *stream)
{
    const char *who = "cs3_cplx_residual_dev";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    if (p->batch * p->n * k > 0 && (!B_dev || !X_dev || !R_dev || (p->nnz > 0 && !Az_dev))) return cx_bad(who, "null array");
    if (cx_misaligned(Az_dev, 16) || cx_misaligned(B_dev, 16) || cx_misaligned(X_dev, 16) || cx_misaligned(R_dev, 16))
        return cx_bad(who, "complex arrays must be aligned to 16 bytes");
    return cx_residual(p, op, Az_dev, B_dev, X_dev, R_dev, k, (hipStream_t) stream);
}

int cs3_cplx_rotation_dev(cs3_cplx p, const double **s_dev)
{
    const char *who = "cs3_cplx_rotation_dev";
    if (!p || !s_dev) return cx_bad(who, "null argument");
    if (int rc = cx_upload(p, who)) return rc;
    *s_dev = p->d_s.get();
    return CS3_OK;
}

// ---- host-array forms: the same kernels on copies (they synchronise)

int cs3_cplx_values(cs3_cplx p, const double *Az, double *Rx)
{
    const char *who = "cs3_cplx_values";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_upload(p, who)) return rc;
    const size_t total = (size_t) p->batch * (size_t) p->nnz;
    if (total == 0) return CS3_OK;
    if (!Az || !Rx) return cx_bad(who, "null value array");
    DevBuf<double> az, rx;
    CS3_HIP(az.upload(Az, 2 * total));
    CS3_HIP(rx.alloc(4 * total));
    if (int rc = cx_values(p, az.get(), rx.get(), nullptr)) return rc;
    CS3_HIP(hipMemcpy(Rx, rx.get(), 4 * total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_cplx_pack(cs3_cplx p, int64_t op, const double *Z, double *Y, int64_t k)
{
    const char *who = "cs3_cplx_pack";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    const size_t total = (size_t) p->batch * (size_t) p->n * (size_t) k;
    if (total == 0) return CS3_OK;
    if (!Z || !Y) return cx_bad(who, "null array");
    DevBuf<double> z, y;
    CS3_HIP(z.upload(Z, 2 * total));
    CS3_HIP(y.alloc(2 * total));
    if (int rc = cx_pack(p, op, z.get(), y.get(), k, nullptr)) return rc;
    CS3_HIP(hipMemcpy(Y, y.get(), 2 * total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_cplx_unpack(cs3_cplx p, int64_t op, const double *Y, double *Z, int64_t k, int64_t accumulate)
{
    const char *who = "cs3_cplx_unpack";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    const size_t total = (size_t) p->batch * (size_t) p->n * (size_t) k;
    if (total == 0) return CS3_OK;
    if (!Z || !Y) return cx_bad(who, "null array");
    DevBuf<double> z, y;
    CS3_HIP(y.upload(Y, 2 * total));
    if (accumulate) CS3_HIP(z.upload(Z, 2 * total));
    else CS3_HIP(z.alloc(2 * total));
    if (int rc = cx_unpack(p, op, y.get(), z.get(), k, accumulate, nullptr)) return rc;
    CS3_HIP(hipMemcpy(Z, z.get(), 2 * total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_cplx_residual(cs3_cplx p, int64_t op, const double *Az, const double *B, const double *X, double *R, int64_t k)
{
    const char *who = "cs3_cplx_residual";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_op(who, op, k)) return rc;
    if (int rc = cx_upload(p, who)) return rc;
    const size_t total = (size_t) p->batch * (size_t) p->n * (size_t) k;
    if (total == 0) return CS3_OK;
    if (!B || !X || !R || (p->nnz > 0 && !Az)) return cx_bad(who, "null array");
    DevBuf<double> az, b, x, r;
    CS3_HIP(az.upload(Az, 2 * (size_t) p->batch * (size_t) p->nnz));
    CS3_HIP(b.upload(B, 2 * total));
    CS3_HIP(x.upload(X, 2 * total));
    CS3_HIP(r.alloc(2 * total));
    if (int rc = cx_residual(p, op, az.get(), b.get(), x.get(), r.get(), k, nullptr)) return rc;
    CS3_HIP(hipMemcpy(R, r.get(), 2 * total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

int cs3_cplx_rotation(cs3_cplx p, double *s)
{
    const char *who = "cs3_cplx_rotation";
    if (!p) return cx_bad(who, "null plan");
    if (int rc = cx_upload(p, who)) return rc;
    const size_t total = 2 * (size_t) p->batch * (size_t) p->n;
    if (total == 0) return CS3_OK;
    if (!s) return cx_bad(who, "null output");
    CS3_HIP(hipDeviceSynchronize());                                // the last values call may be on any stream
    CS3_HIP(hipMemcpy(s, p->d_s.get(), total * 8, hipMemcpyDeviceToHost));
    return CS3_OK;
}

}  // extern "C"
