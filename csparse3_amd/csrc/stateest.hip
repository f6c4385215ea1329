// AC state estimation, device side (include/csparse3_amd.h, "AC state estimation"): everything of a weighted-least-squares
// Gauss-Newton step that lies between the voltages and the chain  spgemm values -> Cholesky factor + solve.
//
//   k_se_currents   I = Y V over Y BY ROWS (ascending column, through the positions the plan recorded), for every bus, and
//                   (cos theta_i, sin theta_i) beside it: the later kernels never call sincos.  The row sum itself takes
//                   sincos of the column's angle at every stored entry, as k_pf_mismatch does (nnz_y + n calls in all): a
//                   pass that formed V once per bus first would be one more launch.  One lane per row; a row longer than
//                   SE_WAVE_ROW gets a wave: lane l sums entries l, l + 64, ... in order, then a fixed butterfly.
//   k_se_residual   one lane per measurement: h_i(x), r_i = z_i - h_i, w_i r_i, and the workgroup's partial of sum w r^2 by
//                   a fixed tree over its 256 consecutive rows.  k_se_close: one workgroup adds the partials, thread j
//                   taking j, j + 256, ... in order, then the same tree (the scheme of cs3_quad_normres).  No atomics.
//   k_se_jacobian   one lane per entry of H in row order (grid-stride): the value from the entry's descriptor, stored at up
//                   to three places: H by rows, H in CSC through cpos, w_i H_ij in CSC.
//   k_se_gradient   g_j = sum over column j of H (CSC, stored order) of Hc * (w r): one lane per column, one wave for a
//                   column longer than SE_WAVE_COL (strided, then the tree).  Every product and every sum rounded on its
//                   own, so g is defined to the bit.
//   k_se_update     va[non-ref] += dx[:na], vm += dx[na:], max |dx| by a wave butterfly on the bit patterns and ONE integer
//                   atomic max per wave (non-negative doubles order like their bits; NaN patterns order above infinity);
//                   nothing at all when the handle's status word says that the factorisation behind dx failed.
//
// Index tables are struct-of-arrays and read coalesced by the entry kernel; stores are plain vector stores.  About 60
// bytes move per entry of H and 40 per entry of Y: each kernel costs about a launch at the sizes of a transmission network.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_se.hpp"

// Every product is rounded before it is added: what a host restates, and what defines the gradient and J to the bit.
// Plain operators under this pragma, not the rounding intrinsics of the HIP headers: those are inline functions whose
// multiply and add are compiled with contraction allowed, and after inlining the two fuse (seen on the gradient).
#pragma clang fp contract(off)

namespace cs3 {

using u64 = unsigned long long;

constexpr int SE_STATUS_CLEAN = 0x7f7f7f7f;

struct SeTables {
    const int *Rp, *Rj, *Rpos, *sbus, *kind, *where, *end_from, *end_to, *Hp, *Hi, *cpos, *e_row, *e_src, *e_code, *e_bus, *wave_rows,
        *wave_cols;
    int n, nwave_rows, nwave_cols, na, ns, m, nnz_h;
};

static_assert(SE_BLOCK == 256, "four waves per workgroup: the reductions below add four wave sums");

__device__ inline double se_wave_tree(double s)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off, 64);
    return s;                                               // (lane 0 holds the sum)
}

// the four waves' sums in wave order, valid in thread 0; every thread of the workgroup calls it
__device__ inline double se_block_sum(double s, double *lds)
{
    s = se_wave_tree(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ inline void se_store_bus(double *__restrict__ cur, int i, double ir, double ii, const double *__restrict__ va)
{
    double s, c;
    sincos(va[i], &s, &c);
    double *out = cur + 4ll * i;
    out[0] = ir; out[1] = ii; out[2] = c; out[3] = s;
}

// (ir, ii) += Y_ik V_k for entry p of Y by rows
__device__ inline void se_add_term(const SeTables &T, int p, const double *__restrict__ Yz, const double *__restrict__ vm,
                                   const double *__restrict__ va, double &ir, double &ii)
{
    const int k = T.Rj[p];
    const long long q = T.Rpos[p];
    const double yr = Yz[2 * q], yi = Yz[2 * q + 1];
    double s, c;
    sincos(va[k], &s, &c);
    const double wr = vm[k] * c, wi = vm[k] * s;
    ir += yr * wr - yi * wi;
    ii += yr * wi + yi * wr;
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_currents(SeTables T, int lane_blocks, const double *__restrict__ Yz, const double *__restrict__ vm, const double *__restrict__ va,
              double *__restrict__ cur, u64 *__restrict__ dxbits)
{
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *dxbits = 0ull;           // +0.0: the maximum of the coming update starts there
    if ((int) blockIdx.x < lane_blocks) {
        for (long long i = (long long) blockIdx.x * SE_BLOCK + threadIdx.x; i < T.n; i += (long long) lane_blocks * SE_BLOCK) {
            const int p0 = T.Rp[i], p1 = T.Rp[i + 1];
            if (p1 - p0 > SE_WAVE_ROW) continue;                        // a wave's row
            double ir = 0.0, ii = 0.0;
            for (int p = p0; p < p1; ++p) se_add_term(T, p, Yz, vm, va, ir, ii);
            se_store_bus(cur, (int) i, ir, ii, va);
        }
    } else {
        const int nw = ((int) gridDim.x - lane_blocks) * (SE_BLOCK / 64);
        for (int r = ((int) blockIdx.x - lane_blocks) * (SE_BLOCK / 64) + (int) (threadIdx.x >> 6); r < T.nwave_rows; r += nw) {
            const int i = T.wave_rows[r];
            double ir = 0.0, ii = 0.0;
            for (int p = T.Rp[i] + lane; p < T.Rp[i + 1]; p += 64) se_add_term(T, p, Yz, vm, va, ir, ii);
            for (int off = 32; off > 0; off >>= 1) { ir += __shfl_xor(ir, off); ii += __shfl_xor(ii, off); }
            if (lane == 0) se_store_bus(cur, i, ir, ii, va);
        }
    }
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_residual(SeTables T, const double *__restrict__ Ye, const double *__restrict__ z, const double *__restrict__ w,
              const double *__restrict__ vm, const double *__restrict__ cur, double *__restrict__ r_plan, double *__restrict__ r_out,
              double *__restrict__ wr, double *__restrict__ parts)
{
    __shared__ double lds[4];
    const long long i = (long long) blockIdx.x * SE_BLOCK + threadIdx.x;
    double term = 0.0;
    if (i < T.m) {
        const int kind = T.kind[i], at = T.where[i];
        double h;
        if (kind == 0) {
            h = vm[at];
        } else if (kind <= 2) {
            const double *c = cur + 4ll * at;
            const double vr = vm[at] * c[2], vi = vm[at] * c[3];
            h = kind == 1 ? vr * c[0] + vi * c[1] : vi * c[0] - vr * c[1];
        } else {
            const int f = T.end_from[at], t = T.end_to[at];
            const double *y = Ye + 4ll * at, *cf = cur + 4ll * f, *ct = cur + 4ll * t;
            const double fr = vm[f] * cf[2], fi = vm[f] * cf[3], tr = vm[t] * ct[2], ti = vm[t] * ct[3];
            const double ir = (y[0] * fr - y[1] * fi) + (y[2] * tr - y[3] * ti);      // I_k = yff V_f + yft V_t
            const double ii = (y[0] * fi + y[1] * fr) + (y[2] * ti + y[3] * tr);
            h = kind == 3 ? fr * ir + fi * ii : fi * ir - fr * ii;
        }
        const double r = z[i] - h, wi = w[i];
        r_plan[i] = r;
        if (r_out) r_out[i] = r;
        wr[i] = wi * r;
        term = wi * (r * r);
    }
    const double J = se_block_sum(term, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = J;
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_close(const double *__restrict__ parts, long long nparts, double *__restrict__ J_plan, double *__restrict__ J_out)
{
    __shared__ double lds[4];
    double J = 0.0;
    for (long long g = threadIdx.x; g < nparts; g += SE_BLOCK) J = J + parts[g];
    J = se_block_sum(J, lds);
    if (threadIdx.x == 0) {
        *J_plan = J;
        if (J_out) *J_out = J;
    }
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_jacobian(SeTables T, const double *__restrict__ Yz, const double *__restrict__ Ye, const double *__restrict__ w,
              const double *__restrict__ vm, const double *__restrict__ cur, double *__restrict__ Hr, double *__restrict__ Hc,
              double *__restrict__ WHc)
{
    for (long long q = (long long) blockIdx.x * SE_BLOCK + threadIdx.x; q < T.nnz_h; q += (long long) gridDim.x * SE_BLOCK) {
        const int row = T.e_row[q], code = T.e_code[q];
        const int family = code & 3;
        double v = 1.0;
        if (family != SE_E_ONE) {
            const long long src = T.e_src[q];
            const int j = T.e_bus[q];                                   // the bus of the state this entry differentiates by
            const bool imag = code & SE_E_IMAG, mag = code & SE_E_MAG, near = code & SE_E_NEAR;
            if (family == SE_E_INJ) {
                const int i = T.where[row];
                const double *ci = cur + 4ll * i, *cj = cur + 4ll * j;
                const double yr = Yz[2 * src], yi = Yz[2 * src + 1];
                const double vir = vm[i] * ci[2], vii = vm[i] * ci[3];
                const double wr = yr * cj[2] - yi * cj[3], wi = yr * cj[3] + yi * cj[2];      // Y_ij Vn_j
                const double ur = vir * wr + vii * wi, ui = vii * wr - vir * wi;              // V_i conj(Y_ij Vn_j)
                if (!near) {
                    if (mag) v = imag ? ui : ur;
                    else v = imag ? -(vm[j] * ur) : vm[j] * ui;                               // -j V_i conj(Y_ij V_j)
                } else {
                    const double ir = ci[0], ii = ci[1];
                    if (mag) {
                        v = imag ? ui + (ir * ci[3] - ii * ci[2]) : ur + (ir * ci[2] + ii * ci[3]);
                    } else {
                        const double tr = vm[j] * ur, ti = vm[j] * ui;
                        const double sr = vir * ir + vii * ii, sm = vii * ir - vir * ii;      // V_i conj(I_i)
                        v = imag ? sr - tr : ti - sm;
                    }
                }
            } else {
                const int f = T.end_from[src], t = T.end_to[src];
                const double *y = Ye + 4 * src, *cf = cur + 4ll * f, *ct = cur + 4ll * t;
                const double fr = vm[f] * cf[2], fi = vm[f] * cf[3];
                const double wr = y[2] * ct[2] - y[3] * ct[3], wi = y[2] * ct[3] + y[3] * ct[2];  // yft Vn_t
                const double ur = fr * wr + fi * wi, ui = fi * wr - fr * wi;                  // V_f conj(yft Vn_t)
                if (!mag) {
                    const double ar = vm[t] * ur, ai = vm[t] * ui;                            // A = V_f conj(yft V_t)
                    v = near ? (imag ? ar : -ai) : (imag ? -ar : ai);                         // j A at the from-bus, -j A at the to-bus
                } else if (!near) {
                    v = imag ? ui : ur;
                } else {
                    const double tr = vm[t] * ct[2], ti = vm[t] * ct[3];
                    const double ir = (y[0] * fr - y[1] * fi) + (y[2] * tr - y[3] * ti);      // I_k
                    const double ii = (y[0] * fi + y[1] * fr) + (y[2] * ti + y[3] * tr);
                    // V_f conj(yff Vn_f) = |V_f| conj(yff);  conj(I_k) Vn_f
                    v = imag ? (ir * cf[3] - ii * cf[2]) - vm[f] * y[1] : (ir * cf[2] + ii * cf[3]) + vm[f] * y[0];
                }
            }
        }
        if (Hr) Hr[q] = v;
        if (Hc || WHc) {
            const int at = T.cpos[q];
            if (Hc) Hc[at] = v;
            if (WHc) WHc[at] = w[row] * v;
        }
    }
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_gradient(SeTables T, int lane_blocks, const double *__restrict__ Hc, const double *__restrict__ wr, double *__restrict__ g)
{
    if ((int) blockIdx.x < lane_blocks) {
        for (long long j = (long long) blockIdx.x * SE_BLOCK + threadIdx.x; j < T.ns; j += (long long) lane_blocks * SE_BLOCK) {
            const int p0 = T.Hp[j], p1 = T.Hp[j + 1];
            if (p1 - p0 > SE_WAVE_COL) continue;                        // a wave's column
            double s = 0.0;
            for (int p = p0; p < p1; ++p) s = s + Hc[p] * wr[T.Hi[p]];
            g[j] = s;
        }
    } else {
        const int lane = threadIdx.x & 63;
        const int nw = ((int) gridDim.x - lane_blocks) * (SE_BLOCK / 64);
        for (int c = ((int) blockIdx.x - lane_blocks) * (SE_BLOCK / 64) + (int) (threadIdx.x >> 6); c < T.nwave_cols; c += nw) {
            const int j = T.wave_cols[c];
            double s = 0.0;
            for (int p = T.Hp[j] + lane; p < T.Hp[j + 1]; p += 64) s = s + Hc[p] * wr[T.Hi[p]];
            s = se_wave_tree(s);
            if (lane == 0) g[j] = s;
        }
    }
}

__global__ void __launch_bounds__(SE_BLOCK)
k_se_update(SeTables T, const double *__restrict__ dx, double *__restrict__ vm, double *__restrict__ va, const int *__restrict__ status,
            u64 *__restrict__ dxbits)
{
    if (status[0] != SE_STATUS_CLEAN || status[3] != 0) return;         // the factorisation behind dx failed: nothing moves
    u64 big = 0ull;
    for (int k = blockIdx.x * SE_BLOCK + threadIdx.x; k < T.ns; k += gridDim.x * SE_BLOCK) {
        const double d = dx[k];
        const int bus = T.sbus[k];
        if (k < T.na) va[bus] += d; else vm[bus] += d;
        big = max(big, (u64) __double_as_longlong(fabs(d)));
    }
    for (int off = 32; off > 0; off >>= 1) big = max(big, (u64) __shfl_xor((long long) big, off));
    if ((threadIdx.x & 63) == 0 && big) atomicMax(dxbits, big);
}

namespace {

SeTables se_tables(const cs3_se_s *p)
{
    const auto &m = p->mem;
    return SeTables{m.Rp.get(), m.Rj.get(), m.Rpos.get(), m.sbus.get(), m.kind.get(), m.where.get(), m.end_from.get(), m.end_to.get(),
                    m.Hp.get(), m.Hi.get(), m.cpos.get(), m.e_row.get(), m.e_src.get(), m.e_code.get(), m.e_bus.get(), m.wave_rows.get(),
                    m.wave_cols.get(), (int) p->n, (int) p->wave_rows.size(), (int) p->wave_cols.size(), (int) p->na, (int) p->ns,
                    (int) p->m, (int) p->nnz_h};
}

unsigned se_blocks(long long items) { return (unsigned) std::max<long long>(1, std::min<long long>((items + SE_BLOCK - 1) / SE_BLOCK, SE_GRID_CAP)); }

}  // namespace

int se_upload(cs3_se_s *p)
{
    if (p->uploaded) return CS3_OK;
    if (no_device("the state estimation")) return CS3_ERR_HIP;
    auto &m = p->mem;
    CS3_HIP(m.Rp.upload(p->Rp));
    CS3_HIP(m.Rj.upload(p->Rj));
    CS3_HIP(m.Rpos.upload(p->Rpos));
    CS3_HIP(m.sbus.upload(p->sbus));
    CS3_HIP(m.kind.upload(p->kind));
    CS3_HIP(m.where.upload(p->where));
    CS3_HIP(m.end_from.upload(p->end_from));
    CS3_HIP(m.end_to.upload(p->end_to));
    CS3_HIP(m.Hp.upload(p->Hp));
    CS3_HIP(m.Hi.upload(p->Hi));
    CS3_HIP(m.cpos.upload(p->cpos));
    CS3_HIP(m.e_row.upload(p->e_row));
    CS3_HIP(m.e_src.upload(p->e_src));
    CS3_HIP(m.e_code.upload(p->e_code));
    CS3_HIP(m.e_bus.upload(p->e_bus));
    CS3_HIP(m.wave_rows.upload(p->wave_rows));
    CS3_HIP(m.wave_cols.upload(p->wave_cols));
    CS3_HIP(m.cur.alloc((size_t) p->n * 4));
    CS3_HIP(m.r.alloc((size_t) p->m));
    CS3_HIP(m.wr.alloc((size_t) p->m));
    CS3_HIP(m.parts.alloc(((size_t) p->m + SE_BLOCK - 1) / SE_BLOCK));
    CS3_HIP(m.jsum.alloc(1));
    CS3_HIP(m.dxbits.alloc(1));
    p->uploaded = true;
    return CS3_OK;
}

int se_launch_currents(cs3_se_s *p, const double *Yz, const double *vm, const double *va, hipStream_t st)
{
    const unsigned lane_blocks = se_blocks(p->n);
    const unsigned wave_blocks = p->wave_rows.empty() ? 0u : se_blocks((long long) p->wave_rows.size() * 64);
    hipLaunchKernelGGL(k_se_currents, dim3(lane_blocks + wave_blocks), dim3(SE_BLOCK), 0, st, se_tables(p), (int) lane_blocks, Yz, vm, va,
                       p->mem.cur.get(), p->mem.dxbits.get());
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int se_launch_residual(cs3_se_s *p, const double *Ye, const double *z, const double *w, const double *vm, double *r_out, double *J_out,
                       hipStream_t st)
{
    auto &m = p->mem;
    const long long nparts = (p->m + SE_BLOCK - 1) / SE_BLOCK;          // no grid cap: workgroup g owns rows 256 g .. 256 g + 255
    hipLaunchKernelGGL(k_se_residual, dim3((unsigned) nparts), dim3(SE_BLOCK), 0, st, se_tables(p), Ye, z, w, vm, m.cur.get(), m.r.get(),
                       r_out, m.wr.get(), m.parts.get());
    CS3_HIP(hipGetLastError());
    if (!J_out) return CS3_OK;
    hipLaunchKernelGGL(k_se_close, dim3(1), dim3(SE_BLOCK), 0, st, m.parts.get(), nparts, m.jsum.get(), J_out == m.jsum.get() ? nullptr : J_out);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int se_launch_jacobian(cs3_se_s *p, const double *Yz, const double *Ye, const double *w, const double *vm, double *Hr, double *Hc,
                       double *WHc, hipStream_t st)
{
    hipLaunchKernelGGL(k_se_jacobian, dim3(se_blocks(p->nnz_h)), dim3(SE_BLOCK), 0, st, se_tables(p), Yz, Ye, w, vm, p->mem.cur.get(), Hr, Hc,
                       WHc);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int se_launch_gradient(cs3_se_s *p, const double *Hc, const double *wr, double *g, hipStream_t st)
{
    const unsigned lane_blocks = se_blocks(p->ns);
    const unsigned wave_blocks = p->wave_cols.empty() ? 0u : se_blocks((long long) p->wave_cols.size() * 64);
    hipLaunchKernelGGL(k_se_gradient, dim3(lane_blocks + wave_blocks), dim3(SE_BLOCK), 0, st, se_tables(p), (int) lane_blocks, Hc, wr, g);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int se_launch_update(cs3_se_s *p, const double *dx, double *vm, double *va, const int *status, hipStream_t st)
{
    hipLaunchKernelGGL(k_se_update, dim3(se_blocks(p->ns)), dim3(SE_BLOCK), 0, st, se_tables(p), dx, vm, va, status, p->mem.dxbits.get());
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

}  // namespace cs3
