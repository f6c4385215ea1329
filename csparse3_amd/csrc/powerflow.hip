// AC power flow, device side (include/csparse3_amd.h, "AC power flow"): the two steps between a bus admittance matrix
// and the factor + solve chain of a Newton iteration, and the small kernels that keep the per-scenario state.
//
//   k_pf_mismatch   I = Y V over Y BY ROWS (ascending column, through the positions the plan recorded: no transposed
//                   values), mis = V conj(I) - S, -F into the right-hand side, max |F| per scenario.  One lane per row; a
//                   row longer than PF_WAVE_ROW gets a wave: lane l sums entries l, l + 64, ... in order, then a fixed
//                   butterfly.  The maximum of a scenario: a wave butterfly on the bit patterns of |F| (non-negative
//                   doubles order like their bits; NaN patterns order above infinity), then ONE integer atomic max per
//                   wave -- order-independent, the same bits on every run.  No float atomics.
//   k_pf_jacobian   one lane per stored entry of Y (grid-stride): up to four values through jpos.  A frozen scenario
//                   gets the identity.
//   k_pf_decide     one workgroup per scenario: reads the maximum, freezes the scenario (converged / out of iterations /
//                   not finite), zeroes its right-hand side, counts the active ones down by integer atomics.
//   k_pf_update     va[pvpq] += dx, vm[pq] += dx for the active scenarios, unless the handle's status word says that the
//                   factorisation behind dx failed.
//
// All index tables are struct-of-arrays and read coalesced by the entry kernels; stores are plain vector stores.  About
// 100 bytes move per entry of Y: these kernels cost about a launch each at the sizes of a transmission network.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/csparse3_amd.h"
#include "cs3_internal.hpp"
#include "cs3_pf.hpp"

namespace cs3 {

using u64 = unsigned long long;

constexpr u64 PF_INF_BITS = 0x7ff0000000000000ull;
constexpr int PF_STATUS_CLEAN = 0x7f7f7f7f;

struct PfTables {
    const int *jpos, *yrow, *ycol, *Rp, *Rj, *Rpos, *upos_a, *upos_m, *ubus, *wave_rows;
    int n, nnz, nwave, npvpq, nj, nnz_j;
    long long y_stride;                       // doubles between the Y values of two scenarios (0: one Y for all)
};

__device__ inline u64 pf_abs_bits(double x) { return (u64) __double_as_longlong(fabs(x)); }

// Row i with its current (ir, ii): stores it, and with injections the two mismatches.  Returns the larger bit pattern.
__device__ inline u64 pf_finish_row(const PfTables &T, int i, double ir, double ii, const double *__restrict__ S,
                                    const double *__restrict__ vm, const double *__restrict__ va, double *__restrict__ rhs,
                                    double *__restrict__ cur)
{
    cur[2 * (long long) i] = ir;
    cur[2 * (long long) i + 1] = ii;
    if (!S) return 0ull;
    double s, c;
    sincos(va[i], &s, &c);
    const double vr = vm[i] * c, vi = vm[i] * s;
    const double mr = vr * ir + vi * ii - S[2 * (long long) i];
    rhs[T.upos_a[i]] = -mr;
    u64 big = pf_abs_bits(mr);
    const int um = T.upos_m[i];
    if (um >= 0) {                            // (the imaginary part of S at a PV bus is never read)
        const double mi = vi * ir - vr * ii - S[2 * (long long) i + 1];
        rhs[um] = -mi;
        big = max(big, pf_abs_bits(mi));
    }
    return big;
}

__global__ void __launch_bounds__(PF_BLOCK)
k_pf_mismatch(PfTables T, int batch, int lane_blocks, const double *__restrict__ Yz, const double *__restrict__ S,
              const double *__restrict__ vm, const double *__restrict__ va, const int *__restrict__ state,
              double *__restrict__ rhs, double *__restrict__ cur, u64 *__restrict__ nbits)
{
    const int lane = threadIdx.x & 63;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const bool frozen = state && state[b] != 0;
        const double *y = Yz + (long long) b * T.y_stride;
        const double *Sb = S ? S + 2ll * b * T.n : nullptr;
        const double *vmb = vm + (long long) b * T.n, *vab = va + (long long) b * T.n;
        double *rb = rhs ? rhs + (long long) b * T.nj : nullptr, *cb = cur + 2ll * b * T.n;
        u64 big = 0ull;
        if ((int) blockIdx.x < lane_blocks) {
            for (long long i = (long long) blockIdx.x * PF_BLOCK + threadIdx.x; i < T.n; i += (long long) lane_blocks * PF_BLOCK) {
                const int ua = T.upos_a[i];
                if (ua < 0) continue;                                   // a reference bus
                const int p0 = T.Rp[i], p1 = T.Rp[i + 1];
                if (p1 - p0 > PF_WAVE_ROW) continue;                    // a wave's row
                if (frozen) {
                    if (Sb) { rb[ua] = 0.0; if (T.upos_m[i] >= 0) rb[T.upos_m[i]] = 0.0; }
                    continue;
                }
                double ir = 0.0, ii = 0.0;
                for (int p = p0; p < p1; ++p) {
                    const int k = T.Rj[p];
                    const long long q = T.Rpos[p];
                    const double yr = y[2 * q], yi = y[2 * q + 1];
                    double s, c;
                    sincos(vab[k], &s, &c);
                    const double wr = vmb[k] * c, wi = vmb[k] * s;
                    ir += yr * wr - yi * wi;
                    ii += yr * wi + yi * wr;
                }
                big = max(big, pf_finish_row(T, (int) i, ir, ii, Sb, vmb, vab, rb, cb));
            }
        } else {
            const int nw = ((int) gridDim.x - lane_blocks) * (PF_BLOCK / 64);
            for (int r = ((int) blockIdx.x - lane_blocks) * (PF_BLOCK / 64) + (int) (threadIdx.x >> 6); r < T.nwave; r += nw) {
                const int i = T.wave_rows[r];
                if (frozen) {
                    if (Sb && lane == 0) { rb[T.upos_a[i]] = 0.0; if (T.upos_m[i] >= 0) rb[T.upos_m[i]] = 0.0; }
                    continue;
                }
                double ir = 0.0, ii = 0.0;
                for (int p = T.Rp[i] + lane; p < T.Rp[i + 1]; p += 64) {
                    const int k = T.Rj[p];
                    const long long q = T.Rpos[p];
                    const double yr = y[2 * q], yi = y[2 * q + 1];
                    double s, c;
                    sincos(vab[k], &s, &c);
                    const double wr = vmb[k] * c, wi = vmb[k] * s;
                    ir += yr * wr - yi * wi;
                    ii += yr * wi + yi * wr;
                }
                for (int off = 32; off > 0; off >>= 1) { ir += __shfl_xor(ir, off); ii += __shfl_xor(ii, off); }
                if (lane == 0) big = max(big, pf_finish_row(T, i, ir, ii, Sb, vmb, vab, rb, cb));
            }
        }
        if (nbits) {
            for (int off = 32; off > 0; off >>= 1) big = max(big, (u64) __shfl_xor((long long) big, off));
            if (lane == 0 && big) atomicMax(&nbits[b], big);
        }
    }
}

__global__ void __launch_bounds__(PF_BLOCK)
k_pf_jacobian(PfTables T, int batch, const double *__restrict__ Yz, const double *__restrict__ vm, const double *__restrict__ va,
              const double *__restrict__ cur, const int *__restrict__ state, double *__restrict__ Jx)
{
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const bool frozen = state && state[b] != 0;
        const double *y = Yz + (long long) b * T.y_stride;
        const double *vmb = vm + (long long) b * T.n, *vab = va + (long long) b * T.n, *cb = cur + 2ll * b * T.n;
        double *J = Jx + (long long) b * T.nnz_j;
        for (long long q = (long long) blockIdx.x * PF_BLOCK + threadIdx.x; q < T.nnz; q += (long long) gridDim.x * PF_BLOCK) {
            const int ph = T.jpos[q], pn = T.jpos[T.nnz + q], pm = T.jpos[2ll * T.nnz + q], pl = T.jpos[3ll * T.nnz + q];
            if ((ph & pn & pm & pl) == -1) continue;                    // a bus type removes all four
            const int i = T.yrow[q], j = T.ycol[q];
            double h, nn, m, l;
            if (frozen) {
                h = l = (i == j) ? 1.0 : 0.0;
                nn = m = 0.0;
            } else {
                const double yr = y[2 * q], yi = y[2 * q + 1];
                double si, ci, sj, cj;
                sincos(vab[j], &sj, &cj);
                sincos(vab[i], &si, &ci);
                const double vir = vmb[i] * ci, vii = vmb[i] * si;
                const double wr = yr * cj - yi * sj, wi = yr * sj + yi * cj;       // Y_ij Vn_j
                const double ur = vir * wr + vii * wi, ui = vii * wr - vir * wi;   // V_i conj(Y_ij Vn_j): d/d|V|_j off the diagonal
                const double tr = vmb[j] * ur, ti = vmb[j] * ui;                   // V_i conj(Y_ij V_j)
                if (i != j) {
                    h = ti; m = -tr; nn = ur; l = ui;
                } else {
                    const double ir = cb[2ll * i], ii = cb[2ll * i + 1];
                    const double sr = vir * ir + vii * ii, sm = vii * ir - vir * ii;   // V_i conj(I_i)
                    h = ti - sm; m = sr - tr;
                    nn = ur + (ir * ci + ii * si);
                    l = ui + (ir * si - ii * ci);
                }
            }
            if (ph >= 0) J[ph] = h;
            if (pn >= 0) J[pn] = nn;
            if (pm >= 0) J[pm] = m;
            if (pl >= 0) J[pl] = l;
        }
    }
}

// ints: state [batch] (0 active, 1 frozen), iters [batch], flag [batch], active [1]
__global__ void __launch_bounds__(PF_BLOCK)
k_pf_init(int batch, int *__restrict__ ints, u64 *__restrict__ nbits, double *__restrict__ norm)
{
    for (int b = blockIdx.x * PF_BLOCK + threadIdx.x; b < batch; b += gridDim.x * PF_BLOCK) {
        ints[b] = 0; ints[batch + b] = 0; ints[2 * batch + b] = 0;
        nbits[b] = 0ull; norm[b] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ints[3 * batch] = batch;
}

__global__ void __launch_bounds__(PF_BLOCK)
k_pf_decide(int batch, int nj, int it, int max_iters, double tol, int *__restrict__ ints, u64 *__restrict__ nbits,
            double *__restrict__ norm, double *__restrict__ rhs)
{
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int st = ints[b];
        const u64 bits = nbits[b];
        __syncthreads();                                                // every lane has read what lane 0 now changes
        if (st == 0) {
            const double nrm = __longlong_as_double((long long) bits);
            const int fl = bits >= PF_INF_BITS ? 2 : nrm <= tol ? 0 : it == max_iters ? 1 : -1;
            if (threadIdx.x == 0) {
                norm[b] = nrm;
                nbits[b] = 0ull;
                if (fl >= 0) { ints[b] = 1; ints[batch + b] = it; ints[2 * batch + b] = fl; atomicSub(&ints[3 * batch], 1); }
            }
            if (fl >= 0)
                for (int k = threadIdx.x; k < nj; k += PF_BLOCK) rhs[(long long) b * nj + k] = 0.0;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PF_BLOCK)
k_pf_update(PfTables T, int batch, const double *__restrict__ dx, double *__restrict__ vm, double *__restrict__ va,
            const int *__restrict__ state, const int *__restrict__ status)
{
    if (status[0] != PF_STATUS_CLEAN || status[3] != 0) return;         // the factorisation behind dx failed: nothing moves
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        if (state[b] != 0) continue;
        for (int k = blockIdx.x * PF_BLOCK + threadIdx.x; k < T.nj; k += gridDim.x * PF_BLOCK) {
            const double d = dx[(long long) b * T.nj + k];
            const long long at = (long long) b * T.n + T.ubus[k];
            if (k < T.npvpq) va[at] += d; else vm[at] += d;
        }
    }
}

namespace {

PfTables pf_tables(const cs3_pf_s *p)
{
    const auto &m = p->mem;
    return PfTables{m.jpos.get(), m.yrow.get(), m.ycol.get(), m.Rp.get(), m.Rj.get(), m.Rpos.get(), m.upos_a.get(), m.upos_m.get(),
                    m.ubus.get(), m.wave_rows.get(), (int) p->n, (int) p->nnz_y, (int) p->wave_rows.size(), (int) (p->npv + p->npq),
                    (int) p->nj, (int) p->nnz_j, p->y_batch == 1 ? 0ll : 2ll * p->nnz_y};
}

unsigned pf_blocks(long long items) { return (unsigned) std::max<long long>(1, std::min<long long>((items + PF_BLOCK - 1) / PF_BLOCK, PF_GRID_CAP)); }
unsigned pf_grid_y(const cs3_pf_s *p) { return (unsigned) std::min<long long>(p->batch, 65535); }

}  // namespace

int pf_upload(cs3_pf_s *p)
{
    if (p->uploaded) return CS3_OK;
    if (no_device("the power flow")) return CS3_ERR_HIP;
    auto &m = p->mem;
    CS3_HIP(m.jpos.upload(p->jpos));
    CS3_HIP(m.yrow.upload(p->yrow));
    CS3_HIP(m.ycol.upload(p->ycol));
    CS3_HIP(m.Rp.upload(p->Rp));
    CS3_HIP(m.Rj.upload(p->Rj));
    CS3_HIP(m.Rpos.upload(p->Rpos));
    CS3_HIP(m.upos_a.upload(p->upos_a));
    CS3_HIP(m.upos_m.upload(p->upos_m));
    CS3_HIP(m.ubus.upload(p->ubus));
    CS3_HIP(m.wave_rows.upload(p->wave_rows));
    CS3_HIP(m.cur.alloc((size_t) p->batch * (size_t) p->n * 2));
    p->uploaded = true;
    return CS3_OK;
}

int pf_launch_mismatch(cs3_pf_s *p, const double *Yz, const double *S, const double *vm, const double *va, const int32_t *state,
                       double *rhs, u64 *nbits, hipStream_t st)
{
    const unsigned lane_blocks = pf_blocks(p->n);
    const unsigned wave_blocks = p->wave_rows.empty() ? 0u : pf_blocks((long long) p->wave_rows.size() * 64);
    hipLaunchKernelGGL(k_pf_mismatch, dim3(lane_blocks + wave_blocks, pf_grid_y(p)), dim3(PF_BLOCK), 0, st, pf_tables(p), (int) p->batch,
                       (int) lane_blocks, Yz, S, vm, va, state, rhs, p->mem.cur.get(), nbits);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int pf_launch_jacobian(cs3_pf_s *p, const double *Yz, const double *vm, const double *va, const int32_t *state, double *Jx,
                       hipStream_t st)
{
    hipLaunchKernelGGL(k_pf_jacobian, dim3(pf_blocks(p->nnz_y), pf_grid_y(p)), dim3(PF_BLOCK), 0, st, pf_tables(p), (int) p->batch, Yz, vm,
                       va, p->mem.cur.get(), state, Jx);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int pf_launch_init(cs3_pf_s *p, hipStream_t st)
{
    hipLaunchKernelGGL(k_pf_init, dim3(pf_blocks(p->batch)), dim3(PF_BLOCK), 0, st, (int) p->batch, p->mem.ints.get(), p->mem.nbits.get(),
                       p->mem.norm.get());
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int pf_launch_decide(cs3_pf_s *p, int it, int max_iters, double tol, hipStream_t st)
{
    hipLaunchKernelGGL(k_pf_decide, dim3((unsigned) std::min<long long>(p->batch, PF_GRID_CAP)), dim3(PF_BLOCK), 0, st, (int) p->batch,
                       (int) p->nj, it, max_iters, tol, p->mem.ints.get(), p->mem.nbits.get(), p->mem.norm.get(), p->mem.rhs.get());
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

int pf_launch_update(cs3_pf_s *p, double *vm, double *va, const int *status, hipStream_t st)
{
    hipLaunchKernelGGL(k_pf_update, dim3(pf_blocks(p->nj), pf_grid_y(p)), dim3(PF_BLOCK), 0, st, pf_tables(p), (int) p->batch,
                       p->mem.rhs.get(), vm, va, p->mem.ints.get(), status);
    CS3_HIP(hipGetLastError());
    return CS3_OK;
}

}  // namespace cs3
