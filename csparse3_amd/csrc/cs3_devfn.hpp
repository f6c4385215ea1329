// Small device functions shared by the kernel translation units (kernels.hip, forest.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "cs3_device.hpp"

namespace cs3 {

// Load-then-select: a predicated `cond ? p[i] : 0` makes hipcc branch around the
// load and wait for it alone; loading from a safe address keeps loads in flight.
__device__ __forceinline__ double load_if(const double *__restrict__ p, long long off, bool ok)
{
    const double v = p[ok ? off : 0];
    return ok ? v : 0.0;
}

// 1 / x on the critical path of every pivot: v_rcp_f64 and two Newton steps (about 1 ulp) instead of the
// IEEE division sequence (div_scale / fmas / fixup, three times the dependent instructions).  A zero
// or non-finite pivot still yields inf / nan, which the pivot checks reject.
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}

// sqrt(x) and 1 / sqrt(x) together, for the Cholesky pivots: v_rsq_f64, two coupled Newton steps (Goldschmidt: g -> sqrt x,
// h -> 1 / (2 sqrt x)), one correction of the root (about 1 ulp both).  The library sqrt followed by fast_rcp is some forty
// dependent instructions on the critical path of every pivot (650 cycles per pivot measured on a one-wave panel);
// these are ten.  x <= 0 or non-finite yields nan / inf, which the pivot checks reject (they test the pivot itself).
__device__ __forceinline__ void sqrt_and_rsqrt(double x, double &s, double &rs)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double e = fma(-g, h, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    e = fma(-g, h, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    s = fma(fma(-g, g, x), h, g);
    rs = h + h;
}

// The pivot's diagonal entry of the factor and its reciprocal: LU keeps the pivot, Cholesky its root.
template <int KIND>
__device__ __forceinline__ void pivot_scale(double piv, double &dg, double &rp)
{
    if (KIND == CS3_CHOLESKY) sqrt_and_rsqrt(piv, dg, rp);
    else { dg = piv; rp = fast_rcp(piv); }
}

// Static pivot perturbation (LU, PivotRule<true>): a pivot with |p| < delta becomes +delta -- always PLUS delta: several
// kernels derive one pivot in more than one wave, with roundings of their own, and a rule that kept the sign would split
// a noise-level pivot that straddles zero between them.  NaN and +-inf fail the comparison and go on to the pivot checks
// as they are.  Returns whether the pivot was replaced.  The caller stores the replaced value where U_kk lives (the
// sweeps, the inverted diagonal blocks, slogdet and the export read it there) and -- in the one wave or thread whose
// copy of the pivot is the stored one -- counts it.  PivotRule<false>: nothing happens, and nothing is compiled.
template <class Rule>
__device__ __forceinline__ bool perturb_pivot(const Rule &rule, double &piv)
{
    if constexpr (Rule::on) {
        const bool small = fabs(piv) < rule.delta;
        piv = small ? rule.delta : piv;
        return small;
    } else {
        return false;
    }
}

// `hits` replaced pivots of matrix m: one atomic per front (or block) that had any, from one lane.
template <class Rule>
__device__ __forceinline__ void count_perturbed(const Rule &rule, long long m, int hits)
{
    if constexpr (Rule::on) {
        if (hits > 0) atomicAdd(rule.count + m, hits);
    }
}

// 1 / diagonal entry `i` of an r-row panel: the sweeps multiply by it (one division per lane instead
// of one per pivot step executed by the whole wave)
__device__ __forceinline__ double recip_diag(const double *__restrict__ L, long long i, long long r, bool ok)
{
    const double dg = L[ok ? i * (r + 1) : 0];
    return 1.0 / (ok ? dg : 1.0);
}

__device__ __forceinline__ int bcast_lane_i(int x, int k) { return __builtin_amdgcn_readlane(x, k); }   // k wave-uniform

__device__ __forceinline__ double bcast_lane(double x, int k)     // k wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void flag_column(int *status, int col)
{
    atomicMin(status, col);
}

// A lane's first rejected column, kept beside its stores instead of a flag_column between them (k_big_step): the columns
// are offered upward and the first hit wins, so bad_col is the lane's smallest rejected column.  status is an atomicMin
// over columns: one flag_column(bad_col) per lane leaves the same word as one call per rejected column.
__device__ __forceinline__ void first_rejected(bool rej, int col, bool &bad, int &bad_col)
{
    bad_col = (rej & !bad) ? col : bad_col;
    bad = bad | rej;
}

// ---- multipliers handed from wave to wave through LDS (eliminate_parts in k_big_step, the shared fronts of forest.hip) ----
// The producer stores a vector of multipliers, then the number of pivots handed over so far; the consumer polls that number.
// LDS operations of one wave complete in order, so no fence sits on the producer's pivot chain (a release fence per pivot
// measured 350 instead of 275 cycles per pivot); the counter is accessed with relaxed workgroup-scope atomics so that the
// contract with the compiler is explicit, the multipliers through volatile LDS pointers.
typedef volatile __attribute__((address_space(3))) double *lds_vdouble_ptr;
typedef __attribute__((address_space(3))) int *lds_int_ptr;

// CS3_DEBUG_WITHHOLD=1 (cs3_debug_withhold_handover): producers keep their counters back, so that every consumer runs
// into its time-out -- the test of the give-up path.  One copy per translation unit (no relocatable device code in this
// build): kernels.hip and forest.hip each export a setter.
static __device__ int g_withhold_handover = 0;

__device__ __forceinline__ void handover_publish(lds_int_ptr ready, int value, bool withhold)
{
    if (!withhold) __hip_atomic_store(ready, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Waits until the counter exceeds `need`; false when the wait was given up.  A consumer that gives up raises status[3]:
// cs3_factor_status then reports the step as failed (CS3_ERR_STATE) instead of letting a wrong factor pass.
__device__ __forceinline__ bool handover_wait(lds_int_ptr ready, int need, int *status, bool withhold)
{
    const int limit = withhold ? (1 << 8) : (1 << 22);
    for (int it = 0; __hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= need; ++it) {
        if (it >= limit) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(status + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    return true;
}

// Pins a value to the place where it was computed.  The waits split a consumer's pivot steps into basic blocks of their
// own; an FMA whose result is only read later is then SUNK past them, block after block, while the lane reads that
// feed it cannot move: their scalar results pile up (440 of them spilled to vector lanes and read back, in the Cholesky
// consumer of a four-wave front) and the FMAs all run at the end.
__device__ __forceinline__ void keep_here(double &x) { asm volatile("" : "+v"(x)); }

// ---- one wave eliminates a front of order <= 32: lane = row, 32 register columns (the forest's tasks and the level
// kernels' one-wave fronts share it).  Elimination only: column k of the registers is column k of the front for the whole
// loop (no stores, no shifting inside it); the reciprocal of the next pivot is issued right after the first column update
// of a step, behind which its latency hides.  Pivot checks only raise `suspect` (the caller then looks for the column, a
// rare path); RHS carries one vector column along (the fused forward sweep).
//
// PANEL form (UT, LU only): the caller holds only the w pivot columns in `row` (r = w here: no column beyond them is
// touched) and, in `ut`, the pivot ROWS transposed -- lane = a column to the right of the block, ut[i] = F(i, that
// column).  Step k then also applies its multipliers to them, ut[i] -= L(i, k) ut[k] (L(i, k) sits in lane i of the
// multiplier register), which leaves U12 in `ut`; the trailing matrix is left to schur_tiles (MFMA).
// `hits` takes the number of pivots the rule replaced (this wave's copy of a pivot is the stored one).
template <int KIND, bool RHS, bool UT = false, class Rule>
__device__ __forceinline__ void sub_eliminate(double (&row)[32], double &rhs, int r, int w, const Rule &rule, bool &suspect,
                                              double (&ut)[32], int &hits)
{
    constexpr int NC = 32;
    const int lane = threadIdx.x & 63;
    const double inv_tol = rule.inv_tol;
    double piv = bcast_lane(row[0], 0);
    bool hit = false;
    if constexpr (Rule::on) hit = perturb_pivot(rule, piv);
    double dg, rp;
    pivot_scale<KIND>(piv, dg, rp);
#pragma unroll
    for (int k0 = 0; k0 < NC; k0 += 8) {
      if (k0 < w) {                                             // (eight steps skipped at once past the last pivot)
#pragma unroll
       for (int k = k0; k < k0 + 8; ++k) {
        if (k < w) {
            const bool below = lane > k;
            const double l = below ? row[k] * rp : 0.0;         // multiplier, zero on and above the pivot row
            if (below) row[k] = l;
            if (KIND == CS3_CHOLESKY && lane == k) row[k] = (piv > 0.0) ? dg : -1.0;
            if constexpr (Rule::on) { if (lane == k) row[k] = piv; hits += (int) hit; }      // U_kk as it is stored
            if (KIND == CS3_LU) suspect = (int) suspect | (int) !(fabs(l) <= inv_tol) | (int) !(fabs(piv) > 0.0) | (int) !(fabs(piv) < 1.0e300);
            else suspect = (int) suspect | (int) !(piv > 0.0);
            // (the vector is scaled by what the separate forward sweep multiplies by, bit for bit: fast_rcp of the stored root)
            const double rpk = (RHS && KIND == CS3_CHOLESKY) ? fast_rcp(dg) : rp;
            if (k + 1 < NC) {
                if (KIND == CS3_LU) row[k + 1] -= l * bcast_lane(row[k + 1], k);
                else { const double lj = bcast_lane(row[k], k + 1); row[k + 1] -= l * lj; }
                piv = bcast_lane(row[k + 1], k + 1);
                if constexpr (Rule::on) hit = perturb_pivot(rule, piv);
                pivot_scale<KIND>(piv, dg, rp);
            }
            if (RHS) {                                          // forward substitution: y_k final, rows below take it
                if (KIND == CS3_CHOLESKY && lane == k) rhs *= rpk;
                rhs -= l * bcast_lane(rhs, k);
            }
#pragma unroll
            for (int j0 = (k + 2) & ~7; j0 < NC; j0 += 8) {
                if (j0 < r) {                                   // skip register groups beyond the front
                    double bc[8];
#pragma unroll
                    for (int j = (j0 > k + 2 ? j0 : k + 2); j < j0 + 8; ++j)
                        bc[j - j0] = (KIND == CS3_LU) ? bcast_lane(row[j], k) : bcast_lane(row[k], j);
#pragma unroll
                    for (int j = (j0 > k + 2 ? j0 : k + 2); j < j0 + 8; ++j) row[j] -= l * bc[j - j0];
                }
            }
            if (UT && KIND == CS3_LU) {
#pragma unroll
                for (int i0 = (k + 1) & ~7; i0 < NC; i0 += 8) {
                    if (i0 < w) {
                        double bc[8];
#pragma unroll
                        for (int i = (i0 > k + 1 ? i0 : k + 1); i < i0 + 8; ++i) bc[i - i0] = bcast_lane(l, i);
#pragma unroll
                        for (int i = (i0 > k + 1 ? i0 : k + 1); i < i0 + 8; ++i) ut[i] -= bc[i - i0] * ut[k];
                    }
                }
            }
        }
       }
      }
    }
}
template <int KIND, bool RHS, class Rule>
__device__ __forceinline__ void sub_eliminate(double (&row)[32], double &rhs, int r, int w, const Rule &rule, bool &suspect, int &hits)
{
    double none[32];
    sub_eliminate<KIND, RHS, false>(row, rhs, r, w, rule, suspect, none, hits);
}

// The pivot ROWS of an LU front by themselves, transposed: lane = a column of the front (all r of them, the pivot columns
// included), ut[i] = F(i, column) for the w pivot rows.  Row k is final when its turn comes; the rows below take
// ut[i] -= (F(i, k) / pivot) ut[k] with the multiplier formed from lane k of ut[i] -- a wave-uniform value, so this wave needs
// nothing from the wave that factors the pivot COLUMNS (sub_eliminate), and the two run side by side.  Every entry sees
// the same operations in the same order as in the one-wave panel form: U11 comes out identical in both waves (only the
// columns to the right of the block, U12, are taken from here) -- the perturbed pivots included: the same value meets
// the same comparison in both waves.  A replaced pivot goes back into lane k of ut[k]: the rows below read it there.
template <class Rule>
__device__ __forceinline__ void rows_eliminate_lu(double (&ut)[32], int w, const Rule &rule)
{
    constexpr int NC = 32;
    double piv = bcast_lane(ut[0], 0);
    if constexpr (Rule::on) perturb_pivot(rule, piv);
    double rp = fast_rcp(piv);
#pragma unroll
    for (int k0 = 0; k0 < NC; k0 += 8) {
      if (k0 < w) {
#pragma unroll
       for (int k = k0; k < k0 + 8; ++k) {
        if (k < w) {
            const double rpk = rp;
            if constexpr (Rule::on) { if ((int) (threadIdx.x & 63) == k) ut[k] = piv; }
            if (k + 1 < NC) {
                const double l1 = bcast_lane(ut[k + 1], k) * rpk;
                ut[k + 1] -= l1 * ut[k];
                piv = bcast_lane(ut[k + 1], k + 1);
                if constexpr (Rule::on) perturb_pivot(rule, piv);
                rp = fast_rcp(piv);
            }
#pragma unroll
            for (int i0 = (k + 2) & ~7; i0 < NC; i0 += 8) {
                if (i0 < w) {
                    double li[8];
#pragma unroll
                    for (int i = (i0 > k + 2 ? i0 : k + 2); i < i0 + 8; ++i) li[i - i0] = bcast_lane(ut[i], k) * rpk;
#pragma unroll
                    for (int i = (i0 > k + 2 ? i0 : k + 2); i < i0 + 8; ++i) ut[i] -= li[i - i0] * ut[k];
                }
            }
        }
       }
      }
    }
}

// ---- the trailing matrix of a front whose image lives in LDS (column-major, leading dimension ld), by
// v_mfma_f64_16x16x4 (entry (i, j) of the image at F[at(i, j)]: column-major, or the packed lower triangle for Cholesky):
//   C(i, j) - sum_{k < w} L(i, k) U(k, j)   for i, j in [w, r), in 16 x 16 tiles dealt to `nwaves`
// waves; every entry of the result is handed to out(i, j, value) exactly once (Cholesky: the tiles on and below the
// diagonal; the caller drops i < j inside a diagonal tile).  L(i, k) = F[i + k ld]; U(k, j) = F[k + j ld] (LU), or
// L(j, k) (Cholesky).  The sum runs in pivot order with fused multiply-adds, like the column-by-column updates it
// replaces (bit-equal: measured with tools/probes/mfma_f64.hip), at 64 cycles per 1024 of them instead of 490 (two lane
// reads and one FMA per column and pivot).  Tiles are computed TRANSPOSED (A operand = U, B operand = -L), so that the 16
// lanes of an output register hold 16 consecutive ROWS of one column: stores to a column-major block coalesce.
typedef double cs3_double4 __attribute__((ext_vector_type(4)));
template <int KIND, class At, class Out>
__device__ __forceinline__ void schur_tiles(const double *F, At at, int r, int w, int wave, int nwaves, Out out)
{
    const int lane = threadIdx.x & 63, mi = lane & 15, mq = lane >> 4;
    const int nt = (r - w + 15) >> 4;
    int t = 0;
    for (int tj = 0; tj < nt; ++tj) {
        for (int ti = (KIND == CS3_CHOLESKY) ? tj : 0; ti < nt; ++ti, ++t) {
            if (t % nwaves != wave) continue;                   // (wave-uniform)
            const int i = w + 16 * ti + mi;                     // my row: B operand and the outputs' lane & 15
            const int ca = w + 16 * tj + mi;                    // my column of the A operand
            const int ic = min(i, r - 1), cc = min(ca, r - 1);  // (rows / columns past the front: a copy of the last one --
                                                                //  finite values that only reach outputs nobody takes)
            cs3_double4 acc;
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] = F[at(ic, min(w + 16 * tj + mq + 4 * v, r - 1))];
#pragma unroll
            for (int k0 = 0; k0 < 32; k0 += 4) {
                if (k0 < w) {
                    const int k = k0 + mq;
                    const bool kin = k < w;
                    const int kc = kin ? k : 0;
                    const double au = F[(KIND == CS3_LU) ? at(kc, cc) : at(cc, kc)];
                    const double bl = F[at(ic, kc)];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kin ? au : 0.0, kin ? -bl : 0.0, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int c = w + 16 * tj + mq + 4 * v;
                if (i < r && c < r) out(i, c, acc[v]);
            }
        }
    }
}

// ---- k_big_step (kernels.hip): its descriptor in one fetch, and the addresses of a tile's loads and stores ----
// The first 64 bytes of a front's descriptor (lpan .. w) in ONE scalar load, before any early return tests a field: field
// by field the compiler split the fetch along the kernel's returns, each part a dependent scalar round trip of its own.
struct DescHead { long long lpan, dbuf; int c0, r, w; };
__device__ __forceinline__ DescHead load_desc_head(const FrontDesc *d)
{
    static_assert(offsetof(FrontDesc, lpan) == 0 && offsetof(FrontDesc, dbuf) == 32 && offsetof(FrontDesc, c0) == 52 &&
                  offsetof(FrontDesc, r) == 56 && offsetof(FrontDesc, w) == 60 && sizeof(FrontDesc) >= 64, "DescHead");
    typedef int v16i __attribute__((ext_vector_type(16), aligned(8), may_alias));
    const v16i h = *reinterpret_cast<const v16i *>(d);
    return {(long long) (((unsigned long long) (unsigned) h[1] << 32) | (unsigned) h[0]),
            (long long) (((unsigned long long) (unsigned) h[9] << 32) | (unsigned) h[8]), h[13], h[14], h[15]};
}

// Addresses: ONE wave-uniform 64-bit base per operand panel, in scalar registers, plus a 32-bit byte offset per thread --
// the thread's entry in the panel's first column group, advanced by a uniform 32-bit stride from group to group:
// global_load v, v_off, s[base].  An offset stays inside one tile (below 64 (r + 1) doubles: 32 bits hold it for any
// front that fits the memory; launch_big_block refuses the rest).  With a 64-bit address per load and thread
// (v_mad_i64_i32, compare, two selects, 64-bit add) the arithmetic alone stood between the descriptor and the first load
// for some 800 instructions, and a lone wave issues one instruction in four cycles whatever its kind.
// (The empty asm statements only hide a value's origin from the optimiser, so that base + zext(offset) reaches
// instruction selection in one piece and a bound stays one compare.  They change no result; what they buy was read off the
// gfx950 assembly of ROCm 7.2's compiler, AMD clang 22.0.0git, and is to be read again after a compiler change.)
__device__ __forceinline__ double load_at(const char *base, unsigned off)
{
    asm("" : "+v"(off));
    return *reinterpret_cast<const double *>(base + off);
}
__device__ __forceinline__ void store_at(char *base, unsigned off, double v)
{
    asm("" : "+v"(off));
    *reinterpret_cast<double *>(base + off) = v;
}
// A thread's bound on the column groups of a panel, 0 where it has no entry in any of them: one compare per load
__device__ __forceinline__ int lane_limit(bool ok, int lim)
{
    int x = ok ? lim : 0;
    asm("" : "+v"(x));
    return x;
}

// What a tile of k_big_step addresses its operands with: the front as bytes, a column in bytes (ld8; as an offset: ldu),
// the block step [kb, kb + bw) and the previous panel [kp, kp + pw), the tile's rows and columns, the thread's wave (a
// scalar, 0 .. 7) and lane indices, and its offsets: entry (l32, h5) of a panel with 32 rows (h5 = tid / 32, 0 .. 15), row
// l64 of the tile's rows / columns.
constexpr int BIG_THREADS = 512;              // k_big_step: eight waves per workgroup
struct BigTile {
    char *Fb;
    long long ld8;
    unsigned ldu;
    int kb, bw, kp, pw, row0, nrow, col0, ncol, wu, l32, h5;
    unsigned o_kj, o_row, o_col;
};

// The operand panels of the previous block step, RAW: where an entry does not exist the offset is 0 (a panel's first
// entry always exists) and the caller masks the value where it uses it.  Entry e = tid + 512 q of a panel is
// (e % 64, e / 64) = (l64, wu + 8 q) or (e % 32, e / 32) = (l32, h5 + 16 q).
// The 64-wide panels of a tile: ra (A: the L panel of the tile's rows) and rb (B: the U panel of its columns; Cholesky:
// the L panel of its columns).  A block-column tile asks for ra only and a block-row tile for rb only: the other panel of
// theirs is the diagonal block's (big_diag_panels), entry for entry.
template <int KIND, bool A, bool B>
__device__ __forceinline__ void big_tile_panels(const BigTile &t, double (&ra)[4], double (&rb)[4])
{
    const char *pa = t.Fb + 8ll * t.row0 + t.kp * t.ld8;       // L(row0 + l64, kp + wu + 8 q)
    const char *pb = (KIND == CS3_LU) ? t.Fb + 8ll * t.kp + t.col0 * t.ld8 : t.Fb + 8ll * t.col0 + t.kp * t.ld8;
    const int lim_b = lane_limit(t.l32 < t.pw, t.ncol - t.h5); // LU: entry (l32, h5 + 16 q) exists iff 16 q < lim_b
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned k_off = t.wu + 8 * q < t.pw ? (unsigned) (t.wu + 8 * q) * t.ldu : 0u;    // (a scalar)
        if (A) ra[q] = load_at(pa, t.o_row + k_off);
        if (B) rb[q] = load_at(pb, (KIND == CS3_LU) ? (16 * q < lim_b ? t.o_kj + 16 * q * t.ldu : 0u) : t.o_col + k_off);
    }
}

// The 32-wide panels of the diagonal block D = F[kb:ke, kb:ke], for the tiles that need it: rad (L(kb + l32, kp + h5 + 16 q))
// and rbd (U(kp + l32, kb + h5 + 16 q); Cholesky: rad again)
template <int KIND>
__device__ __forceinline__ void big_diag_panels(const BigTile &t, double (&rad)[2], double (&rbd)[2])
{
    const char *pad = t.Fb + 8ll * t.kb + t.kp * t.ld8;
    const char *pbd = (KIND == CS3_LU) ? t.Fb + 8ll * t.kp + t.kb * t.ld8 : pad;
    const int lim_ad = lane_limit(t.l32 < t.bw, t.pw - t.h5);
    const int lim_bd = (KIND == CS3_LU) ? lane_limit(t.l32 < t.pw, t.bw - t.h5) : lim_ad;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        rad[q] = load_at(pad, 16 * q < lim_ad ? t.o_kj + 16 * q * t.ldu : 0u);
        rbd[q] = load_at(pbd, 16 * q < lim_bd ? t.o_kj + 16 * q * t.ldu : 0u);
    }
}

// NCB of the tile's accumulators, the column blocks cb0 .. cb0 + NCB - 1 (cb0 a scalar): acc[c][v] = F(row0 + ti,
// col0 + 16 (cb0 + c) + 4 v + mq), RAW in the same way (o_acc: the thread's entry at cb = v = 0).  A plain trailing tile
// wave takes two: of a plain trailing tile and of a block-row tile the two it is dealt, of a block-column tile the two that
// the tile's 32 columns fill.
template <int NCB, class V4>
__device__ __forceinline__ void big_tile_accumulators(const BigTile &t, int ti, int mq, int cb0, V4 (&acc)[NCB])
{
    const unsigned o_acc = 8u * (unsigned) ti + (unsigned) mq * t.ldu;
    const char *pc = t.Fb + 8ll * t.row0 + t.col0 * t.ld8;
    const int lim_c = lane_limit(ti < t.nrow, t.ncol - mq - 16 * cb0);   // column 16 (cb0 + c) + 4 v + mq exists iff 16 c + 4 v < lim_c
#pragma unroll
    for (int c = 0; c < NCB; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            acc[c][v] = load_at(pc, 16 * c + 4 * v < lim_c ? o_acc + (unsigned) (16 * (cb0 + c) + 4 * v) * t.ldu : 0u);
}

// The two accumulator blocks of a wave of a block-column or block-row tile, whatever its role: acc[c][v] = M(ri, j0 + 16 c +
// 4 v + mq) of the nr x nc matrix M that starts at pm (all of them scalars but ri) -- the tile for a tile wave, the diagonal
// block for a D wave, which uses acc[0] alone (acc[1] then holds the entries of D's next sub-block, or its first entry).
// ONE code path for both roles: with the loads behind a branch on the role, the D waves waited for three of their panel
// loads before they issued their accumulator loads (a wave's registers were the other role's pending destinations to the
// compiler's wait counting): not every load of theirs was out before their first wait.
template <class V4>
__device__ __forceinline__ void big_wave_accumulators(const BigTile &t, const char *pm, int ri, int nr, int nc, int mq, int j0, V4 (&acc)[2])
{
    const unsigned o_acc = 8u * (unsigned) ri + (unsigned) mq * t.ldu;
    const int lim = lane_limit(ri < nr, nc - mq - j0);         // column j0 + 16 c + 4 v + mq exists iff 16 c + 4 v < lim
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            acc[c][v] = load_at(pm, 16 * c + 4 * v < lim ? o_acc + (unsigned) (j0 + 16 * c + 4 * v) * t.ldu : 0u);
}

// ... and of the diagonal block, for the diagonal tile: dacc[v] = F(kb + dr, kb + j0 + 4 v + mq)
template <class V4>
__device__ __forceinline__ void big_diag_accumulator(const BigTile &t, int dr, int mq, int j0, V4 &dacc)
{
    const unsigned o_d = 8u * (unsigned) dr + (unsigned) mq * t.ldu;
    const char *pd = t.Fb + 8ll * t.kb + t.kb * t.ld8;
    const int lim_d = lane_limit(dr < t.bw, t.bw - mq - j0);   // column j0 + 4 v + mq exists iff 4 v < lim_d
#pragma unroll
    for (int v = 0; v < 4; ++v) dacc[v] = load_at(pd, 4 * v < lim_d ? o_d + (unsigned) (j0 + 4 * v) * t.ldu : 0u);
}

// The LDS of k_big_step as its panel tiles use it: As[k][i] = -L(row0 + i, kp + k), Bs[k][j] = U(kp + k, col0 + j), Ad / Bd
// the same for the diagonal block, D the block itself and T the tile that is stacked under it
struct BigLds {
    double (&As)[BIG_NB][64 + 1], (&Bs)[BIG_NB][64 + 1], (&Ad)[BIG_NB][BIG_NB + 1], (&Bd)[BIG_NB][BIG_NB + 1];
    double (&D)[BIG_NB][BIG_NB + 1], (&T)[64][BIG_NB + 1];
};

// A panel tile of k_big_step (the diagonal tile, a block-column tile: bj == 0, or a block-row tile) up to the point where
// the updated diagonal block D (identity-padded past bw) and the tile T meet in LDS: the update of the previous panel,
// for the 16 x 16 blocks that the 32-wide panel uses and no others, dealt to eight waves.  All eight load and stage the
// operand panels (entry tid + 512 q); the accumulators go by role, and the role is a scalar (t.wu): tw = wv & 3 is a
// wave's place among the four of its role.  Every kind issues ALL of its loads before its first wait (the kernel's header
// says why):
//   diagonal tile (0, 0)  D alone: waves 0 .. 3 own its four sub-blocks (tw & 1, tw >> 1), 8 MFMAs each (it has no tile of
//                         its own: T is only read for bi > 0 or bj > 0); waves 4 .. 7 load and stage, and all eight
//                         send the parked block home (send_home)
//   block-column tile     waves 0 .. 3: the tile's 32 columns, row block tw with acc[0 .. 1], 16 MFMAs.  Its U panel IS D's
//                         (col0 = kb, ncol = bw: Bs would repeat Bd entry for entry), so the tile MFMAs read Bd.  Waves
//                         4 .. 7: D's four sub-blocks, 8 MFMAs
//   block-row tile (LU)   waves 0 .. 3: the tile's 32 rows -- wave tw takes row block tw & 1 (ONE B operand feeds both of its
//                         chains) and the column blocks 2 (tw >> 1), 2 (tw >> 1) + 1, and writes them to T[col][row]
//                         itself, 16 MFMAs.  Its L panel is D's (row0 = kb, nrow = bw): Ad.  Waves 4 .. 7: D, 8 MFMAs
// Every entry's sum keeps its terms, their order (k0 upward, the MFMA's own order inside a group of four), its operand
// roles (A = U, B = -L) and the zero padding past pw whichever wave forms it: the bits are those of the full 64 x 64 tile
// path.  The D chain runs in waves of its own beside the tile chains, not behind them.  stamp(p): the profiling stamps
// 0 .. 2 (thread 0: a tile wave of the block-column tile, a D wave of the diagonal tile).
template <int KIND, class Home, class Stamp>
__device__ __forceinline__ void big_panel_tile(const BigTile &t, const BigLds &s, int tid, bool diag, bool col, Home send_home, Stamp stamp)
{
    auto &As = s.As; auto &Bs = s.Bs; auto &Ad = s.Ad; auto &Bd = s.Bd; auto &D = s.D; auto &T = s.T;
    const int kb = t.kb, bw = t.bw, pw = t.pw, nrow = t.nrow, ncol = t.ncol;
    const int tw = (tid >> 6) & 3, mi = tid & 15, mq = (tid >> 4) & 3;
    const int twu = t.wu & 3;                       // tw, as a scalar
    const bool own_d = diag ? t.wu < 4 : t.wu >= 4; // (a scalar) my wave forms a sub-block of D
    const int ti = 16 * tw + mi;                    // tile row of the block-column tile's accumulators
    // D: wave tw of its four owns the 16 x 16 sub-block (tw & 1, tw >> 1): dacc[v] = D(dr, dc0 + 4 v)
    const int dr = 16 * (tw & 1) + mi, dc0 = 16 * (tw >> 1) + mq;
    double rad[2] = {0.0, 0.0}, rbd[2] = {0.0, 0.0};
    // a wave's two accumulators; a D wave keeps its sub-block in the first (the loads of both roles are one code path)
    cs3_double4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    cs3_double4 &dacc = acc[0];
    const char *pdiag = t.Fb + 8ll * t.kb + t.kb * t.ld8;
    auto mask_d = [&]() {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (!(dr < bw && dc0 + 4 * v < bw)) dacc[v] = 0.0;
    };
    auto stage_d = [&]() {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + BIG_THREADS * q;
            { const int i = e % BIG_NB, k = e / BIG_NB; Ad[k][i] = (k < pw && i < bw) ? -rad[q] : 0.0; }
            if (KIND == CS3_LU) { const int k = e % BIG_NB, j = e / BIG_NB; Bd[k][j] = (k < pw && j < bw) ? rbd[q] : 0.0; }
            else { const int j = e % BIG_NB, k = e / BIG_NB; Bd[k][j] = (k < pw && j < bw) ? rbd[q] : 0.0; }
        }
    };
    auto update_d = [&]() {
#pragma unroll
        for (int k0 = 0; k0 < BIG_NB; k0 += 4)
            dacc = __builtin_amdgcn_mfma_f64_16x16x4f64(Bd[k0 + mq][16 * (tw >> 1) + mi], Ad[k0 + mq][dr], dacc, 0, 0, 0);
    };
    auto put_d = [&]() {                            // the updated D, identity-padded past bw
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = dc0 + 4 * v;
            D[dr][j] = (dr < bw && j < bw) ? dacc[v] : (dr == j ? 1.0 : 0.0);
        }
    };
    if (diag) {                                     // ---- diagonal tile
        if (kb > 0) big_diag_panels<KIND>(t, rad, rbd);
        if (own_d) big_diag_accumulator(t, dr, mq, 16 * (twu >> 1), dacc);
        __builtin_amdgcn_sched_barrier(0);
        stamp(0);
        send_home();
        if (own_d) mask_d();
        if (kb > 0) stage_d();
        __syncthreads();
        stamp(1);
        if (own_d && kb > 0) update_d();
        stamp(2);
        if (own_d) put_d();
    } else if (col) {                               // ---- block-column tile: D and T[row][col], 32 columns
        double ra[4], rb[4];                        // (rb stays unused)
        if (kb > 0) {
            big_tile_panels<KIND, true, false>(t, ra, rb);
            big_diag_panels<KIND>(t, rad, rbd);
        }
        big_wave_accumulators(t, own_d ? pdiag : t.Fb + 8ll * t.row0 + t.col0 * t.ld8, own_d ? dr : ti, own_d ? bw : nrow, ncol,
                              mq, own_d ? 16 * (twu >> 1) : 0, acc);     // (ncol = bw)
        __builtin_amdgcn_sched_barrier(0);
        stamp(0);
        if (own_d) mask_d();
        else {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = 16 * cb + mq + 4 * v;
                    if (!(ti < nrow && j < ncol)) acc[cb][v] = 0.0;
                }
        }
        if (kb > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = tid + BIG_THREADS * q;
                const int i = e % 64, k = e / 64;
                As[k][i] = (k < pw && i < nrow) ? -ra[q] : 0.0;     // negated: the MFMA accumulates acc += U' (-L)'
            }
            stage_d();
        }
        __syncthreads();
        stamp(1);
        if (own_d) {
            if (kb > 0) update_d();
            put_d();
        } else {
            if (kb > 0) {
#pragma unroll
                for (int k0 = 0; k0 < BIG_NB; k0 += 4) {
                    const double bl = As[k0 + mq][ti];
                    const double au0 = Bd[k0 + mq][mi], au1 = Bd[k0 + mq][16 + mi];
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(au0, bl, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(au1, bl, acc[1], 0, 0, 0);
                }
            }
            stamp(2);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int v = 0; v < 4; ++v) T[ti][16 * cb + mq + 4 * v] = acc[cb][v];
        }
    } else if constexpr (KIND == CS3_LU) {          // ---- block-row tile: D and T[col][row], 32 rows
        const int cb0 = 2 * (twu >> 1);             // my column blocks cb0, cb0 + 1; my rows are those of D's sub-block: dr
        double ra[4], rb[4];                        // (ra stays unused)
        if (kb > 0) {
            big_tile_panels<KIND, false, true>(t, ra, rb);
            big_diag_panels<KIND>(t, rad, rbd);
        }
        big_wave_accumulators(t, own_d ? pdiag : t.Fb + 8ll * t.row0 + t.col0 * t.ld8, dr, bw, own_d ? bw : ncol,
                              mq, 16 * (own_d ? twu >> 1 : cb0), acc);   // (nrow = bw)
        __builtin_amdgcn_sched_barrier(0);
        if (own_d) mask_d();
        else {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = 16 * (cb0 + c) + mq + 4 * v;
                    if (!(dr < nrow && j < ncol)) acc[c][v] = 0.0;
                }
        }
        if (kb > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = tid + BIG_THREADS * q;
                const int k = e % BIG_NB, j = e / BIG_NB;
                Bs[k][j] = (k < pw && j < ncol) ? rb[q] : 0.0;
            }
            stage_d();
        }
        __syncthreads();
        if (own_d) {
            if (kb > 0) update_d();
            put_d();
        } else {
            if (kb > 0) {
#pragma unroll
                for (int k0 = 0; k0 < BIG_NB; k0 += 4) {
                    const double bl = Ad[k0 + mq][dr];          // -L(kb + dr, k0 + mq): the tile's rows are D's
                    const double au0 = Bs[k0 + mq][16 * cb0 + mi], au1 = Bs[k0 + mq][16 * cb0 + 16 + mi];
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(au0, bl, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(au1, bl, acc[1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) T[16 * (cb0 + c) + mq + 4 * v][dr] = acc[c][v];
        }
    }
}

}  // namespace cs3

