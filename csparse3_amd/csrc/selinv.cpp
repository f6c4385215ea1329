// The plan of a selected inversion (cs3_selinv_*), from the symbolic analysis alone: the fronts in top-down order, their
// launch groups, the offsets of their blocks in zpool and where an entry Z(k, l) sits.  Kernels: selinv.hip.
#include <algorithm>

#include "cs3_device.hpp"

namespace cs3 {

namespace {

i32 order_of(const Symbolic &S, i32 s) { return (i32) (S.st_ptr[s + 1] - S.st_ptr[s]); }

int class_of(i32 r) { return r <= SELINV_WAVE_R ? SELINV_WAVE : r <= SELINV_LDS_R ? SELINV_LDS : SELINV_BIG; }

unsigned ceil_div(i64 a, i64 b) { return (unsigned) ((a + b - 1) / b); }

}  // namespace

void build_selinv_plan(const Symbolic &S, SelinvPlan &P)
{
    P = SelinvPlan();
    const i32 ns = S.nsuper;
    std::vector<i32> order(ns);
    for (i32 s = 0; s < ns; ++s) order[s] = s;
    // parents before children: level descending; inside a level by class, then by supernode (a fixed order)
    std::stable_sort(order.begin(), order.end(), [&](i32 a, i32 b) {
        if (S.sn_level[a] != S.sn_level[b]) return S.sn_level[a] > S.sn_level[b];
        return class_of(order_of(S, a)) < class_of(order_of(S, b));
    });
    P.z_off.assign(ns, 0);
    for (i32 s : order) {
        const i64 r = order_of(S, s);
        P.z_off[s] = P.zpool_doubles;
        P.zpool_doubles += r * r;
    }
    P.fronts.resize(ns);
    P.front_sn = order;
    P.front_launch.assign(ns, 0);
    for (i32 t = 0; t < ns; ++t) {
        const i32 s = order[t], par = S.sn_parent[s];
        SelFront &f = P.fronts[t];
        f = SelFront();
        f.lpan = S.lpan_off[s]; f.upan = S.upan_off[s];
        f.u_sk = S.u_sk[s]; f.u_sj = S.u_sj[s];
        f.r = order_of(S, s); f.w = S.sn_ptr[s + 1] - S.sn_ptr[s];
        f.z = P.z_off[s];
        f.zpar = par >= 0 ? P.z_off[par] : 0;
        f.rpar = par >= 0 ? order_of(S, par) : 0;
        f.rel = S.rel_ptr[s];
        const int cls = class_of(f.r);
        const i64 c = f.r - f.w;
        if (cls == SELINV_BIG) { f.wk = P.work_doubles; P.work_doubles += 2 * c * f.w; P.nbig += 1; }
        else P.nsmall += 1;
        if (P.groups.empty() || P.groups.back().cls != cls || S.sn_level[order[P.groups.back().first]] != S.sn_level[s]) {
            SelinvGroup g{};
            g.cls = cls; g.first = t; g.launch = (int) P.nlaunches;
            P.groups.push_back(g);
            P.nlaunches += cls == SELINV_BIG ? 3 : 1;
        }
        SelinvGroup &g = P.groups.back();
        g.count += 1;
        g.max_r = std::max(g.max_r, f.r);
        if (cls == SELINV_BIG) {
            // slices of X, of Y and of the identity, then the gather of Z_CC (at least one workgroup, 16 entries per thread)
            const unsigned gather = std::max(1u, std::min(256u, ceil_div(c * c, 4096)));
            g.grid_prep = std::max(g.grid_prep, 2 * ceil_div(c, SELINV_SLICE) + ceil_div(f.w, SELINV_SLICE) + gather);
            const i64 tc = ceil_div(c, SELINV_TILE), tw = ceil_div(f.w, SELINV_TILE);
            g.grid_cross = std::max(g.grid_cross, std::max(1u, ceil_div(2 * tc * tw, 4)));
            g.grid_pivot = std::max(g.grid_pivot, ceil_div(tw * tw, 4));
        }
        P.front_launch[t] = g.launch;
    }
}

i64 selinv_position(const Symbolic &S, const SelinvPlan &P, i64 k, i64 l)
{
    const i64 lo = std::min(k, l), hi = std::max(k, l);
    const i32 s = S.col2sn[lo];
    const i64 c0 = S.sn_ptr[s], r = order_of(S, s);
    const i32 *st = S.st_idx.data() + S.st_ptr[s];
    const i32 *it = std::lower_bound(st, st + r, (i32) hi);
    if (it == st + r || *it != hi) return -1;
    const i64 at_lo = lo - c0, at_hi = it - st;
    return P.z_off[s] + (k == lo ? at_lo : at_hi) + (l == lo ? at_lo : at_hi) * r;
}

}  // namespace cs3
