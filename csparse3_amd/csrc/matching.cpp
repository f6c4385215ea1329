// Maximum-product transversal with scalings (Duff & Koster; MC64 job 5; the weighted relative of cs_maxtrans): the
// step that makes static diagonal pivots safe on matrices without a strong diagonal.  Host code, sequential by nature
// (shortest augmenting paths), like the ordering next to it.
//
// With c_ij = log max_i |a_ij| - log |a_ij| >= 0 the transversal of largest product is the perfect matching of least cost.
// Duals u_i (rows), v_j (columns) with u_i + v_j <= c_ij, equality on matched entries, are kept throughout; at the end
//     dr_i = exp(u_i),  dc_j = exp(v_j) / max_i |a_ij|   give   |dr_i a_ij dc_j| = exp(u_i + v_j - c_ij) <= 1, = 1 matched.
// An entry whose value is exactly 0 is absent.  Every choice among equals takes the lowest index, so the result is the same
// on every run.
#include <algorithm>
#include <cmath>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

#include "cs3_internal.hpp"

namespace cs3 {

i64 match_scale(i64 n, const i32 *Ap, const i32 *Ai, const double *Ax, i32 *rowperm, double *dr, double *dc)
{
    const i64 nnz = n > 0 ? Ap[n] : 0;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> cost((size_t) nnz), amax((size_t) n, 0.0), u((size_t) n, inf), v((size_t) n, inf);
    // costs; -1 marks an absent entry (a stored zero)
    for (i64 j = 0; j < n; ++j) {
        for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) amax[j] = std::max(amax[j], std::fabs(Ax[p]));
        const double lmax = amax[j] > 0.0 ? std::log(amax[j]) : 0.0;
        for (i64 p = Ap[j]; p < Ap[j + 1]; ++p)
            cost[p] = Ax[p] == 0.0 ? -1.0 : std::max(0.0, lmax - std::log(std::fabs(Ax[p])));
    }
    // cheap initial assignment: u_i = min_j c_ij, v_j = min_i (c_ij - u_i), then every column takes its first free row
    // among its tight entries
    for (i64 p = 0; p < nnz; ++p)
        if (cost[p] >= 0.0) u[Ai[p]] = std::min(u[Ai[p]], cost[p]);
    for (i64 i = 0; i < n; ++i) if (u[i] == inf) u[i] = 0.0;
    std::vector<i32> mrow((size_t) n, -1), mcol((size_t) n, -1);      // column of a row, row of a column
    for (i64 j = 0; j < n; ++j) {
        for (i64 p = Ap[j]; p < Ap[j + 1]; ++p)
            if (cost[p] >= 0.0) v[j] = std::min(v[j], cost[p] - u[Ai[p]]);
        if (v[j] == inf) { v[j] = 0.0; continue; }
        i32 best = -1;
        for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) {
            const i32 i = Ai[p];
            if (cost[p] >= 0.0 && cost[p] - u[i] == v[j] && mrow[i] < 0 && (best < 0 || i < best)) best = i;
        }
        if (best >= 0) { mrow[best] = (i32) j; mcol[j] = best; }
    }
    // shortest augmenting paths from every column that is still free (Dijkstra on the reduced costs)
    using Key = std::pair<double, i32>;                                // (distance, row): ties go to the lowest row
    std::priority_queue<Key, std::vector<Key>, std::greater<Key>> heap;
    std::vector<double> dist((size_t) n, inf);
    std::vector<i32> pred((size_t) n, -1), touched, tree;
    std::vector<char> done((size_t) n, 0);
    i64 matched = 0;
    for (i64 j = 0; j < n; ++j) matched += mcol[j] >= 0;
    for (i64 j0 = 0; j0 < n; ++j0) {
        if (mcol[j0] >= 0) continue;
        touched.clear(); tree.clear();
        heap = decltype(heap)();
        i64 j = j0;
        double lsp = 0.0;                                              // length of the shortest path to column j
        i32 ifree = -1;
        for (;;) {
            for (i64 p = Ap[j]; p < Ap[j + 1]; ++p) {
                const i32 i = Ai[p];
                if (cost[p] < 0.0 || done[i]) continue;
                const double dn = lsp + std::max(0.0, cost[p] - u[i] - v[j]);
                if (dn < dist[i]) {
                    if (dist[i] == inf) touched.push_back(i);
                    dist[i] = dn; pred[i] = (i32) j;
                    heap.push(Key(dn, i));
                }
            }
            i32 i = -1;
            while (!heap.empty()) {
                const Key top = heap.top();
                heap.pop();
                if (!done[top.second] && top.first == dist[top.second]) { i = top.second; break; }
            }
            if (i < 0) break;                                          // no augmenting path: column j0 stays free
            done[i] = 1;
            if (mrow[i] < 0) { ifree = i; break; }
            tree.push_back(i);
            j = mrow[i];
            lsp = dist[i];
        }
        if (ifree >= 0) {
            const double delta = dist[ifree];
            for (i32 i : tree) { u[i] -= delta - dist[i]; v[mrow[i]] += delta - dist[i]; }
            v[j0] += delta;
            for (i32 i = ifree;;) {                                    // flip the path back to j0
                const i32 jc = pred[i], inext = mcol[jc];
                mcol[jc] = i; mrow[i] = jc;
                if (jc == j0) break;
                i = inext;
            }
            matched += 1;
        }
        for (i32 i : touched) { dist[i] = inf; done[i] = 0; }
    }
    if (matched < n) return matched;
    // the matched entry of every column exactly tight (the dual updates above round)
    for (i64 j = 0; j < n; ++j) {
        double c = inf;                                                // (the cheapest, should the entry be stored twice)
        for (i64 p = Ap[j]; p < Ap[j + 1]; ++p)
            if (Ai[p] == mcol[j] && cost[p] >= 0.0) c = std::min(c, cost[p]);
        v[j] = c - u[mcol[j]];
    }
    for (i64 j = 0; j < n; ++j) {
        rowperm[j] = mcol[j];
        dr[j] = std::exp(u[j]);
        dc[j] = std::exp(v[j]) / amax[j];
    }
    return matched;
}

}  // namespace cs3
