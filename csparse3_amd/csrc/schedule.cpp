// The launch schedule: which launch goes to which stream, in what order, behind which event.  Pure host code, no HIP call:
// the planners below turn the launch groups of a handle into a LaunchPlan (cs3_device.hpp), issue_plan in kernels.hip
// issues it, cs3_debug_launch_plan prints it.
#include <algorithm>
#include <cstdlib>

#include "cs3_device.hpp"

namespace cs3 {

static bool env_is_1(const char *name) { return getenv(name) && getenv(name)[0] == '1'; }

bool gemm_sweeps_on()
{
    static const bool on = !env_is_1("CS3_NO_GEMM_SWEEPS");
    return on;
}

// The permutations can ride on the sweeps when every pivot row of X is read (forward) and written (backward) by a kernel
// that knows the row map: the lane = right-hand-side kernels and the GEMM sweeps, i.e. 16 or more right-hand sides, no
// interleaved batch, GEMM sweeps on.
bool permutation_can_fuse(const DeviceFactor &D, int nrhs)
{
    // (measured on config 4: the extra row-map round trip per front costs more than the two permutation kernels below a
    // few hundred right-hand sides; at 1024 the fused form saves 0.14 ms of 2.3)
    constexpr int min_rhs = 256;
    return gemm_sweeps_on() && nrhs >= std::max(min_rhs, RHS_LANES_MIN) && D.il_len == 0;
}

// One workgroup per (big front, matrix) when the batch fills the chip by itself and the panels fit the LDS.
int wg_panel_ld(const LaunchGroup &g) { return (g.max_r + 1) | 1; }
size_t wg_lds_bytes(int kind, const LaunchGroup &g)
{
    // (Cholesky, left-looking: the block column + the block's own rows of the factor, 16 x max_w)
    return ((size_t) WG_NB * 33 + (size_t) (kind == CS3_LU ? 2 : 1) * WG_NB * wg_panel_ld(g) +
            (kind == CS3_LU ? 0 : (size_t) 16 * (size_t) g.max_w)) * sizeof(double);
}
bool big_group_in_one_workgroup(int kind, long long batch, const LaunchGroup &g)
{
    static const long long min_batch = getenv("CS3_WG_MIN_BATCH") ? atoll(getenv("CS3_WG_MIN_BATCH")) : 48;    // (32 matrices: 1.01 ms in one workgroup each, 0.95 block step by block step; 64: 1.21 / 1.22; 128: 1.56 / 1.70)
    return g.cls == FC_BIG && batch >= min_batch && wg_lds_bytes(kind, g) <= 150 * 1024;
}

// A group of big fronts = one gather launch, then launches 0 .. nblk of the block step (nblk = closing: last update +
// last parked block).
static int big_group_blocks(const LaunchGroup &g) { return (g.max_w + BIG_NB - 1) / BIG_NB; }

BigSweepPlan big_sweep_plan(long long batch, const LaunchGroup &g, int nrhs)
{
    BigSweepPlan pl;
    pl.by = (unsigned) (batch * nrhs);
    pl.wide = batch * nrhs < 8;
    pl.multi = nrhs >= BIG_KT;
    pl.by_multi = (unsigned) (batch * ((nrhs + BIG_KT - 1) / BIG_KT));
    // latency-bound: two blocks per launch, four where that saves a launch
    pl.cw = pl.wide ? (g.max_w > BIG_CW ? BIG_CW4 : BIG_CW) : SOLVE_BW;
    // one front without rows of ancestors (the dense root): nothing for k_bwd_big_init to subtract
    pl.no_init = pl.cw == BIG_CW4 && g.count == 1 && g.max_r == g.max_w;
    pl.nchunk = (g.max_w + pl.cw - 1) / pl.cw;
    const int sr = (pl.cw == BIG_CW4) ? BIG_SR4 : 64;       // rows of a workgroup's slice
    pl.slices = std::max(1, (g.max_r + sr - 1) / sr);
    return pl;
}

// With few right-hand sides SK_SMALL and SK_WAVE fronts share the one-wave-per-front kernels:
// the two groups of a level are adjacent in the schedule and go out as one launch.
// A handful of small fronts beside the level's workgroup-per-front group (the top of the tree) join that group: a second
// launch for four fronts costs a dependent launch (sweeps, 11 us) or a fork and a join across hardware queues
// (factorisation, 13 us), the workgroup kernels take fronts of any order.
static void absorb_small_group(std::vector<LaunchGroup> &out, const LaunchGroup &g, int small_cls, int wg_cls)
{
    if (!out.empty() && out.back().level == g.level && out.back().cls == small_cls && g.cls == wg_cls &&
        out.back().count <= PROMOTE_MAX && out.back().first + out.back().count == g.first) {
        LaunchGroup &m = out.back();
        m.cls = wg_cls; m.count += g.count;
        m.max_r = std::max(m.max_r, g.max_r); m.max_w = std::max(m.max_w, g.max_w);
        m.n16 = 0;
    } else {
        out.push_back(g);
    }
}

static std::vector<LaunchGroup> sweep_groups(const ScheduleInput &in)
{
    if (in.nrhs >= RHS_LANES_MIN) return *in.sgroups;
    std::vector<LaunchGroup> merged, out;
    for (const LaunchGroup &g : *in.sgroups) {
        if (!merged.empty() && merged.back().level == g.level && merged.back().cls == SK_SMALL && g.cls == SK_WAVE &&
            merged.back().first + merged.back().count == g.first) {
            LaunchGroup &m = merged.back();
            m.cls = SK_WAVE; m.count += g.count;
            m.max_r = std::max(m.max_r, g.max_r); m.max_w = std::max(m.max_w, g.max_w);
        } else {
            merged.push_back(g);
        }
    }
    if (in.batch != 1) return merged;       // (a batch fills the chip with waves: one per front stays cheaper)
    for (const LaunchGroup &g : merged) absorb_small_group(out, g, SK_WAVE, SK_BLOCK);
    return out;
}

// the same for the factorisation of a single matrix: few fronts of order <= 64 beside the level's LDS-image fronts
static std::vector<LaunchGroup> factor_groups(const ScheduleInput &in)
{
    if (in.batch != 1) return *in.fgroups;
    std::vector<LaunchGroup> out;
    for (const LaunchGroup &g : *in.fgroups) absorb_small_group(out, g, FC_R64, FC_LDS);
    return out;
}

// The groups of one level: forward, the end of the run that starts at g; backward, the start of the run that ends at g.
static size_t level_edge(const std::vector<LaunchGroup> &groups, size_t g, bool forward)
{
    const int level = groups[forward ? g : g - 1].level;
    if (forward) while (g < groups.size() && groups[g].level == level) ++g;
    else while (g > 0 && groups[g - 1].level == level) --g;
    return g;
}

// Rough cost of a launch group in dependent-launch units, to place the fork.
static int factor_group_cost(const LaunchGroup &g) { return (g.cls == FC_BIG) ? 4 * ((g.max_w + BIG_NB - 1) / BIG_NB + 2) : 2; }
static int sweep_group_cost(const LaunchGroup &g) { return (g.cls == SK_BIG) ? 2 + (g.max_w + BIG_CW - 1) / BIG_CW : 1; }

namespace {

struct Planner {
    const ScheduleInput &in;
    LaunchPlan plan;
    int events = 0;
    const LaunchGroup none{0, 0, 0, 0, 0, 0, 0};

    void launch(int kind, const LaunchGroup &g, int slot, int arg = -1) { plan.push_back(PlanStep{kind, slot, g, arg, -1}); }
    int record(int slot) { plan.push_back(PlanStep{STEP_RECORD, slot, none, -1, events}); return events++; }
    void wait(int slot, int event) { plan.push_back(PlanStep{STEP_WAIT, slot, none, -1, event}); }

    void factor_group(const LaunchGroup &g, int slot)
    {
        const bool chain = g.cls == FC_BIG && !big_group_in_one_workgroup(in.kind, in.batch, g);
        if (!chain && g.cls != FC_SCHUR) return launch(STEP_FRONT_GROUP, g, slot);
        launch(STEP_BIG_GATHER, g, slot);
        // a Schur handle's last front: assembled, taken out, never eliminated (schur.hip)
        if (g.cls == FC_SCHUR) return launch(STEP_SCHUR_TAKE, g, slot);
        for (int blk = 0; blk <= big_group_blocks(g); ++blk) launch(STEP_BIG_BLOCK, g, slot, blk);
    }

    void sweep_group(const LaunchGroup &g, bool forward, int slot)
    {
        // (with many right-hand sides a group of big fronts sweeps as GEMMs like every other group of fronts of order > 64)
        if (g.cls != SK_BIG || (gemm_sweeps_on() && in.nrhs >= RHS_LANES_MIN)) return launch(forward ? STEP_SWEEP_FWD : STEP_SWEEP_BWD, g, slot);
        const BigSweepPlan pl = big_sweep_plan(in.batch, g, in.nrhs);
        if (forward) launch(STEP_FWD_BIG_PRE, g, slot);
        else if (!pl.no_init) launch(STEP_BWD_BIG_PRE, g, slot);
        for (int c = 0; c < pl.nchunk; ++c) launch(forward ? STEP_FWD_BIG_CHUNK : STEP_BWD_BIG_CHUNK, g, slot, c);
    }

    // The launch groups [g0, g1) of one tree level: in line on slot 0, or (parallel) the first on slot 0 and the others
    // on side streams that fork from it and join it again.  add(group, slot) appends one group.
    template <class Add>
    void level(const std::vector<LaunchGroup> &groups, size_t g0, size_t g1, bool parallel, Add add)
    {
        const size_t ng = g1 - g0, nside = ForkJoin::NSIDE;
        if (ng <= 1 || !parallel) { for (size_t i = g0; i < g1; ++i) add(groups[i], 0); return; }
        const int fork = record(0);
        // the heaviest group (last: big fronts / block kernels sort last) stays on the main stream and is captured FIRST: the
        // runtime keeps a node's first captured dependent in the node's own hardware queue (fork_and_root_chain)
        add(groups[g1 - 1], 0);
        for (size_t i = 0; i + 1 < ng; ++i) {
            if (i < nside) wait(1 + (int) i, fork);          // (a side stream that is used again is behind the fork already)
            add(groups[g0 + i], 1 + (int) (i % nside));
        }
        for (size_t i = 0; i < std::min(ng - 1, nside); ++i) wait(0, record(1 + (int) i));
    }

    // the factor level that starts at g0; returns its end
    size_t factor_level(const std::vector<LaunchGroup> &groups, size_t g0)
    {
        const size_t g1 = level_edge(groups, g0, true);
        level(groups, g0, g1, true, [&](const LaunchGroup &g, int slot) { factor_group(g, slot); });
        return g1;
    }

    // forward sweep of levels lo .. hi
    void forward_sweep(const std::vector<LaunchGroup> &sgroups, int lo, int hi, int slot)
    {
        // (the bottom forest, when its factor launch carries the forward sweep, has nothing left to sweep)
        for (const LaunchGroup &g : sgroups)
            if (g.level >= lo && g.level <= hi && !(g.cls == SK_SUB && in.fwd_in_factor)) sweep_group(g, true, slot);
    }

    void by_level_on_aux(const std::vector<LaunchGroup> &fgroups, const std::vector<LaunchGroup> &sgroups);
    void fork_and_root_chain(const std::vector<LaunchGroup> &fgroups, const std::vector<LaunchGroup> &sgroups, int nlevels, bool overlap);
    int root_chain(const LaunchGroup &rootf, const LaunchGroup &roots, int ready, const std::vector<LaunchGroup> &sgroups);
};

// BATCHES: every level is a launch of 100 us or more, so a cross-queue edge (5-10 us) per level is cheap and the
// forward sweep follows the factorisation level by level on aux -- sweep level l as soon as level l is factorised --
// instead of waiting for the fork level (round 3; kernel trace of 512 matrices: the sweep of levels 1..9, 400 us of
// small launches, ran after the root with nothing beside it).  Sweep level l is CAPTURED after factor level l + 1, so
// that the factor chain stays the first captured dependent of its own nodes (fork_and_root_chain).
void Planner::by_level_on_aux(const std::vector<LaunchGroup> &fgroups, const std::vector<LaunchGroup> &sgroups)
{
    int pending = -1, pending_level = -1;
    auto flush = [&] {
        if (pending < 0) return;
        wait(SLOT_AUX, pending);
        forward_sweep(sgroups, pending_level, pending_level, SLOT_AUX);
    };
    for (size_t f0 = 0; f0 < fgroups.size(); ) {
        const int lvl = fgroups[f0].level;
        f0 = factor_level(fgroups, f0);
        flush();
        pending = record(0);
        pending_level = lvl;
    }
    flush();
    wait(0, record(SLOT_AUX));
}

// The last level, when it is one group of wide big fronts (the dense root): its forward sweep does not wait
// for the end of its factorisation either.  Column block b of the factor is final in F after block launch
// b + 1 (k_big_step), so chunk c of the sweep follows on aux as soon as its blocks are home, while the
// later blocks are still being factorised.  ONE release (every cross-stream edge costs the block chain about 10 us): the
// first k chunks go to aux after block launch k * cwb; the other chunks follow on slot 0 after the join.  Returns k.
int Planner::root_chain(const LaunchGroup &rootf, const LaunchGroup &roots, int ready, const std::vector<LaunchGroup> &sgroups)
{
    const BigSweepPlan pl = big_sweep_plan(in.batch, roots, in.nrhs);
    const int nblk = big_group_blocks(rootf), cwb = pl.cw / BIG_NB;
    // k the largest count that the remaining launches still cover (one launch of slack: the side queue starts a chunk
    // 10-15 us after its release)
    int k = 0;
    while (k < pl.nchunk && (k + 1) * cwb <= nblk && nblk - (k + 1) * cwb >= k + 2) ++k;
    launch(STEP_BIG_GATHER, rootf, 0);
    for (int blk = 0, home = -1; blk <= nblk; ++blk) {
        launch(STEP_BIG_BLOCK, rootf, 0, blk);
        if (blk == 0) {                    // after the chain's first block: the sweep of the lower levels + the root's gather
            if (ready >= 0) { wait(SLOT_AUX, ready); forward_sweep(sgroups, 0, roots.level - 1, SLOT_AUX); }
            launch(STEP_FWD_BIG_PRE, roots, SLOT_AUX);
        }
        if (home >= 0) {                   // after the block that follows the release point (k * cwb < nblk: there is one)
            wait(SLOT_AUX, home);
            for (int c = 0; c < k; ++c) launch(STEP_FWD_BIG_CHUNK, roots, SLOT_AUX, c);
            home = -1;
        }
        if (k > 0 && blk == k * cwb) home = record(0);       // blocks 0 .. blk - 1 are home
    }
    return k;
}

// The sweep of levels 0..K needs only the panels of those levels, so once level K is factorised it runs on aux beside the
// factorisation of levels K+1.. (the tail of the tree: few, large fronts, many dependent launches).
// K is the last level whose tail is still long enough to cover the sweep; one fork, one join -- a
// fork per level costs more than it hides (measured).  Same kernels, same operands: same bits.
//
// The side branch is CAPTURED after the next launch of the chain it forks from: the runtime keeps a node's FIRST
// captured dependent in the node's own hardware queue and moves the others to another queue, whose first dispatch
// then waits 40-60 us (measured: profiles/r02_timeline_fused_step.json) -- the late start must land on the sweep,
// which has slack, not on the factorisation.  (Tried and removed, DESIGN.md: the sweep captured first; the block chain
// waiting for the side branch before the release; hand-overs through memory words with a waiting kernel.)
void Planner::fork_and_root_chain(const std::vector<LaunchGroup> &fgroups, const std::vector<LaunchGroup> &sgroups, int nlevels, bool overlap)
{
    std::vector<long long> tail(nlevels + 1, 0), head(nlevels + 1, 0);   // factor cost of levels >= l; sweep cost of levels < l
    for (const LaunchGroup &g : fgroups) tail[g.level] += factor_group_cost(g);
    for (int l = nlevels - 1; l >= 0; --l) tail[l] += tail[l + 1];
    for (const LaunchGroup &g : sgroups) head[g.level + 1] += (g.cls == SK_SUB && in.fwd_in_factor) ? 0 : sweep_group_cost(g);
    for (int l = 0; l < nlevels; ++l) head[l + 1] += head[l];
    int fork_level = -1;
    for (int l = 0; overlap && l + 1 < nlevels; ++l)
        if (tail[l + 1] >= head[l + 1]) fork_level = l;

    const LaunchGroup *rootf = nullptr, *roots = nullptr;
    // (with many right-hand sides the root sweeps as GEMMs like every other group)
    if (in.nrhs < RHS_LANES_MIN && nlevels >= 2 && fork_level == nlevels - 2) {
        int nf = 0, ns = 0;
        for (const LaunchGroup &g : fgroups) if (g.level == nlevels - 1) { ++nf; rootf = &g; }
        for (const LaunchGroup &g : sgroups) if (g.level == nlevels - 1) { ++ns; roots = &g; }
        if (nf != 1 || ns != 1 || rootf->cls != FC_BIG || roots->cls != SK_BIG || rootf->count != roots->count)
            rootf = roots = nullptr;
    }
    int ready = -1, swept = -1;            // panels of levels 0..fork_level are final; their sweep is done
    int root_rest = 0;                     // first chunk of the root's sweep that is still to do after the join
    for (size_t f0 = 0; f0 < fgroups.size(); ) {
        const int lvl = fgroups[f0].level;
        if (rootf && lvl == nlevels - 1) {             // (the last level, one group)
            root_rest = root_chain(*rootf, *roots, ready, sgroups);
            swept = record(SLOT_AUX);
            break;
        }
        f0 = factor_level(fgroups, f0);
        if (!rootf && ready >= 0 && swept < 0) {       // the level above the fork has been captured: now the side branch
            wait(SLOT_AUX, ready);
            forward_sweep(sgroups, 0, fork_level, SLOT_AUX);
            swept = record(SLOT_AUX);
        }
        if (lvl == fork_level) ready = record(0);
    }
    if (swept >= 0) wait(0, swept);
    if (!rootf) return forward_sweep(sgroups, fork_level + 1, nlevels, 0);
    for (int c = root_rest; c < big_sweep_plan(in.batch, *roots, in.nrhs).nchunk; ++c) launch(STEP_FWD_BIG_CHUNK, *roots, 0, c);
}

}  // namespace

LaunchPlan plan_factor_levels(const ScheduleInput &in)
{
    Planner p{in};
    const std::vector<LaunchGroup> groups = factor_groups(in);
    for (size_t g0 = 0; g0 < groups.size(); ) g0 = p.factor_level(groups, g0);
    return p.plan;
}

LaunchPlan plan_solve_levels(const ScheduleInput &in, bool forward)
{
    Planner p{in};
    const std::vector<LaunchGroup> groups = sweep_groups(in);
    // one right-hand side: the per-level launches are short, fork/join costs more than it hides (measured), so they stay
    // in line.  Many right-hand sides: the lane = right-hand-side group and the GEMM group of a level take 10-40 us each
    // and are independent -- side by side they save 60 us of 1.73 ms at 1024 right-hand sides, 24 us of 0.83 at 128.
    // (re-measured with the fronts of order 33-64 on the GEMM sweeps: the fork now pays from 512 right-hand sides on only
    //  -- 128: 0.82 ms forked, 0.77 in line; 256: equal; 1024: equal to 0.5 %)
    const bool parallel = in.nrhs >= 512;
    auto add = [&](const LaunchGroup &g, int slot) { p.sweep_group(g, forward, slot); };
    if (forward)
        for (size_t g0 = 0, g1; g0 < groups.size(); g0 = g1) p.level(groups, g0, g1 = level_edge(groups, g0, true), parallel, add);
    else
        for (size_t g1 = groups.size(), g0; g1 > 0; g1 = g0) p.level(groups, g0 = level_edge(groups, g1, false), g1, parallel, add);
    return p.plan;
}

// Factorisation with the forward sweep partly hidden behind it.
LaunchPlan plan_factor_with_forward(const ScheduleInput &in)
{
    static const bool overlap = !env_is_1("CS3_NO_OVERLAP");
    if (in.forest && !in.forest_sweeps) {
        // a bottom forest under the factorisation, but sweeps on the level schedule of the whole tree (several right-hand
        // sides): the two number their levels differently, so nothing is overlapped.  (Two plans end to end: the sweep's
        // events count from 0 again and take the pool's first events a second time.)
        LaunchPlan plan = plan_factor_levels(in);
        const LaunchPlan sweep = plan_solve_levels(in, true);
        plan.insert(plan.end(), sweep.begin(), sweep.end());
        return plan;
    }
    Planner p{in};
    const std::vector<LaunchGroup> fgroups = factor_groups(in), sgroups = sweep_groups(in);
    const int nlevels = fgroups.empty() ? 0 : fgroups.back().level + 1;
    if (overlap && in.batch >= 16 && nlevels >= 2) p.by_level_on_aux(fgroups, sgroups);
    else p.fork_and_root_chain(fgroups, sgroups, nlevels, overlap);
    return p.plan;
}

}  // namespace cs3
