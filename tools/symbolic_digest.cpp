// Stand-alone digest of the symbolic analysis: runs cs3::analyze (and build_csc_factors) over a manifest of runs and
// prints, per run, one line per field of cs3::Symbolic -- name, length and a 64-bit FNV-1a over its bytes -- or the
// text of the exception.  Two builds of this file against two versions of symbolic.cpp that print the same bytes
// compute the same analysis.  Links with symbolic.cpp + ordering.cpp alone (no HIP, no api.cpp); tools/symbolic_digest.py
// writes the inputs, builds and runs it.
//
//   symbolic_digest MANIFEST                 digest every run of the manifest
//   symbolic_digest MANIFEST --time LABEL K  K analyses of run LABEL: prints t_order + t_symbolic of each (seconds)
//
// Manifest line:  LABEL PATTERN_FILE KIND ORDER BATCH FLAGS     FLAGS: '-' or a comma list of
//   q (pass the file's q), schur (pass the file's Schur set), nullai, nullidx (pass a null pointer instead).
// Pattern file, raw little-endian: int64 n, int32 Ap[n + 1], int32 Ai[Ap[n]], then optionally int64 nq, int32 q[nq],
//   int64 ns, int32 idx[ns].
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cs3_internal.hpp"

using cs3::i32;
using cs3::i64;

namespace {

uint64_t fnv1a(const void *data, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

struct Pattern {
    std::string file;
    i64 n = 0;
    std::vector<i32> Ap, Ai, q, idx;
};

template <class T>
void read_raw(std::ifstream &in, T *dst, size_t count, const std::string &file)
{
    in.read(reinterpret_cast<char *>(dst), (std::streamsize) (count * sizeof(T)));
    if ((size_t) in.gcount() != count * sizeof(T)) throw std::runtime_error("short read in " + file);
}

void load(const std::string &file, Pattern &P)
{
    if (P.file == file) return;
    P = Pattern();
    std::ifstream in(file, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + file);
    read_raw(in, &P.n, 1, file);
    P.Ap.resize((size_t) P.n + 1);
    read_raw(in, P.Ap.data(), P.Ap.size(), file);
    P.Ai.resize((size_t) P.Ap[(size_t) P.n]);
    read_raw(in, P.Ai.data(), P.Ai.size(), file);
    i64 count = 0;
    if (in.peek() != EOF) { read_raw(in, &count, 1, file); P.q.resize((size_t) count); read_raw(in, P.q.data(), P.q.size(), file); }
    if (in.peek() != EOF) { read_raw(in, &count, 1, file); P.idx.resize((size_t) count); read_raw(in, P.idx.data(), P.idx.size(), file); }
    P.file = file;
}

struct Digest {
    i64 fields = 0;
    template <class T> void scalar(const char *name, const T &v) { line(name, 1, fnv1a(&v, sizeof(T))); }
    template <class T> void vec(const char *name, const std::vector<T> &v) { line(name, v.size(), fnv1a(v.data(), v.size() * sizeof(T))); }
    // one member of every element of a vector of structs (no padding enters the hash)
    template <class E, class M> void member(const char *name, const std::vector<E> &v, M E::*m)
    {
        uint64_t h = fnv1a(nullptr, 0);
        for (const E &e : v) h = fnv1a(&(e.*m), sizeof(M), h);
        line(name, v.size(), h);
    }
    void line(const char *name, size_t len, uint64_t h) { std::printf("  %s %zu %016" PRIx64 "\n", name, len, h); ++fields; }
};

void groups(Digest &D, const std::string &name, const std::vector<cs3::LaunchGroup> &g)
{
    using G = cs3::LaunchGroup;
    D.member((name + ".level").c_str(), g, &G::level); D.member((name + ".cls").c_str(), g, &G::cls);
    D.member((name + ".first").c_str(), g, &G::first); D.member((name + ".count").c_str(), g, &G::count);
    D.member((name + ".max_r").c_str(), g, &G::max_r); D.member((name + ".max_w").c_str(), g, &G::max_w);
    D.member((name + ".n16").c_str(), g, &G::n16);
}

// every field of Symbolic except t_order / t_symbolic
void digest(Digest &D, const cs3::Symbolic &S)
{
#define SC(f) D.scalar(#f, S.f)
#define VE(f) D.vec(#f, S.f)
    SC(n); SC(nnzA); SC(batch); SC(kind);
    VE(q_amd); VE(parent_amd); VE(post_amd); VE(count_amd); VE(q); VE(pinv); VE(parent); VE(colcount);
    SC(nsuper); VE(sn_ptr); VE(col2sn); VE(sn_parent); VE(sn_level); VE(sn_class);
    VE(st_ptr); VE(st_idx); VE(child_ptr); VE(child_idx);
    VE(lpan_off); VE(upan_off); VE(cb_off); VE(cb_ld); VE(u_sk); VE(u_sj); VE(cv_off); VE(rel_ptr); VE(rel_idx);
    SC(vals_size); SC(cb_size); SC(cv_size); SC(pool_size);
    SC(il_len); VE(ila_ptr); VE(ila_pairs); SC(big_begin);
    VE(fa_ptr); VE(ch_ptr); VE(fa_tgt); VE(fa_src); VE(ch_tab);
    VE(fasm_ptr); VE(fasm_src); VE(fasm_tgt); VE(flong_src);
    VE(ssched); VE(rl_ptr); VE(rl_pairs); VE(sl_ptr); VE(sl_rounds); VE(sl_src); VE(bv_off); SC(bv_size);
    VE(gv_off); VE(dinv_off); SC(gv_size); SC(dinv_size); VE(inv_tasks);
    groups(D, "sgroups", S.sgroups);
    VE(sn_in_forest); VE(sn_tlevel);
    {
        const cs3::SubForest &T = S.sub_forest;
        D.scalar("sub_forest.ntasks", T.ntasks); D.scalar("sub_forest.max_fronts", T.max_fronts);
        D.scalar("sub_forest.max_levels", T.max_levels); D.scalar("sub_forest.max_rel", T.max_rel);
        D.scalar("sub_forest.max_child", T.max_child); D.scalar("sub_forest.max_arena", T.max_arena);
        D.scalar("sub_forest.max_varena", T.max_varena); D.scalar("sub_forest.max_r", T.max_r);
    }
    {
        using K = cs3::SubTask;
        const std::vector<K> &v = S.sub_tasks;
        D.member("sub_tasks.front0", v, &K::front0); D.member("sub_tasks.nfronts", v, &K::nfronts);
        D.member("sub_tasks.lvl0", v, &K::lvl0); D.member("sub_tasks.nlevels", v, &K::nlevels);
        D.member("sub_tasks.rel0", v, &K::rel0); D.member("sub_tasks.nrel", v, &K::nrel);
        D.member("sub_tasks.child0", v, &K::child0); D.member("sub_tasks.nchild", v, &K::nchild);
    }
    {
        using F = cs3::SubFront;
        const std::vector<F> &v = S.sub_fronts;
        D.member("sub_fronts.lpan", v, &F::lpan); D.member("sub_fronts.upan", v, &F::upan); D.member("sub_fronts.cb", v, &F::cb);
        D.member("sub_fronts.cv", v, &F::cv); D.member("sub_fronts.c0", v, &F::c0); D.member("sub_fronts.r", v, &F::r);
        D.member("sub_fronts.w", v, &F::w); D.member("sub_fronts.a_begin", v, &F::a_begin); D.member("sub_fronts.a_count", v, &F::a_count);
        D.member("sub_fronts.child_begin", v, &F::child_begin); D.member("sub_fronts.child_count", v, &F::child_count);
        D.member("sub_fronts.rel", v, &F::rel); D.member("sub_fronts.st", v, &F::st); D.member("sub_fronts.u_sj", v, &F::u_sj);
        D.member("sub_fronts.parent", v, &F::parent); D.member("sub_fronts.arena", v, &F::arena);
    }
    VE(sub_sn); VE(sub_lvl); VE(sub_rel); VE(sub_child); VE(sub_st); VE(sub_a_tgt); VE(sub_a_src);
    VE(ssched1); groups(D, "sgroups1", S.sgroups1);
    SC(nlevels); VE(sched); groups(D, "groups", S.groups);
    VE(fsn_ptr); VE(fst_idx); VE(fst_ptr); SC(nnz_l); SC(nnz_u);
    VE(Lp); VE(Li); VE(Up); VE(Ui); VE(Lmap); VE(Umap);
    SC(max_front); SC(max_width); SC(flops);
    VE(schur_idx); SC(schur_sn);
#undef SC
#undef VE
}

// which branches of the analysis this run went through
void coverage(const cs3::Symbolic &S)
{
    i64 fc[cs3::FC_COUNT] = {0}, sk[6] = {0}, riders = 0;
    for (i32 s = 0; s < S.nsuper; ++s) {
        ++fc[S.sn_class[(size_t) s]];
        if (S.sn_class[(size_t) s] == cs3::FC_BIG && S.st_ptr[(size_t) s + 1] - S.st_ptr[(size_t) s] <= 136) ++riders;
    }
    for (const cs3::LaunchGroup &g : S.sgroups) sk[g.cls] += g.count;
    for (const cs3::LaunchGroup &g : S.sgroups1) if (g.cls == cs3::SK_SUB) sk[g.cls] += g.count;
    std::printf("coverage fc");
    for (i64 c : fc) std::printf(" %" PRId64, c);
    std::printf(" sk");
    for (i64 c : sk) std::printf(" %" PRId64, c);
    std::printf(" riders %" PRId64 " flong_src %d ila_pairs %d rl_pairs %d sl_src %d inv_tasks %d sub_fronts %d schur_idx %d\n", riders,
                !S.flong_src.empty(), !S.ila_pairs.empty(), !S.rl_pairs.empty(), !S.sl_src.empty(), !S.inv_tasks.empty(),
                !S.sub_fronts.empty(), !S.schur_idx.empty());
}

struct Run {
    std::string label, file, flags;
    int kind = 0, order = 0;
    i64 batch = 1;
    bool has(const char *flag) const { return ("," + flags + ",").find(std::string(",") + flag + ",") != std::string::npos; }
};

void analyze(const Run &R, const Pattern &P, cs3::Symbolic &S)
{
    static const i32 none = 0;                 // (an empty vector's data() may be null: that is the nullai / nullidx case only)
    const i32 *Ai = R.has("nullai") ? nullptr : (P.Ai.empty() ? &none : P.Ai.data());
    const i32 *q = R.has("q") ? (P.q.empty() ? &none : P.q.data()) : nullptr;
    const cs3::SchurSet set{R.has("nullidx") ? nullptr : (P.idx.empty() ? &none : P.idx.data()), (i64) P.idx.size()};
    cs3::analyze(R.kind, R.order, P.n, P.Ap.data(), Ai, q, S, R.batch, R.has("schur") ? &set : nullptr);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2 && !(argc == 5 && !std::strcmp(argv[2], "--time"))) {
        std::fprintf(stderr, "usage: %s MANIFEST [--time LABEL REPS]\n", argv[0]);
        return 2;
    }
    std::ifstream manifest(argv[1]);
    if (!manifest) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::string only = argc == 5 ? argv[3] : "";
    const int reps = argc == 5 ? std::atoi(argv[4]) : 0;
    Pattern P;
    i64 runs = 0, fields = 0;
    std::string text;
    while (std::getline(manifest, text)) {
        if (text.empty() || text[0] == '#') continue;
        std::istringstream in(text);
        Run R;
        if (!(in >> R.label >> R.file >> R.kind >> R.order >> R.batch >> R.flags)) { std::fprintf(stderr, "bad manifest line: %s\n", text.c_str()); return 2; }
        if (!only.empty() && R.label != only) continue;
        load(R.file, P);
        if (reps > 0) {
            for (int k = 0; k < reps; ++k) {
                cs3::Symbolic S;
                analyze(R, P, S);
                std::printf("time %s %.6f\n", R.label.c_str(), S.t_order + S.t_symbolic);
            }
            continue;
        }
        std::printf("run %s kind %d order %d batch %" PRId64 " flags %s\n", R.label.c_str(), R.kind, R.order, R.batch, R.flags.c_str());
        ++runs;
        try {
            cs3::Symbolic S;
            analyze(R, P, S);
            cs3::build_csc_factors(S);
            Digest D;
            digest(D, S);
            fields += D.fields;
            coverage(S);
        } catch (const std::exception &e) {
            std::printf("  error %zu %016" PRIx64 " %s\n", std::strlen(e.what()), fnv1a(e.what(), std::strlen(e.what())), e.what());
            ++fields;
        }
    }
    if (reps == 0) std::printf("total runs %" PRId64 " fields %" PRId64 "\n", runs, fields);
    return 0;
}
