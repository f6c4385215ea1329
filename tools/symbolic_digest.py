#!/usr/bin/env python3
"""Digest of the symbolic analysis over a wide run set, to compare two versions of csrc/symbolic.cpp bit for bit.

Writes the patterns and the manifest from the project's own generators, builds tools/symbolic_digest.cpp against a source
directory (symbolic.cpp + ordering.cpp, plain g++, no HIP) and runs it.  Every field of cs3::Symbolic of every run is
hashed; refusals are digested by their text.

  tools/symbolic_digest.py run --src csparse3_amd/csrc --work /tmp/head
  tools/symbolic_digest.py run --src csparse3_amd/csrc --work /tmp/san --cxxflags="-O1 -g -fsanitize=address,undefined"
  tools/symbolic_digest.py compare --parent /tmp/parent_tree/csparse3_amd/csrc --head csparse3_amd/csrc \
        --work /tmp/cmp --json profiles/analyze_split.json

`compare` runs the set on both source directories with the same compiler and flags, requires identical output (the
CS3_DUMP_GROUPS dump of one run included), checks the coverage condition and times the analysis (alternating parent and
head).  The parent's tree comes from `git worktree add` or `git archive` of the parent commit.

Each environment variant runs in a process of its own: CS3_SUBTREE and the CS3_DUMP_GROUPS timing flag are read once per
process.
"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from csparse3_amd import synth  # noqa: E402
import forest_cases  # noqa: E402
import rhs_cases  # noqa: E402
import schur_cases  # noqa: E402
import sweep_cases  # noqa: E402
import wide_chunk_cases  # noqa: E402

LU, CHOL = 0, 1
NATURAL, AMD, GIVEN = 0, 1, 2
KINDS = (("lu", LU), ("chol", CHOL))
ORDERS = (("amd", AMD), ("nat", NATURAL), ("given", GIVEN))
BATCHES = (1, 2, 8, 15, 16, 64, 127, 128, 130, 255, 256, 512)      # both sides of every batch threshold of symbolic.cpp
BATCHES_50K = (1, 128, 512)
ENVS = (("none", {}), ("subtree0", {"CS3_SUBTREE": "0"}), ("height64", {"CS3_SUB_HEIGHT": "64"}),
        ("relax02_height2", {"CS3_RELAX_Z": "0.2", "CS3_SUB_HEIGHT": "2"}), ("ilmin100000", {"CS3_IL_MIN_BATCH": "100000"}),
        ("ilmin1", {"CS3_IL_MIN_BATCH": "1"}))
# the environment variants run against these: patterns with a forest at batch 1, and large batches
ENV_PATTERNS = ("grid5000", "grid50000", "spd5000", "forest_fans", "forest_isl", "forest_chain6", "rhs_hub", "schur_grid2k")
ENV_BATCHES = (1, 128, 512)
TIMED = (("grid50000.lu.amd.b1", "grid50000_lu_b1"), ("spd5000.chol.amd.b512", "spd5000_chol_b512"))
DUMPED = "grid5000.lu.amd.b1"
FRONT_CLASSES = ("FC_R16", "FC_R32", "FC_R64", "FC_LDS", "FC_BIG", "FC_IL", "FC_SUB", "FC_SCHUR")
SOLVE_KINDS = ("SK_SMALL", "SK_WAVE", "SK_BLOCK", "SK_BIG", "SK_IL", "SK_SUB")
CONTAINERS = ("flong_src", "ila_pairs", "rl_pairs", "sl_src", "inv_tasks", "sub_fronts", "schur_idx")


def given_order(cols, seed=2024):
    """A fixed permutation of `cols`: shuffled inside windows of 16, then reversed (a uniformly random order of a
    50 000-column grid fills in until the analysis alone takes gigabytes)."""
    rng = np.random.default_rng(seed)
    cols = np.array(cols, dtype=np.int32)
    for k in range(0, len(cols), 16):
        rng.shuffle(cols[k:k + 16])
    return cols[::-1].copy()


def star(leaves=80):
    """A hub column coupled to `leaves` columns of degree one: in the natural order the hub's front gets one addition per
    leaf on its first row (a run of more than 64 equal targets in the forward-sweep gather list)."""
    n = leaves + 1
    rows = np.concatenate([np.arange(n), np.full(leaves, leaves), np.arange(leaves)])
    cols = np.concatenate([np.arange(n), np.arange(leaves), np.full(leaves, leaves)])
    return synth._coo_to_sorted_csc(n, rows, cols, np.ones(len(rows)))[1:4]


def arrow(n=33000):
    """Column 0 coupled to every other: in the natural order the factor is dense, one front of order n whose r x r buffer
    passes 2^30 entries -- refused in step 7 before anything of that size is allocated."""
    rows = np.concatenate([np.arange(n), np.arange(1, n), np.zeros(n - 1, dtype=np.int64)])
    cols = np.concatenate([np.arange(n), np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])
    return synth._coo_to_sorted_csc(n, rows, cols, np.ones(len(rows)))[1:4]


def patterns():
    """-> [(name, n, Ap, Ai, Schur set or None)]; all of them structurally symmetric, so every one runs both kinds."""
    out = [("n0", 0, np.zeros(1, np.int32), np.zeros(0, np.int32), None),
           ("n1", 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), None),
           ("toy10",) + tuple(synth.toy10()[1:4]) + (None,),
           ("jacobian",) + tuple(synth.jacobian_like()[1:4]) + (None,)]
    for n in (2000, 5000, 20000, 50000):
        out.append(("grid%d" % n,) + tuple(synth.grid_jacobian(n=n, seed=n)[1:4]) + (None,))
    ei, ej = synth.spd_grid_pattern(5000)
    out.append(("spd5000",) + tuple(synth.spd_grid_matrix(5000, ei, ej, seed=1)[1:4]) + (None,))
    lower = synth.spd_grid_matrix(5000, ei, ej, seed=1, lower_only=True)[1:4]
    out.append(("spd5000_lower",) + tuple(lower) + (None,))
    diag = np.arange(5000)
    upper = synth._coo_to_sorted_csc(5000, np.concatenate([ei, diag]), np.concatenate([ej, diag]), np.ones(len(ei) + 5000))[1:4]
    out.append(("spd5000_upper",) + tuple(upper) + (None,))
    out.append(("dense700",) + tuple(synth.dense_block_matrix(700, 300)[1:4]) + (None,))
    for name in forest_cases.CASES:
        M = forest_cases.case_matrix(name)
        out.append(("forest_" + name, M.n, M.Ap, M.Ai, None))
    for name in rhs_cases.TREES:
        out.append(("rhs_" + name,) + tuple(rhs_cases.case_matrix(name)[1:4]) + (None,))
    for name in sweep_cases.CASES:
        out.append(("sweep_" + name,) + tuple(sweep_cases.case_matrix(name)[1:4]) + (None,))
    for name in wide_chunk_cases.CASES:
        out.append(("wide_" + name,) + tuple(wide_chunk_cases.case_matrix(name)[1:4]) + (None,))
    out.append(("star80",) + tuple(star()) + (None,))
    out.append(("schur_toy10",) + tuple(schur_cases.matrix("toy10")[1:4]) + (schur_cases.schur_set("toy10", 3),))
    out.append(("schur_grid2k",) + tuple(schur_cases.matrix("grid2k")[1:4]) + (schur_cases.schur_set("grid2k", 33),))
    n, Ap, Ai, _, idx = schur_cases.saddle_point()[:5]
    out.append(("schur_saddle", n, Ap, Ai, idx))
    n, Ap, Ai, _, idx = schur_cases.pendant_zero()[:5]
    out.append(("schur_pendant", n, Ap, Ai, idx))
    return out


def write_pattern(path, n, Ap, Ai, q=None, idx=None):
    with open(path, "wb") as f:
        f.write(np.int64(n).tobytes())
        f.write(np.ascontiguousarray(Ap, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(Ai, dtype=np.int32).tobytes())
        if q is not None or idx is not None:
            q = np.zeros(0, np.int32) if q is None else np.ascontiguousarray(q, dtype=np.int32)
            f.write(np.int64(len(q)).tobytes() + q.tobytes())
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            f.write(np.int64(len(idx)).tobytes() + idx.tobytes())


def refusals(work):
    """-> manifest lines of the runs that analyze() refuses, in the order in which it checks."""
    n, Ap, Ai = synth.toy10()[1:4]
    Ap, Ai = np.array(Ap, np.int32), np.array(Ai, np.int32)
    nat = np.arange(n, dtype=np.int32)
    lines = []

    def case(label, Ap=Ap, Ai=Ai, q=nat, idx=None, kind=LU, order=AMD, flags="-", n=n):
        path = os.path.join(work, "refuse_%s.bin" % label)
        write_pattern(path, n, Ap, Ai, q, idx)
        lines.append("refuse.%s %s %d %d 1 %s" % (label, path, kind, order, flags))

    case("null_ai", flags="nullai")
    case("kind", kind=7)
    bad = Ap.copy(); bad[0] = 1
    case("ap0", Ap=bad)
    bad = Ap.copy(); bad[3] = bad[2] - 1
    case("ap_monotone", Ap=bad)
    bad = Ai.copy(); bad[5] = n
    case("row_range", Ai=bad)
    bad = Ai.copy(); bad[5] = -1
    case("row_negative", Ai=bad)
    bad = Ai.copy(); bad[Ap[4] + 1] = bad[Ap[4]]
    case("duplicate", Ai=bad)
    case("order", order=9)
    case("given_without_q", order=GIVEN)
    bad = nat.copy(); bad[3] = bad[2]
    case("q_repeated", q=bad, order=GIVEN, flags="q")
    bad = nat.copy(); bad[3] = n
    case("q_range", q=bad, order=GIVEN, flags="q")
    # Schur sets
    idx = np.array([7, 2, 5], np.int32)
    inner = np.array([v for v in range(n) if v not in (7, 2, 5)], np.int32)
    case("schur_null_idx", idx=idx, flags="schur,nullidx")
    case("schur_ns0", idx=np.zeros(0, np.int32), flags="schur")
    case("schur_ns_n", idx=nat, flags="schur")
    case("schur_idx_range", idx=np.array([7, n, 5], np.int32), flags="schur")
    case("schur_idx_negative", idx=np.array([7, -1, 5], np.int32), flags="schur")
    case("schur_idx_repeated", idx=np.array([7, 2, 7], np.int32), flags="schur")
    case("schur_order", idx=idx, order=9, flags="schur")
    case("schur_given_without_q", idx=idx, order=GIVEN, flags="schur")
    bad = inner.copy(); bad[1] = 7
    case("schur_q_border", q=bad, idx=idx, order=GIVEN, flags="schur,q")
    bad = inner.copy(); bad[1] = bad[0]
    case("schur_q_repeated", q=bad, idx=idx, order=GIVEN, flags="schur,q")
    # an earlier check wins over a later one
    bad = Ap.copy(); bad[0] = 1
    case("kind_before_ap0", Ap=bad, kind=7)
    case("schur_before_order", idx=np.array([7, 2, 7], np.int32), order=9, flags="schur")
    # a factor pool beyond 2^30 entries
    an, aAp, aAi = arrow()
    case("pool", Ap=aAp, Ai=aAi, q=None, order=NATURAL, n=an)
    return lines


def write_inputs(work):
    """-> {variant: [manifest lines]}"""
    os.makedirs(work, exist_ok=True)
    full, env = [], []
    for name, n, Ap, Ai, idx in patterns():
        interior = np.arange(n) if idx is None else np.setdiff1d(np.arange(n), idx)
        path = os.path.join(work, name + ".bin")
        write_pattern(path, n, Ap, Ai, given_order(interior), idx)
        for kname, kind in KINDS:
            for oname, order in ORDERS:
                flags = ",".join(f for f, on in (("q", order == GIVEN), ("schur", idx is not None)) if on) or "-"
                for batch in (BATCHES_50K if name == "grid50000" else BATCHES):
                    line = "%s.%s.%s.b%d %s %d %d %d %s" % (name, kname, oname, batch, path, kind, order, batch, flags)
                    full.append(line)
                    if name in ENV_PATTERNS and batch in ENV_BATCHES and order != GIVEN:
                        env.append(line)
    return {"none": full + refusals(work), **{v: env for v, _ in ENVS[1:]}}


def build(src, work, cxxflags):
    exe = os.path.join(work, "symbolic_digest")
    cmd = ["g++"] + cxxflags.split() + ["-std=c++17", "-I", src, os.path.join(ROOT, "tools", "symbolic_digest.cpp"),
                                        os.path.join(src, "symbolic.cpp"), os.path.join(src, "ordering.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _shard(exe, manifest, env):
    r = subprocess.run([exe, manifest], env={**os.environ, **env}, stdout=subprocess.PIPE, check=True)
    return r.stdout.decode()


def run_set(exe, work, manifests, jobs):
    """-> the whole output as one string: the variants in order, each cut into `jobs` processes."""
    tasks = []
    for variant, env in ENVS:
        lines = manifests[variant]
        for k in range(jobs):
            path = os.path.join(work, "manifest_%s_%d.txt" % (variant, k))
            with open(path, "w") as f:
                f.write("\n".join(lines[k::jobs]) + "\n")
            tasks.append((variant, path, env))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        outs = list(pool.map(lambda t: _shard(exe, t[1], t[2]), tasks))
    return "".join("variant %s shard %s\n%s" % (t[0], os.path.basename(t[1]), o) for t, o in zip(tasks, outs))


def group_dump(exe, work, manifests):
    """stderr of one run under CS3_DUMP_GROUPS, the step times blanked (their labels stay)."""
    path = os.path.join(work, "manifest_dump.txt")
    with open(path, "w") as f:
        f.write([ln for ln in manifests["none"] if ln.startswith(DUMPED + " ")][0] + "\n")
    r = subprocess.run([exe, path], env={**os.environ, "CS3_DUMP_GROUPS": "1"}, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, check=True)
    return re.sub(r"(?m)^(analysis .*?)\s+[0-9.]+ ms$", r"\1 <t> ms", r.stderr.decode())


def totals(text):
    runs = fields = refused = 0
    fc, sk, riders = [0] * len(FRONT_CLASSES), [0] * len(SOLVE_KINDS), 0
    has = dict.fromkeys(CONTAINERS, 0)
    for ln in text.splitlines():
        if ln.startswith("total runs"):
            w = ln.split(); runs += int(w[2]); fields += int(w[4])
        elif ln.startswith("  error"):
            refused += 1
        elif ln.startswith("coverage"):
            w = ln.split()
            a, b = w.index("fc"), w.index("sk")
            fc = [x + int(y) for x, y in zip(fc, w[a + 1:b])]
            sk = [x + int(y) for x, y in zip(sk, w[b + 1:w.index("riders")])]
            riders += int(w[w.index("riders") + 1])
            for c in CONTAINERS:
                has[c] += int(w[w.index(c) + 1])
    return {"runs": runs, "fields_compared": fields, "refusals": refused, "fronts_per_class": dict(zip(FRONT_CLASSES, fc)),
            "fronts_per_solve_kind": dict(zip(SOLVE_KINDS, sk)), "rider_fronts": riders, "runs_with_nonempty": has}


def check_coverage(T):
    """Every class and kind the analysis can give occurs, riders occur, every listed container is non-empty somewhere.
    (FC_R16 is a name in the enum only: front_class() never returns it.)"""
    missing = [c for c, k in T["fronts_per_class"].items() if k == 0 and c != "FC_R16"]
    missing += [c for c, k in T["fronts_per_solve_kind"].items() if k == 0]
    missing += [c for c, k in T["runs_with_nonempty"].items() if k == 0]
    if T["rider_fronts"] == 0:
        missing.append("riders")
    if missing:
        raise SystemExit("coverage condition fails: nothing reaches " + ", ".join(missing))


def digest_of(src, work, cxxflags, jobs, manifests=None):
    os.makedirs(work, exist_ok=True)
    manifests = manifests or write_inputs(work)
    exe = build(src, work, cxxflags)
    text = run_set(exe, work, manifests, jobs) + "group dump of %s\n%s" % (DUMPED, group_dump(exe, work, manifests))
    with open(os.path.join(work, "digest.txt"), "w") as f:
        f.write(text)
    return exe, text, manifests


def time_pair(exes, work, manifests, reps):
    """Alternates the executables, one analysis per process.  -> {run: {which: [seconds]}}"""
    out = {}
    for label, key in TIMED:
        path = os.path.join(work, "manifest_time_%s.txt" % key)
        with open(path, "w") as f:
            f.write([ln for ln in manifests["none"] if ln.startswith(label + " ")][0] + "\n")
        t = {which: [] for which in exes}
        for _ in range(reps):
            for which, exe in exes.items():
                r = subprocess.run([exe, path, "--time", label, "1"], stdout=subprocess.PIPE, check=True)
                t[which].append(float(r.stdout.split()[2]))
        out[key] = t
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("run", "compare"):
        p = sub.add_parser(name)
        p.add_argument("--work", required=True, help="directory for the patterns, manifests, executables and outputs")
        p.add_argument("--cxxflags", default="-O3")
        p.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
        if name == "run":
            p.add_argument("--src", required=True, help="directory that holds symbolic.cpp, ordering.cpp, cs3_internal.hpp")
        else:
            p.add_argument("--parent", required=True, help="the parent commit's csrc directory")
            p.add_argument("--head", required=True, help="the new csrc directory")
            p.add_argument("--reps", type=int, default=15)
            p.add_argument("--json", help="write the record here (profiles/analyze_split.json)")
    a = ap.parse_args()
    if a.cmd == "run":
        _, text, _ = digest_of(a.src, a.work, a.cxxflags, a.jobs)
        T = totals(text)
        print(json.dumps(T, indent=1))
        print("sha256", hashlib.sha256(text.encode()).hexdigest())
        check_coverage(T)
        return
    pexe, ptext, manifests = digest_of(a.parent, os.path.join(a.work, "parent"), a.cxxflags, a.jobs)
    T = totals(ptext)
    check_coverage(T)                                   # on the parent, before anything is compared
    hexe, htext, _ = digest_of(a.head, os.path.join(a.work, "head"), a.cxxflags, a.jobs, manifests)
    rec = {"what": "cs3::analyze + build_csc_factors, parent commit against this one, tools/symbolic_digest.py compare",
           "cxxflags": a.cxxflags, **T, "sha256_parent": hashlib.sha256(ptext.encode()).hexdigest(),
           "sha256_head": hashlib.sha256(htext.encode()).hexdigest()}
    rec["identical"] = ptext == htext
    if a.reps > 0:
        rec["timing"] = {"what": "t_order + t_symbolic in ms, one analysis per process, parent and head alternating", "reps": a.reps}
        for key, t in time_pair({"parent": pexe, "head": hexe}, a.work, manifests, a.reps).items():
            q = statistics.quantiles(t["parent"], n=4)
            rec["timing"][key] = {"parent_median_ms": round(1e3 * statistics.median(t["parent"]), 3),
                                  "head_median_ms": round(1e3 * statistics.median(t["head"]), 3),
                                  "parent_iqr_ms": round(1e3 * (q[2] - q[0]), 3)}
            rec["timing"][key]["head_within_parent_iqr"] = (rec["timing"][key]["head_median_ms"] - rec["timing"][key]["parent_median_ms"]
                                                            <= rec["timing"][key]["parent_iqr_ms"])
    print(json.dumps(rec, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    if not rec["identical"]:
        raise SystemExit("the outputs differ: diff %s/parent/digest.txt %s/head/digest.txt" % (a.work, a.work))


if __name__ == "__main__":
    main()
