#!/usr/bin/env python3
"""Union plans: a contingency family of SPD 5k x 5k matrices (the config-5 grid, every member without a few random chord
edges and with values of its own) on ONE batched handle over the union pattern (csparse3_amd.streams.UnionBatch) --
against the same members on a handle each (DistinctBatch), against a plain batched handle on the base pattern with every
member complete (the floor: a union with nothing missing), and the embedding launch alone against a device-to-device copy
of the same output.  Every leg in this process, event-timed, median of --reps.  Writes profiles/union_bench.json.
    python tools/bench_union.py [--nmat 64 512] [--distinct-upto 64] [--reps 20]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth
from csparse3_amd.streams import DistinctBatch, UnionBatch

ap = argparse.ArgumentParser()
ap.add_argument("--nmat", type=int, nargs="+", default=[64, 512])
ap.add_argument("--distinct-upto", type=int, default=64, help="largest family that also runs on one handle per member")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--max-drop", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "union_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
n5 = 5000
ei, ej = synth.spd_grid_pattern(n5)
chords = synth.chord_edges(n5, ei, ej)


def median_ms(fn, before=None):
    """Median over args.reps of the device time of fn(), between two events on the current stream."""
    for _ in range(3):
        if before: before()
        fn()
    ts = []
    for _ in range(args.reps):
        if before: before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


out = {"n": n5, "reps": args.reps, "base_edges": int(len(ei)), "chord_edges": int(len(chords)), "max_drop": args.max_drop,
       "entries_per_lane": int(hip.union_limits().entries_per_lane)}
for nmat in args.nmat:
    rng = np.random.default_rng(nmat)
    mats, full = [], []
    for c in range(nmat):
        keep = np.ones(len(ei), dtype=bool)
        keep[rng.choice(chords, size=int(rng.integers(1, args.max_drop + 1)), replace=False)] = False
        mats.append(synth.spd_grid_matrix(n5, ei[keep], ej[keep], seed=5000 + c))
        full.append(synth.spd_grid_matrix(n5, ei, ej, seed=5000 + c))
    rhs0 = torch.from_numpy(np.random.default_rng(1).standard_normal((nmat, n5))).to(dev)
    x = torch.empty_like(rhs0)
    refill = lambda: x.copy_(rhs0)                                  # noqa: E731
    cat = torch.from_numpy(np.concatenate([mm[4] for mm in mats])).to(dev)
    key = lambda s: "%s_%d" % (s, nmat)                             # noqa: E731

    with UnionBatch([mm[:4] for mm in mats], kind=hip.CS3_CHOLESKY) as U:
        inf, hinf = U.plan.info, U.factorization.info
        out[key("nnz_union")], out[key("nnz_total")] = int(inf.nnz_union), int(inf.nnz_total)
        out[key("padded")], out[key("distinct_patterns")] = int(inf.padded), int(inf.distinct_patterns)
        out[key("plan_s")] = U.plan_s
        out[key("handle_analysis_s")] = float(hinf.t_order_s + hinf.t_symbolic_s)
        out[key("union_ms")] = median_ms(lambda: U.factor_solve(cat, x), refill)
        U.status()
        x_union = x.clone()
        out[key("embed_us")] = 1e3 * median_ms(lambda: U.embed(cat))                    # the launch alone
        src = U.union_values.clone()
        out[key("copy_us")] = 1e3 * median_ms(lambda: U.union_values.copy_(src))       # hipMemcpyAsync, device to device
        out[key("embed_bytes")] = int(inf.nmat * inf.nnz_union * 12 + 8 * (inf.nmat * inf.nnz_union - inf.padded))
        out[key("copy_bytes")] = int(inf.nmat * inf.nnz_union * 16)

    if nmat <= args.distinct_upto:
        vals = [torch.from_numpy(mm[4]).to(dev) for mm in mats]
        with DistinctBatch([mm[:4] for mm in mats], kind=hip.CS3_CHOLESKY) as D:
            out[key("distinct_analysis_s")] = D.analysis_s
            rows = list(x)                                           # views of x: member i's right-hand side
            out[key("distinct_ms")] = median_ms(lambda: D.factor_solve(vals, rows), refill)
            D.status()
            out[key("union_vs_distinct_max_rel_diff")] = float(((x - x_union).abs().amax(dim=1) / x_union.abs().amax(dim=1)).max())
        out[key("distinct_over_union")] = out[key("distinct_ms")] / out[key("union_ms")]

    m, n, Ap, Ai, _ = full[0]
    with hip.Factorization(n5, n5, Ap, Ai, kind=hip.CS3_CHOLESKY, batch=nmat) as F:
        ax = torch.from_numpy(np.stack([mm[4] for mm in full])).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        out[key("floor_ms")] = median_ms(lambda: F.factor_solve_dev(ax.data_ptr(), x.data_ptr(), 1, 0.0, st), refill)
        F.factor_status(st)
    out[key("union_over_floor")] = out[key("union_ms")] / out[key("floor_ms")]
    out[key("embed_over_copy")] = out[key("embed_us")] / out[key("copy_us")]

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
