#!/usr/bin/env python3
"""Selected inversion against the route it replaces, one GPU, one JSON line (median event-timed ms over --reps after
warm-up).  Config 3 (the 50k grid Jacobian, LU), factors held, all in one process:
  * a_selinv_ms: cs3_selinv_dev;
  * b_selinv_diag_ms: cs3_selinv_dev + cs3_selinv_diag_dev, the n diagonal entries of A^-1;
  * c_sens_diag_ms: the same n entries by sens_solve_dev with unit B and C, one plan per tile of 1024 columns
    (Y = E' A^-1 E is 1024 x 1024 per tile, its diagonal is kept);
  * d_factor_ms: one factor_dev, for scale;
  * the launch count, the ratios b / c and a / d, and the max error of (b) against (c) on one tile of 1024 entries.
The same (a), (b), (d) on a batch of 64 spd_grid_matrix(5000) through Cholesky (the sens route takes no batch).
--kernel-stats FILE: a rocprofv3 --kernel-trace --stats CSV of a run of this tool; the time per kernel family of
selinv.hip is read from it (kernel_ms: average per call, and the calls seen).
    python tools/bench_selinv.py [--reps 20] [--n 50000] [--skip-sens] [--kernel-stats FILE] [--out profiles/selinv_bench.json]"""
import argparse, csv, json, os, re, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--skip-sens", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream
TILE = int(hip.sens_limits().max_tile)


def timed(body, warm=2):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def measure(F, d_ax, batch, n):
    """(a), (b), (d) and the plan's sizes of a factorised handle; -> (dict, the diagonal as a device tensor)."""
    d_diag = torch.empty((batch, n), dtype=torch.float64, device=dev)
    L = hip.lib()

    def selinv_diag():
        F.selinv(sh)
        hip._check(L.cs3_selinv_diag_dev(F._h, d_diag.data_ptr(), sh))

    info = F.selinv_info()
    res = {"a_selinv_ms": timed(lambda: F.selinv(sh)), "b_selinv_diag_ms": timed(selinv_diag),
           "d_factor_ms": timed(lambda: F.factor_dev(d_ax.data_ptr(), 0.0, sh)),
           "nlaunches": int(info.nlaunches), "nfronts_small": int(info.nfronts_small), "nfronts_big": int(info.nfronts_big),
           "zpool_mbytes": info.zpool_doubles * 8 * batch / 1e6}
    res["a_over_d"] = res["a_selinv_ms"] / res["d_factor_ms"]
    selinv_diag()
    torch.cuda.synchronize()
    return res, d_diag


out = {"reps": args.reps}
m, n, Ap, Ai, Ax = synth.grid_jacobian(n=args.n) if args.n != 50000 else synth.grid_jacobian()
F = hip.Factorization(m, n, Ap, Ai)
d_ax = torch.from_numpy(np.ascontiguousarray(Ax[:Ap[n]])).to(dev)
F.factor_dev(d_ax.data_ptr(), 0.0, sh)
F.factor_status(sh)
cfg3, d_diag = measure(F, d_ax, 1, n)
cfg3["n"] = n
if not args.skip_sens:
    tiles = [(c0, min(TILE, n - c0)) for c0 in range(0, n, TILE)]
    plans = []
    for c0, t in tiles:                                   # B = columns c0 .. c0 + t of I, C = the same rows of I
        unit = (t, np.arange(t + 1, dtype=np.int32), np.arange(c0, c0 + t, dtype=np.int32))
        plans.append(F.sens_plan(unit, unit, side="right"))
    ones = torch.ones(TILE, dtype=torch.float64, device=dev)
    d_y = torch.empty((TILE, TILE), dtype=torch.float64, device=dev)
    d_sens = torch.empty(n, dtype=torch.float64, device=dev)

    def sens_diag():
        for (c0, t), plan in zip(tiles, plans):
            F.sens_solve_dev(plan, ones.data_ptr(), ones.data_ptr(), d_y.data_ptr(), sh)
            d_sens[c0:c0 + t] = d_y.view(-1)[:t * t].view(t, t).diagonal()

    cfg3["c_sens_diag_ms"] = timed(sens_diag, warm=1)
    cfg3["sens_tiles"] = len(tiles)
    cfg3["b_over_c"] = cfg3["b_selinv_diag_ms"] / cfg3["c_sens_diag_ms"]
    c0, t = tiles[len(tiles) // 2]
    got, want = d_diag[0, c0:c0 + t].cpu().numpy(), d_sens[c0:c0 + t].cpu().numpy()
    cfg3["max_err_vs_sens_on_one_tile"] = float(np.abs(got - want).max() / np.abs(want).max())
    for plan in plans:
        plan.close()
F.close()
out["config3_lu"] = cfg3

nb, ns = 64, 5000
ei, ej = synth.spd_grid_pattern(ns)
mats = [synth.spd_grid_matrix(ns, ei, ej, seed=s) for s in range(nb)]
m, n, Ap, Ai = mats[0][:4]
AX = np.stack([c[4][:Ap[n]] for c in mats])
F = hip.Factorization(m, n, Ap, Ai, hip.CS3_CHOLESKY, batch=nb)
d_ax = torch.from_numpy(AX).to(dev)
F.factor_dev(d_ax.data_ptr(), 0.0, sh)
F.factor_status(sh)
out["spd5000_batch64_cholesky"], _ = measure(F, d_ax, nb, n)
out["spd5000_batch64_cholesky"].update(n=n, batch=nb)
F.close()

if args.kernel_stats:
    fam = {}
    with open(args.kernel_stats) as f:
        for row in csv.DictReader(f):
            if "k_selinv" in row["Name"]:
                name = re.search(r"k_selinv\w*(<[^>]*>)?", row["Name"]).group(0)
                fam[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    out["kernel_families"] = fam

line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
