#!/usr/bin/env python3
"""Low-rank-modified solves against what they are made of and against what they replace, one GPU, one JSON line (median
event-timed ms over --reps after warm-up).  Config 3 (the 50k grid Jacobian, LU, tol 1e-3), factors held, --cases branch
outages by seed:
  * updates_ms: one solve_updates_dev of the whole list;
  * solves_ms: the plain solve_dev calls of the same widths (one per tile) + the one-column solve, and the ratio;
  * refactor_ms_per_case: the only way without this path -- the case's values edited in HBM and factor_solve_dev --
    over --refactor-cases cases, and the whole list priced from it.  With --only-refactor nothing else runs (and no
    entry point of the low-rank path is touched: this leg also runs on a library built from an older commit, through
    CS3_LIB_PATH);
  * apply_bytes: what k_upd_apply moves per call (Z read once + X written once), to set against its time in a kernel
    trace of this tool.
    python tools/bench_updates.py [--reps 20] [--cases 1024]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from csparse3_amd import csc_hip as hip, synth
from helpers import csc_to_scipy
import updates_ref as ur

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--cases", type=int, default=1024)
ap.add_argument("--refactor-cases", type=int, default=64)
ap.add_argument("--only-refactor", action="store_true")
ap.add_argument("--n", type=int, default=50000)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream


def timed(body, prep=None, warm=3, reps=None):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps or args.reps)]
    for _ in range(warm):
        if prep: prep()
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        if prep: prep()
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


m, n, Ap, Ai, Ax = synth.grid_jacobian(n=args.n) if args.n != 50000 else synth.grid_jacobian()
A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsc()
A.sort_indices()
cases = ur.branch_outages(A, args.cases, seed=1024)
b = np.random.default_rng(0).standard_normal(n)
d_b = torch.from_numpy(b.copy()).to(dev)
out = {"n": n, "cases": len(cases)}
F = hip.Factorization(m, n, Ap, Ai)
F.factor(Ax, 1e-3)

# the per-case refactorisation: entry positions of (i, j) in the analysed value array, values edited in HBM
pos = {}
cols = np.repeat(np.arange(n), np.diff(Ap))
for c in cases[:args.refactor_cases]:
    for i, j in zip(c[0], c[1]):
        p = Ap[j] + int(np.searchsorted(Ai[Ap[j]:Ap[j + 1]], i))
        assert Ai[p] == i and cols[p] == j
        pos[(int(i), int(j))] = p
d_ax0 = torch.from_numpy(np.asarray(Ax, dtype=np.float64).copy()).to(dev)
d_ax = d_ax0.clone()
d_x = torch.empty(n, dtype=torch.float64, device=dev)
edits = [(torch.tensor([pos[(int(i), int(j))] for i, j in zip(c[0], c[1])], device=dev),
          torch.from_numpy(np.asarray(c[2])).to(dev)) for c in cases[:args.refactor_cases]]


def refactor_all():
    for idx, val in edits:
        d_ax.copy_(d_ax0)
        d_ax.index_add_(0, idx, val)
        F.factor_solve_bx_dev(d_ax.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, 1e-3, sh)


per_case = timed(refactor_all, reps=5, warm=1) / len(edits)
F.factor_status(sh)
out["refactor_ms_per_case"] = per_case
out["refactor_ms_whole_list"] = per_case * len(cases)
if not args.only_refactor:
    F.factor(Ax, 1e-3)
    pattern, cx = ur.flatten(cases)
    d_cx = torch.from_numpy(cx.copy()).to(dev)
    plan = F.updates_plan(pattern)
    info, tiles = plan.info, plan.tiles()
    out.update(rows_unique=info.nrows_unique, tiles=[[int(v) for v in t] for t in tiles])
    d_X = torch.empty((n, len(cases)), dtype=torch.float64, device=dev)
    d_r = torch.empty(len(cases), dtype=torch.float64, device=dev)
    out["updates_ms"] = timed(lambda: F.solve_updates_dev(plan, d_cx.data_ptr(), d_b.data_ptr(), d_X.data_ptr(),
                                                          d_r.data_ptr(), 1e-10, sh))
    assert bool(torch.isfinite(d_X).all()) and float(d_r.min()) > 1e-6
    solves = timed(lambda: F.solve_dev(d_x.data_ptr(), 1, sh), lambda: d_x.copy_(d_b))
    out["solve_1_ms"] = solves
    for w in sorted(set(int(t[3]) for t in tiles)):
        d_Z = torch.zeros((n, w), dtype=torch.float64, device=dev)
        d_Z[torch.arange(w, device=dev) * 7 % n, torch.arange(w, device=dev)] = 1.0
        d_Z0 = d_Z.clone()
        t_w = timed(lambda: F.solve_dev(d_Z.data_ptr(), w, sh), lambda: d_Z.copy_(d_Z0))
        out["solve_%d_ms" % w] = t_w
        solves += t_w * sum(1 for t in tiles if int(t[3]) == w)
        del d_Z, d_Z0
    out["solves_ms"] = solves
    out["updates_over_solves"] = out["updates_ms"] / solves
    out["refactor_over_updates"] = out["refactor_ms_whole_list"] / out["updates_ms"]
    out["apply_bytes"] = int(sum(8 * n * (int(t[3]) + int(t[1])) for t in tiles))
    out["units_bytes"] = int(sum(8 * n * int(t[3]) for t in tiles))
    plan.close()
F.close()
print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))
