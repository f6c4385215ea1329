#!/usr/bin/env python3
"""Sparse right-hand sides, Y = C A^-1 B, against what they are made of and against what they replace, one GPU, one JSON
line (median event-timed ms over --reps after warm-up).  Config 3 (the 50k grid Jacobian, LU, tol 1e-3), factors held;
--p monitored rows with two entries each, --k injection columns with one or two entries each:
  * right_ms / left_ms / auto_ms: one sens_solve_dev from either side and with side "auto" (auto_side: what it picked);
  * right_solves_ms / left_solves_ms: the plain solve_dev / solve_t_dev calls at the same widths (one per tile), timed
    alone on dense blocks, and the ratio call / sum of its solves;
  * per side the two kernels alone (cs3_debug_sens_parts): scatter_ms, combine_ms, the bytes they move (the scatter writes
    every tile once; the combine reads one row of the tile per entry of the other operand and writes its block of Y) and
    the rates;
  * today_ms: the path without this feature -- B densified on the host 1024 columns at a time, F.solve from host arrays
    (both PCIe crossings), C @ X on the host -- wall clock, median of --host-reps.
    python tools/bench_sens.py [--reps 20] [--k 8192] [--p 1024] [--out profiles/sens_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from csparse3_amd import csc_hip as hip, synth
import sens_cases as sc
import sens_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--k", type=int, default=8192)
ap.add_argument("--p", type=int, default=1024)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--out", default=None)
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
B = sc.incidence(n, args.k, seed=8192)
Ct = sc.incidence(n, args.p, seed=1024, single_every=1 << 30)            # every monitored row has two entries
d_bx, d_cx = (torch.from_numpy(np.array(o.values)).to(dev) for o in (B, Ct))
d_y = torch.empty((args.p, args.k), dtype=torch.float64, device=dev)
out = {"n": n, "k": args.k, "p": args.p, "nnz_b": int(B.indptr[-1]), "nnz_c": int(Ct.indptr[-1]), "reps": args.reps}
F = hip.Factorization(m, n, Ap, Ai)
F.factor(Ax, 1e-3)
lim = hip.sens_limits()

results = {}
for side in ("right", "left", "auto"):
    with F.sens_plan(B[:3], Ct[:3], side=side) as plan:
        info = plan.info
        run = lambda parts=7: F.debug_sens_parts(plan, parts, d_bx.data_ptr(), d_cx.data_ptr(), d_y.data_ptr(), sh)   # noqa: E731
        out[side + "_ms"] = timed(lambda: F.sens_solve_dev(plan, d_bx.data_ptr(), d_cx.data_ptr(), d_y.data_ptr(), sh))
        results[side] = d_y.cpu().numpy()
        if side == "auto":
            out["auto_side"] = "right" if info.side == sr.RIGHT else "left"
            continue
        ns, ng, nnz_other = (args.k, args.p, out["nnz_c"]) if side == "right" else (args.p, args.k, out["nnz_b"])
        tl = sr.tiles(ns, lim)
        assert info.ntiles == len(tl)
        out[side + "_tiles"] = [[t, w] for _, t, w in tl]
        trans = side == "left"
        solves = 0.0
        for w in sorted({w for _, _, w in tl}):
            d_z = torch.zeros((n, w), dtype=torch.float64, device=dev)
            d_z[torch.arange(w, device=dev) * 7 % n, torch.arange(w, device=dev)] = 1.0
            d_z0 = d_z.clone()
            t_w = timed(lambda: F.solve_dev(d_z.data_ptr(), w, sh, trans=trans), lambda: d_z.copy_(d_z0))
            out["%s_solve_%d_ms" % ("solve_t" if trans else "solve", w)] = t_w
            solves += t_w * sum(1 for _, _, ww in tl if ww == w)
            del d_z, d_z0
        out[side + "_solves_ms"] = solves
        out[side + "_over_solves"] = out[side + "_ms"] / solves
        sc_bytes = sum(8 * n * w for _, _, w in tl)
        cb_bytes = sum(8 * t * (nnz_other + ng) for _, t, _ in tl)
        out[side + "_scatter_ms"] = timed(lambda: run(1))
        out[side + "_combine_ms"] = timed(lambda: run(4))
        out[side + "_scatter_bytes"], out[side + "_combine_bytes"] = int(sc_bytes), int(cb_bytes)
        out[side + "_scatter_TBps"] = sc_bytes / out[side + "_scatter_ms"] * 1e-9
        out[side + "_combine_TBps"] = cb_bytes / out[side + "_combine_ms"] * 1e-9
scale = np.abs(results["right"]).max()
out["left_vs_right_rel"] = float(np.abs(results["left"] - results["right"]).max() / scale)
out["auto_is_faster_side"] = out["auto_side"] == ("right" if out["right_ms"] <= out["left_ms"] else "left")
assert out["left_vs_right_rel"] < 1e-10 and np.array_equal(results["auto"], results[out["auto_side"]])

# today: densify on the host, solve from host arrays, multiply on the host
Bs, Cs = sr.to_scipy(B, n), sr.to_scipy(Ct, n).T.tocsr()
walls = []
for _ in range(args.host_reps):
    t0 = time.perf_counter()
    Y = np.empty((args.p, args.k))
    for c0 in range(0, args.k, lim.max_tile):
        c1 = min(args.k, c0 + lim.max_tile)
        Y[:, c0:c1] = Cs @ F.solve(Bs[:, c0:c1].toarray())
    walls.append((time.perf_counter() - t0) * 1e3)
out["today_ms"] = float(np.median(walls))
out["today_vs_right_rel"] = float(np.abs(Y - results["right"]).max() / scale)
out["today_over_auto"] = out["today_ms"] / out["auto_ms"]
F.close()
line = json.dumps({k: (float("%.4g" % v) if isinstance(v, float) and abs(v) < 1e-3 else round(v, 4) if isinstance(v, float) else v)
                   for k, v in out.items()})
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
