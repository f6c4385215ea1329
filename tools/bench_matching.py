#!/usr/bin/env python3
"""What a matched handle (cs3_analyze_matched) costs, one GPU, one JSON line:
  * the fused step cs3_factor_solve_dev, 1 RHS, on config 3 (the 50k grid Jacobian, tol 1e-3): a plain handle against a
    matched handle built from the same matrix (its matching is the identity with scalings, so both run the same schedule),
    in one process, alternating, median of event-timed ms over --reps after warm-up, --rounds times;
  * the same for cs3_solve_dev with 1 and 64 right-hand sides;
  * host seconds of the matching next to t_order_s of the same analysis, on that matrix and on its scrambled form
    (tests/match_cases.scramble: rows permuted, rows and columns scaled over eight decades).
    python tools/bench_matching.py [--reps 50] [--rounds 3]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from csparse3_amd import csc_hip as hip, synth
import match_cases as mc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream


def timed(body, prep=None, warm=5):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        if prep: prep()
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        if prep: prep()
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


m, n, Ap, Ai, Ax = synth.grid_jacobian()
P = hip.Factorization(m, n, Ap, Ai)
M = hip.Factorization(m, n, Ap, Ai, match_values=Ax)
assert np.array_equal(M.matching()[0], np.arange(n))
out = {"n": n, "nnz": int(Ap[n]), "t_match_s": M.match_time, "t_order_s": float(M.info.t_order_s)}
sn, sAp, sAi, sAx, _ = mc.scramble((m, n, Ap, Ai, Ax), 1)
with hip.Factorization(sn, sn, sAp, sAi, match_values=sAx) as S:
    out["scrambled_t_match_s"], out["scrambled_t_order_s"] = S.match_time, float(S.info.t_order_s)
ax = torch.from_numpy(Ax).to(dev)
B = torch.from_numpy(np.random.default_rng(0).standard_normal((n, 64))).to(dev)
b1 = B[:, 0].contiguous()
x1, X = torch.empty_like(b1), torch.empty_like(B)
legs = {"fused1": lambda F: timed(lambda: F.factor_solve_dev(ax.data_ptr(), x1.data_ptr(), 1, 1e-3, sh), lambda: x1.copy_(b1)),
        "solve1": lambda F: timed(lambda: F.solve_dev(x1.data_ptr(), 1, sh), lambda: x1.copy_(b1)),
        "solve64": lambda F: timed(lambda: F.solve_dev(X.data_ptr(), 64, sh), lambda: X.copy_(B))}
for F in (P, M):
    F.factor_dev(ax.data_ptr(), 1e-3, sh)
    F.factor_status(sh)
for leg, run in legs.items():
    rows = {"plain": [], "matched": []}
    for _ in range(args.rounds):
        for tag, F in (("plain", P), ("matched", M)):
            rows[tag].append(run(F))
    for tag in rows:
        out["%s_%s_ms" % (leg, tag)] = [round(v, 4) for v in rows[tag]]
    out["%s_matched_minus_plain_us" % leg] = round(1e3 * (np.median(rows["matched"]) - np.median(rows["plain"])), 2)
xp, xm = b1.clone(), b1.clone()
P.factor_solve_dev(ax.data_ptr(), xp.data_ptr(), 1, 1e-3, sh)
M.factor_solve_dev(ax.data_ptr(), xm.data_ptr(), 1, 1e-3, sh)
torch.cuda.synchronize()
out["max_rel_diff_matched_vs_plain"] = float((xp - xm).abs().max() / xp.abs().max())
P.close(); M.close()
print(json.dumps(out))
