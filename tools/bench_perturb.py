#!/usr/bin/env python3
"""What static pivot perturbation (cs3_set_pivot_perturbation) costs, one GPU, one JSON line: the fused step
cs3_factor_solve_bx_dev, 1 RHS, on config 3 (the 50k grid Jacobian, tol 1e-3) with delta = 0 (the kernels of a handle that
never heard of it) against delta = sqrt(eps) max|Ax| (the perturbing instances; no pivot of this matrix is that small,
so both compute the same factors), two handles in one process, alternating, median of event-timed ms over --reps after
warm-up, --rounds times; and the number of pivots the second handle replaced.
    python tools/bench_perturb.py [--reps 50] [--rounds 3]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream


def timed(body, warm=5):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


m, n, Ap, Ai, Ax = synth.grid_jacobian()
delta = hip.perturbation_delta(True, Ax, False)
off = hip.Factorization(m, n, Ap, Ai)
on = hip.Factorization(m, n, Ap, Ai).set_perturbation(delta)
ax = torch.from_numpy(Ax).to(dev)
b = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).to(dev)
x = {"off": torch.empty_like(b), "on": torch.empty_like(b)}
rows = {"off": [], "on": []}
for _ in range(args.rounds):
    for tag, F in (("off", off), ("on", on)):
        rows[tag].append(timed(lambda: F.factor_solve_bx_dev(ax.data_ptr(), b.data_ptr(), x[tag].data_ptr(), 1, 1e-3, sh)))
for F in (off, on):
    F.factor_status(sh)
out = {"n": n, "delta": delta, "perturbed": int(on.perturbed(sh)[0]),
       "fused1_delta0_ms": [round(v, 4) for v in rows["off"]], "fused1_delta_ms": [round(v, 4) for v in rows["on"]],
       "delta_minus_delta0_us": round(1e3 * (np.median(rows["on"]) - np.median(rows["off"])), 2),
       "same_bits": bool(torch.equal(x["off"], x["on"]))}
off.close(); on.close()
print(json.dumps(out))
