#!/usr/bin/env python3
"""What the doubled-precision residual and one extra-precise refinement pass (cs3_refine_xp_dev) cost next to the plain
residual and one stationary round (cs3_refine_dev) on the same handle, one GPU, one JSON line, also written to
profiles/refine_xp_bench.json.  Config 3 (the 50k grid Jacobian) at k = 1, 16, 128; the factors are those of A0 and the
values refined against are A0 (1 + 1e-9 noise), so that every system needs a second correction.
  residual: k_residual_xp (with a tail, writing r only, as the iteration runs it) against k_residual_rows, both
    event-timed without any synchronisation (median of --reps), with the GB/s of the traffic both share: per entry a value
    and two indices once per row pass, the gathered x per right-hand side, and b and r per output (the doubled kernel
    gathers the tail as well);
  pass: [call capped at 2 corrections] - [call capped at 1], event-timed around the whole call: the doubled residual, the
    solve, the maxima, the control and update kernels and the 4-byte read that synchronises the stream; against one
    cs3_refine_dev round (residual, solve, axpy; no synchronisation) in the same visit.
    python tools/bench_refine_xp.py [--reps 20]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream


def timed(body, warm=3):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


m, n, Ap, Ai, Ax0 = synth.grid_jacobian()
nnz = int(Ap[n])
rng = np.random.default_rng(5)
Ax = Ax0 * (1.0 + 1e-9 * rng.standard_normal(Ax0.size))
F = hip.Factorization(m, n, Ap, Ai).factor(Ax0)
ax = torch.from_numpy(Ax).to(dev)
out = {"n": n, "nnz": nnz, "reps": args.reps, "configs": []}
for k in (1, 16, 128):
    b_h = rng.standard_normal((n, k))
    x0_h = F.solve(b_h)
    b, x0 = torch.from_numpy(b_h).to(dev), torch.from_numpy(x0_h).to(dev)
    x, xt, r = torch.empty_like(x0), torch.zeros_like(x0), torch.empty_like(x0)
    x.copy_(x0)

    def call(cap):
        x.copy_(x0)
        return F.refine_xp_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), k, cap, 0, sh)

    full = call(10)
    plain_ms = timed(lambda: F.residual_dev(ax.data_ptr(), b.data_ptr(), x0.data_ptr(), r.data_ptr(), k, sh))
    xp_ms = timed(lambda: F.residual_xp_dev(ax.data_ptr(), b.data_ptr(), x0.data_ptr(), r.data_ptr(), 0, xt.data_ptr(), k, sh))
    round_ms = timed(lambda: F.refine_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), k, 1, sh, want_correction=False))
    capped = {c: timed(lambda c=c: call(c)) for c in (1, 2)}
    ran = {c: int(call(c)["iters"].min()) for c in (1, 2)}
    assert ran == {1: 1, 2: 2}, ran                  # every system ran all the corrections the cap allows
    pass_ms = capped[2] - capped[1]
    # bytes both kernels move at the least: the row view (two ints per entry and the value), x gathered per entry and
    # right-hand side, b read and r written per output
    traffic = 16.0 * nnz + 8.0 * nnz * k + 16.0 * n * k
    out["configs"].append({
        "k": k, "iters_to_converge_max": int(full["iters"].max()), "flags": sorted(set(int(f) for f in full["flag"])),
        "residual_rows_ms": round(plain_ms, 4), "residual_xp_ms": round(xp_ms, 4),
        "residual_ratio": round(xp_ms / plain_ms, 3),
        "residual_rows_GBps": round(traffic / plain_ms / 1e6, 1),
        "residual_xp_GBps": round((traffic + 8.0 * nnz * k) / xp_ms / 1e6, 1),
        "refine_round_ms": round(round_ms, 4), "capped_call_ms": {str(c): round(v, 4) for c, v in capped.items()},
        "xp_pass_ms": round(pass_ms, 4), "pass_ratio_to_refine_round": round(pass_ms / round_ms, 3)})
F.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "refine_xp_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
