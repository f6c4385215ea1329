#!/usr/bin/env python3
"""What a GMRES iteration on held factors (cs3_gmres_dev) costs next to a stationary refinement round (cs3_refine_dev) on
the same handle, one GPU, one JSON line, also written to profiles/gmres_bench.json.  Config 3 (the 50k grid Jacobian),
k = 1; the factors are those of A0, the values of A have 40 diagonal entries multiplied by 2 .. 41, and rtol = 0 keeps
every system iterating, so a call capped at max_iters = j + 1 runs the iterations 0 .. j (iters_to_1e-12 says what a
real call needs).
  iteration j = [call capped at j + 1] - [call capped at j], both event-timed around the whole call (median of --reps):
    one solve, one product, the six launches of the vector layer and the 4-byte read that synchronises the stream;
  its parts alone, event-timed without any synchronisation: solve_dev + matvec_dev, and the multi-dot and the update of
    iteration j through cs3_debug_gmres_kernel with their GB/s (bytes: the multi-dot reads j + 1 basis vectors and w once
    per 8 of them; the update reads j + 1 basis vectors and w and writes w);
  the synchronisation: iteration - (solve + product + 2 dots + 2 updates), which also holds the two small launches;
  one cs3_refine_dev round (product, solve, axpy; no synchronisation) in the same visit: the yardstick.
    python tools/bench_gmres.py [--reps 30]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream
R, RESTART, JS = 40, 30, (1, 4, 8, 16)


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
rng = np.random.default_rng(3)
Ax = Ax0.copy()
for f, i in enumerate(rng.choice(n, size=R, replace=False)):
    p = Ap[i] + int(np.flatnonzero(Ai[Ap[i]:Ap[i + 1]] == i)[0])
    Ax[p] *= 2.0 + f
F = hip.Factorization(m, n, Ap, Ai).factor(Ax0)
b_h = rng.standard_normal(n)
x0_h = F.solve(b_h)
ax, b, x0 = (torch.from_numpy(a).to(dev) for a in (Ax, b_h, x0_h))
x, y = torch.empty_like(x0), torch.empty_like(x0)


def call(max_iters, rtol=0.0):
    x.copy_(x0)
    return F.gmres_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), 1, rtol, RESTART, max_iters, sh)


iters, relres = call(100, 1e-12)
out = {"n": n, "k": 1, "restart": RESTART, "iters_to_1e-12": int(iters[0]), "relres": float(relres[0]),
       "launches_per_iteration_besides_solve_and_product": 6}
lib = hip.lib()
refine_ms = timed(lambda: F.refine_dev(ax.data_ptr(), b.data_ptr(), x.data_ptr(), 1, 1, sh, want_correction=False))
solve_ms = timed(lambda: F.solve_dev(y.data_ptr(), 1, sh))
matvec_ms = timed(lambda: F.matvec_dev(ax.data_ptr(), x0.data_ptr(), y.data_ptr(), 1, sh))
out.update(refine_round_ms=round(refine_ms, 4), solve_ms=round(solve_ms, 4), matvec_ms=round(matvec_ms, 4))
capped = {c: timed(lambda c=c: call(c)) for c in sorted({j for j in JS} | {j + 1 for j in JS})}
ran = {c: int(call(c)[0][0]) for c in capped}
assert all(ran[c] == c for c in capped), ran         # every capped call ran all its iterations
out["capped_call_ms"] = {str(c): round(v, 4) for c, v in capped.items()}
rows = []
for j in JS:
    it_ms = capped[j + 1] - capped[j]
    probe = [timed(lambda w=w: lib.cs3_debug_gmres_kernel(F._h, w, j, sh)) for w in (0, 1, 2)]
    dot_bytes = 8.0 * n * ((j + 1) + -(-(j + 1) // 8))
    upd_bytes = 8.0 * n * (j + 3)
    parts = solve_ms + matvec_ms + 2 * probe[0] + probe[1] + probe[2]
    rows.append({"j": j, "iteration_ms": round(it_ms, 4), "ratio_to_refine_round": round(it_ms / refine_ms, 3),
                 "dot_ms": round(probe[0], 4), "dot_GBps": round(dot_bytes / probe[0] / 1e6, 1),
                 "update_ms": round(probe[1], 4), "update_GBps": round(upd_bytes / probe[1] / 1e6, 1),
                 "update_norm_ms": round(probe[2], 4),
                 "enqueued_parts_ms": round(parts, 4), "ratio_of_parts_to_refine_round": round(parts / refine_ms, 3),
                 "sync_and_small_launches_ms": round(it_ms - parts, 4)})
out["iterations"] = rows
F.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "gmres_bench.json"), "w") as f:
    f.write(line + "\n")
print(line)
