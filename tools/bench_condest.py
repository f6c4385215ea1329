#!/usr/bin/env python3
"""Condition estimates and log-determinants against the solves they are built from, one GPU, one JSON line (median
event-timed ms over --reps after warm-up), for
  * config 3 (the 50k grid Jacobian, LU, tol 1e-3),
  * the config-5 batch (512 SPD matrices of 5 000 columns, Cholesky),
  * an LU batch of 128 matrices of 5 000 columns:
solve_dev (1 RHS), solve_dev(trans=True), condest (host form: adaptive slots, values staged from host memory),
condest_dev (11 fixed slots) and slogdet_dev; plus the number of solves the host form ran for config 3 (from the port
in tests/lacn2_ref.py, which runs the same sequence).
    python tools/bench_condest.py [--reps 20]"""
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


def timed(body, prep=None, warm=3):
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


def legs(tag, F, AX):
    nb = F.batch
    AX = np.ascontiguousarray(AX, dtype=np.float64).reshape(-1)
    d_ax = torch.from_numpy(AX.copy()).to(dev)
    B = torch.from_numpy(np.random.default_rng(0).standard_normal(nb * F.n)).to(dev)
    X = torch.empty_like(B)
    c = torch.empty(nb, dtype=torch.float64, device=dev); i = torch.empty_like(c)
    s = torch.empty_like(c); l = torch.empty_like(c)
    out = {}
    out[tag + "_solve"] = timed(lambda: F.solve_dev(X.data_ptr(), 1, sh), lambda: X.copy_(B))
    out[tag + "_solve_t"] = timed(lambda: F.solve_dev(X.data_ptr(), 1, sh, trans=True), lambda: X.copy_(B))
    out[tag + "_condest_host"] = timed(lambda: F.condest(AX))
    out[tag + "_condest_dev"] = timed(lambda: F.condest_dev(d_ax.data_ptr(), c.data_ptr(), i.data_ptr(), sh))
    out[tag + "_slogdet_dev"] = timed(lambda: F.slogdet_dev(s.data_ptr(), l.data_ptr(), sh))
    # the host form's Ax upload alone (pageable host memory, as cs3_condest copies it)
    out[tag + "_ax_upload"] = timed(lambda: d_ax.copy_(torch.from_numpy(AX)))
    return out


out = {}
m, n, Ap, Ai, Ax = synth.grid_jacobian()
F = hip.Factorization(m, n, Ap, Ai)
F.factor(Ax, 1e-3)
out.update(legs("cfg3", F, Ax))
F.close()
ei, ej = synth.spd_grid_pattern(5000, seed=5000)
mats = [synth.spd_grid_matrix(5000, ei, ej, seed=5001 + b) for b in range(512)]
G = hip.Factorization(5000, 5000, mats[0][2], mats[0][3], kind=hip.CS3_CHOLESKY, batch=512)
AX5 = np.stack([x[4] for x in mats])
G.factor(AX5)
out.update(legs("chol512", G, AX5))
G.close()
mb, nb_, Bp, Bi, Bx = synth.grid_jacobian(n=5000, seed=5000)
AX = Bx[None, :] * (1.0 + 0.05 * np.random.default_rng(0).uniform(-1.0, 1.0, size=(128, len(Bx))))
H = hip.Factorization(mb, nb_, Bp, Bi, batch=128)
H.factor(AX, 1e-3)
out.update(legs("lu128", H, AX))
H.close()
for tag in ("cfg3", "chol512", "lu128"):
    tf, tt = out[tag + "_solve"], out[tag + "_solve_t"]
    out[tag + "_dev_over_6F5T"] = out[tag + "_condest_dev"] / (6 * tf + 5 * tt)
out["cfg3_host_over_3F1T"] = out["cfg3_condest_host"] / (3 * out["cfg3_solve"] + out["cfg3_solve_t"])
out["cfg3_host_minus_upload_over_3F1T"] = ((out["cfg3_condest_host"] - out["cfg3_ax_upload"])
                                           / (3 * out["cfg3_solve"] + out["cfg3_solve_t"]))
print(json.dumps({k: round(v, 4) for k, v in out.items()}))
