#!/usr/bin/env python3
"""Transposed solves against plain ones, one GPU, one JSON line (median event-timed ms over --reps after warm-up):
  * config 3 (the 50k grid Jacobian, tol 1e-3): solve_dev vs solve_dev(trans=True) at 1, 128 and 1024 right-hand sides;
  * the workaround the transposed solve replaces: factor of A' on an already-analysed handle, then its solve (1 RHS);
  * an LU batch of 128 matrices of 5 000 columns (interleaved sweeps), plain vs transposed, 1 right-hand side.
    python tools/bench_trans.py [--reps 20]"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scipy.sparse as sp
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
        if prep: prep()                          # fresh right-hand sides outside the timed bracket (the solve is in place)
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


out = {}
m, n, Ap, Ai, Ax = synth.grid_jacobian()
F = hip.Factorization(m, n, Ap, Ai)
F.factor(Ax, 1e-3)
for k in (1, 128, 1024):
    B = torch.from_numpy(synth.grid_rhs(n, k)).to(dev).reshape(n, -1); X = torch.empty_like(B)
    for trans in (False, True):
        out["cfg3_%s_%d" % ("trans" if trans else "plain", k)] = timed(
            lambda: F.solve_dev(X.data_ptr(), k, sh, trans=trans), lambda: X.copy_(B))
    out["cfg3_ratio_%d" % k] = out["cfg3_trans_%d" % k] / out["cfg3_plain_%d" % k]
# the workaround: A' analysed once, then factor + solve per Newton step
At = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n)).T.tocsc(); At.sort_indices()
Ft = hip.Factorization(n, n, At.indptr.astype(np.int32), At.indices.astype(np.int32))
d_atx = torch.from_numpy(At.data.copy()).to(dev)
B = torch.from_numpy(synth.grid_rhs(n, 1)).to(dev).reshape(-1); X = torch.empty_like(B)
Ft.factor_dev(d_atx.data_ptr(), 1e-3, sh); Ft.factor_status(sh)


def workaround():
    Ft.factor_dev(d_atx.data_ptr(), 1e-3, sh)
    Ft.solve_dev(X.data_ptr(), 1, sh)


out["cfg3_workaround_factor_solve_1"] = timed(workaround, lambda: X.copy_(B))
Ft.factor_status(sh); Ft.close()
F.close()
# LU batch of 128: lane = matrix sweeps
mb, nb_, Bp, Bi, Bx = synth.grid_jacobian(n=5000, seed=5000)
rng = np.random.default_rng(0)
AX = Bx[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(128, len(Bx))))
G = hip.Factorization(mb, nb_, Bp, Bi, batch=128)
G.factor(AX, 1e-3)
Bb = torch.from_numpy(rng.standard_normal((128, nb_))).to(dev); Xb = torch.empty_like(Bb)
for trans in (False, True):
    out["batch128_%s_1" % ("trans" if trans else "plain")] = timed(
        lambda: G.solve_dev(Xb.data_ptr(), 1, sh, trans=trans), lambda: Xb.copy_(Bb))
out["batch128_ratio_1"] = out["batch128_trans_1"] / out["batch128_plain_1"]
G.close()
print(json.dumps({k: round(v, 4) for k, v in out.items()}))
