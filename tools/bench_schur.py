#!/usr/bin/env python3
"""Schur handles against the route that exists without them, one GPU, one JSON line per border set (median event-timed ms
over --reps after warm-up).  Config 3 (the 50k grid Jacobian, LU, tol 1e-3); border sets of --ns variables drawn as a
contiguous index range ("range") and as random buses ("random"):
  * plain_factor_ms: factor_dev of the whole matrix on a plain handle (what a Schur factorisation is set against);
  * schur_factor_ms: factor_dev on the Schur handle (S is in the handle's buffer afterwards), nnz_l and flops of both;
  * halves_k1_ms / halves_k128_ms: schur_forward_dev + schur_backward_dev;
  * take_bytes: what k_schur_take moves per factorisation (front read + S written + identity written), to set against
    its time in a kernel trace of this tool;
  * the route without Schur handles: a plain handle on A11 (route_factor_ms), solve_dev with the ns densified columns
    of A12 (route_solve_ms), then X to the host and A22 - A21 @ X there (route_host_ms, wall clock); route_ms their sum.
    python tools/bench_schur.py [--reps 20] [--ns 64 512 2048] [--no-route]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from csparse3_amd import csc_hip as hip, synth
from helpers import csc_to_scipy, rel_err

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ns", type=int, nargs="+", default=[64, 512, 2048])
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--no-route", action="store_true")
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


m, n, Ap, Ai, Ax = synth.grid_jacobian(n=args.n) if args.n != 50000 else synth.grid_jacobian()
A = csc_to_scipy(m, n, Ap, Ai, Ax).tocsr()
d_ax = torch.from_numpy(np.asarray(Ax, dtype=np.float64).copy()).to(dev)
with hip.Factorization(m, n, Ap, Ai) as P:
    plain = dict(plain_factor_ms=timed(lambda: P.factor_dev(d_ax.data_ptr(), 1e-3, sh)), plain_nnz_l=int(P.info.nnz_l),
                 plain_gflop=P.info.flops_factor / 1e9)
    P.factor_status(sh)

for ns in args.ns:
    for draw in ("range", "random"):
        idx = (np.arange(n // 2, n // 2 + ns) if draw == "range"
               else np.random.default_rng(ns).choice(n, size=ns, replace=False)).astype(np.int32)
        out = dict(n=n, ns=ns, draw=draw, **plain)
        try:
            F = hip.Factorization(m, n, Ap, Ai, schur=idx)
        except hip.Cs3Error as e:
            out["error"] = str(e)
            print(json.dumps(out)); continue
        info = F.info
        out.update(schur_nnz_l=int(info.nnz_l), schur_gflop=info.flops_factor / 1e9, max_front=int(info.max_front),
                   factor_mbytes=info.factor_bytes / 1e6)
        out["schur_factor_ms"] = timed(lambda: F.factor_dev(d_ax.data_ptr(), 1e-3, sh))
        F.factor_status(sh)
        S = F.schur()
        out["take_bytes"] = 3 * 8 * ns * ns
        for k in (1, 128):
            d_x = torch.randn((n, k), dtype=torch.float64, device=dev)
            out["halves_k%d_ms" % k] = timed(lambda: (F.schur_forward_dev(d_x.data_ptr(), k, sh),
                                                        F.schur_backward_dev(d_x.data_ptr(), k, sh)))
            del d_x
        F.close()
        if not args.no_route:
            mask = np.ones(n, dtype=bool); mask[idx] = False
            inter = np.flatnonzero(mask)
            A11 = A[inter][:, inter].tocsc(); A11.sort_indices()
            A12 = A[inter][:, idx].toarray()
            A21, A22 = A[idx][:, inter].tocsr(), A[idx][:, idx].toarray()
            n1 = len(inter)
            d_a11 = torch.from_numpy(A11.data.copy()).to(dev)
            d_b = torch.from_numpy(A12).to(dev)
            d_x = torch.empty_like(d_b)
            with hip.Factorization(n1, n1, A11.indptr.astype(np.int32), A11.indices.astype(np.int32)) as R:
                out["route_factor_ms"] = timed(lambda: R.factor_dev(d_a11.data_ptr(), 1e-3, sh))
                R.factor_status(sh)
                out["route_solve_ms"] = timed(lambda: R.solve_dev(d_x.data_ptr(), ns, sh), lambda: d_x.copy_(d_b))
                torch.cuda.synchronize()
                host = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    S_route = A22 - A21 @ d_x.cpu().numpy()
                    host.append(1e3 * (time.perf_counter() - t0))
                out["route_host_ms"] = float(np.median(host))
            out["route_ms"] = out["route_factor_ms"] + out["route_solve_ms"] + out["route_host_ms"]
            out["schur_vs_route_rel_diff"] = rel_err(S, S_route)
            del d_a11, d_b, d_x
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
