#!/usr/bin/env python3
"""Entries of Z-bus and Kron reduction on a complex handle, against what they are made of and against what they replace:
one GPU, one JSON line (median event-timed ms over --reps after warm-up).  The matrix is synth.ybus at --n buses with
--edges branches (the chords beyond the spanning tree are random: fill grows quickly with them), LU with the rotation,
factors held; --p rows of C with two entries each, --k columns of B with one or two entries each, complex values.
  * right_ms / left_ms / auto_ms: one ComplexFactorization.sens_solve_dev from either side and with side "auto";
  * (a) right_solves_ms / left_solves_ms: the real handle's solve_dev / solve_t_dev at the widths the call is made of (one
    per tile) on dense [2n, w] blocks, and the ratio call / sum of its solves; per side the two kernels alone
    (cs3_debug_cplx_sens_parts);
  * (b) composed_ms: what the library allowed before: B densified on the host one tile at a time, ComplexFactorization.
    solve_dev on the tile (upload, pack, solve, unpack, download), C @ X on the host -- wall clock, median of --host-reps;
  * real_left_width: the solved-for columns side left would need through cs3_sens_plan on the real form, 2p against p;
  * kron: for every --ns boundary buses the factorisation of the Schur handle (values + factor) next to that of the plain
    complex handle, and the read-out of S.
    python tools/bench_csens.py [--reps 20] [--out profiles/csens_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from csparse3_amd import csc_hip as hip, synth
import csens_cases as cc
import sens_cases as sc
import sens_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--k", type=int, default=8192)
ap.add_argument("--p", type=int, default=1024)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--edges", type=int, default=None, help="branches; default n + n / 50")
ap.add_argument("--ns", type=int, nargs="*", default=[64, 256])
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


edges = args.edges if args.edges is not None else args.n + args.n // 50
n, Ap, Ai, Az = synth.ybus(args.n, edges, seed=args.n)
B = cc.cplx(sc.incidence(n, args.k, seed=8192), 1)
Ct = cc.cplx(sc.incidence(n, args.p, seed=1024, single_every=1 << 30), 2)     # every row of C has two entries
d_bz, d_cz = (torch.from_numpy(np.array(o.values)).to(dev) for o in (B, Ct))
d_y = torch.empty((args.p, args.k), dtype=torch.complex128, device=dev)
d_az = torch.from_numpy(Az).to(dev)
out = {"n": n, "edges": edges, "nnz": int(Ap[n]), "k": args.k, "p": args.p, "nnz_b": int(B.indptr[-1]), "nnz_c": int(Ct.indptr[-1]),
       "reps": args.reps}
F = hip.ComplexFactorization(n, Ap, Ai)
F.factor(Az)
out["nnz_l_real"], out["max_front_real"] = int(F.real.info.nnz_l), int(F.real.info.max_front)
lim = hip.cplx_sens_limits()
rx = F.plan.workspace_dev(0, 4 * F.nnz)


def refactor(G):
    G.plan.values_dev(d_az.data_ptr(), rx, sh)
    G.real.factor_dev(rx, 0.0, sh)


out["factor_ms"] = timed(lambda: refactor(F))
F.factor_status(sh)

results = {}
for side in ("right", "left", "auto"):
    with F.sens_plan(B[:3], Ct[:3], side=side) as plan:
        info = plan.info
        run = lambda parts: F.debug_sens_parts(plan, parts, d_bz.data_ptr(), d_cz.data_ptr(), d_y.data_ptr(), sh)   # noqa: E731
        out[side + "_ms"] = timed(lambda: F.sens_solve_dev(plan, d_bz.data_ptr(), d_cz.data_ptr(), d_y.data_ptr(), sh))
        results[side] = d_y.cpu().numpy()
        if side == "auto":
            out["auto_side"] = "right" if info.side == sr.RIGHT else "left"
            continue
        ns = args.k if side == "right" else args.p
        tl = sr.tiles(ns, lim)
        assert info.ntiles == len(tl) and info.max_width == max(w for _, _, w in tl)
        out[side + "_tiles"] = [[t, w] for _, t, w in tl]
        trans = side == "left"                                                 # op N: inner N from the right, inner T from the left
        solves = 0.0
        for w in sorted({w for _, _, w in tl}):
            d_z = torch.zeros((2 * n, w), dtype=torch.float64, device=dev)
            d_z[torch.arange(w, device=dev) * 7 % (2 * n), torch.arange(w, device=dev)] = 1.0
            d_z0 = d_z.clone()
            t_w = timed(lambda: F.real.solve_dev(d_z.data_ptr(), w, sh, trans=trans), lambda: d_z.copy_(d_z0))
            out["%s_%d_ms" % ("solve_t" if trans else "solve", w)] = t_w
            solves += t_w * sum(1 for _, _, ww in tl if ww == w)
            del d_z, d_z0
        out[side + "_solves_ms"] = solves
        out[side + "_over_solves"] = out[side + "_ms"] / solves
        out[side + "_scatter_ms"] = timed(lambda: run(1))
        out[side + "_combine_ms"] = timed(lambda: run(4))
scale = np.abs(results["right"]).max()
out["left_vs_right_rel"] = float(np.abs(results["left"] - results["right"]).max() / scale)
out["auto_is_faster_side"] = out["auto_side"] == ("right" if out["right_ms"] <= out["left_ms"] else "left")
assert out["left_vs_right_rel"] < 1e-9 and np.array_equal(results["auto"], results[out["auto_side"]])
out["left_width"], out["real_left_width"] = args.p, 2 * args.p

# (b) what the parent commit allows: dense tiles through solve_dev, the product on the host
import scipy.sparse as sp
Bs = sp.csc_matrix((B.values, B.indices, B.indptr), shape=(n, args.k))
Cs = sp.csc_matrix((Ct.values, Ct.indices, Ct.indptr), shape=(n, args.p)).T.tocsr()
walls = []
for _ in range(args.host_reps):
    t0 = time.perf_counter()
    Y = np.empty((args.p, args.k), dtype=np.complex128)
    for c0 in range(0, args.k, lim.max_tile):
        c1 = min(args.k, c0 + lim.max_tile)
        d_t = torch.from_numpy(Bs[:, c0:c1].toarray(order="C")).to(dev)
        F.solve_dev(d_t.data_ptr(), d_t.data_ptr(), c1 - c0, sh)
        Y[:, c0:c1] = Cs @ d_t.cpu().numpy()
    walls.append((time.perf_counter() - t0) * 1e3)
out["composed_ms"] = float(np.median(walls))
out["composed_vs_right_rel"] = float(np.abs(Y - results["right"]).max() / scale)
out["composed_over_auto"] = out["composed_ms"] / out["auto_ms"]
assert out["composed_vs_right_rel"] < 1e-9
F.close()

# Kron reduction: the factorisation with ns boundary buses next to the plain one, and the read-out of S
rng = np.random.default_rng(7)
for ns in args.ns:
    border = np.sort(rng.choice(n, size=ns, replace=False)).astype(np.int32)
    with hip.ComplexFactorization(n, Ap, Ai, schur=border) as G:
        rx = G.plan.workspace_dev(0, 4 * G.nnz)
        out["kron_%d_factor_ms" % ns] = timed(lambda: refactor(G))
        G.factor_status(sh)
        d_s = torch.empty((ns, ns), dtype=torch.complex128, device=dev)
        out["kron_%d_get_ms" % ns] = timed(lambda: G.schur_dev(d_s.data_ptr(), sh))
        out["kron_%d_nnz_l_real" % ns], out["kron_%d_max_front_real" % ns] = int(G.real.info.nnz_l), int(G.real.info.max_front)
        out["kron_%d_over_plain" % ns] = out["kron_%d_factor_ms" % ns] / out["factor_ms"]
        S = d_s.cpu().numpy()
        out["kron_%d_symmetry_rel" % ns] = float(np.abs(S - S.T).max() / np.abs(S).max())      # Y-bus is symmetric: so is S

line = json.dumps({k: (float("%.4g" % v) if isinstance(v, float) and abs(v) < 1e-3 else round(v, 4) if isinstance(v, float) else v)
                   for k, v in out.items()})
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
