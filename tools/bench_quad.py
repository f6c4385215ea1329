#!/usr/bin/env python3
"""The bad-data test of a state estimate on the selected inverse against the route it replaces, one GPU, one JSON line
(median event-timed ms over --reps after warm-up).  synth.se_case at --nbus buses and --nedges branches (default 1.02 nbus,
the chord share of the ybus benchmarks: m = nbus + nedges ~ 2 n measurements.  The chords of synth._connected_graph are random,
so at nedges = 2 nbus, m ~ 3 n, the factors of the gain matrix pass the 32-bit pool offsets and cs3_analyze refuses), G = H' (W H)
through a SpgemmPlan (what CscMat.multiply_plan(transpose_self=True) makes), a Cholesky handle with the factors held, one
gross error planted, all in one process:
  * a_selinv_ms: cs3_selinv_dev;
  * b_normres_ms: cs3_quad_normres_dev alone (the forms, omega, rn, the summary: three launches);
  * c_selinv_normres_ms: (a) + (b) in one timed body;
  * d_sens_ms: the same m values t_i = h_i' G^-1 h_i by sens_solve_dev, one plan per tile of 1024 rows of H (B = the rows as
    columns, C = the rows: Y is 1024 x 1024 per tile, its diagonal is kept);
  * e_copy_ms: a device-to-device copy of the bytes of the term map (positions and row table), the traffic yardstick of (b);
  * the ratios c / d and b / e, the plan's sizes, whether the planted row is found, the max error of t against (d) on one tile.
    python tools/bench_quad.py [--reps 20] [--nbus 50000] [--nedges 51000] [--skip-sens] [--out profiles/quad_bench.json]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--nbus", type=int, default=50000)
ap.add_argument("--nedges", type=int, default=None)
ap.add_argument("--skip-sens", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream
TILE = int(hip.sens_limits().max_tile)
CRIT_TOL = 1e-8


def timed(body, warm=2):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); body(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
m, n, Hp, Hi, Hx, w, crit = synth.se_case(args.nbus, args.nedges or args.nbus + args.nbus // 50, seed=args.nbus)
nnz = int(Hp[n])
cols = np.repeat(np.arange(n), np.diff(Hp))
by_row = np.argsort(Hi, kind="stable")                       # the rows of H: a stable transpose on the host
Ct = (m, np.concatenate([[0], np.cumsum(np.bincount(Hi, minlength=m))]).astype(np.int32), cols[by_row].astype(np.int32))
Cx = Hx[by_row]
matvec = lambda x: np.bincount(Hi, weights=Hx * x[cols], minlength=m)              # H x
rmatvec = lambda y: np.bincount(cols, weights=Hx * y[Hi], minlength=n)             # H' y

gain = hip.SpgemmPlan(m, n, Hp, Hi, m, n, Hp, Hi, transpose_a=True)
Gp, Gi = gain.pattern()
d_hx, d_whx = to_dev(Hx), to_dev(Hx * w[Hi])
d_gx = torch.empty(gain.nnz, dtype=torch.float64, device=dev)
gain.values_dev(d_hx.data_ptr(), d_whx.data_ptr(), d_gx.data_ptr(), sh)
F = hip.Factorization(n, n, Gp, Gi, hip.CS3_CHOLESKY)
F.factor_dev(d_gx.data_ptr(), 0.0, sh)
F.factor_status(sh)

rng = np.random.default_rng(1)
bad = int(np.flatnonzero(np.diff(Ct[1]) > 2)[7])             # an injection row
z = matvec(rng.standard_normal(n)) + rng.standard_normal(m) / np.sqrt(w)
z[bad] += 40.0 / np.sqrt(w[bad])
r = z - matvec(F.solve(rmatvec(w * z)))

plan = F.quad_plan(Ct)
info = plan.info
d_cx, d_w, d_r = to_dev(Cx), to_dev(w), to_dev(r)
d_t, d_omega, d_rn = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(3))
d_sum = torch.empty(4, dtype=torch.float64, device=dev)
normres = lambda: F.normalized_residuals_dev(plan, d_cx.data_ptr(), d_w.data_ptr(), d_r.data_ptr(), CRIT_TOL, d_sum.data_ptr(),
                                             d_t.data_ptr(), d_omega.data_ptr(), d_rn.data_ptr(), sh)


def both():
    F.selinv(sh)
    normres()


F.selinv(sh)
map_bytes = int(info.nterms) * 8 + m * 32
src, dst = (torch.empty(map_bytes, dtype=torch.uint8, device=dev) for _ in range(2))
out = {"reps": args.reps, "nbus": n, "nedges": m - (n - len(crit)), "m": m, "nnz_h": nnz, "nnz_g": gain.nnz, "nterms": int(info.nterms),
       "rows_lane": int(info.rows_lane), "rows_wave": int(info.rows_wave), "rows_workgroup": int(info.rows_workgroup),
       "term_map_mbytes": map_bytes / 1e6,
       "a_selinv_ms": timed(lambda: F.selinv(sh)), "b_normres_ms": timed(normres), "c_selinv_normres_ms": timed(both),
       "e_copy_ms": timed(lambda: dst.copy_(src))}
out["b_over_e"] = out["b_normres_ms"] / out["e_copy_ms"]
summary = d_sum.cpu().numpy()
out.update(worst=float(summary[0]), worst_row=int(summary[1]), planted_row=bad, J=float(summary[2]), critical=int(summary[3]),
           designed_critical=len(crit))

if not args.skip_sens:
    tiles = [(r0, min(TILE, m - r0)) for r0 in range(0, m, TILE)]
    plans, vals = [], []
    for r0, t in tiles:                                     # B = rows r0 .. r0 + t of H as columns, C = the same rows
        lo, hi = int(Ct[1][r0]), int(Ct[1][r0 + t])
        rows = (t, (Ct[1][r0:r0 + t + 1] - lo).astype(np.int32), Ct[2][lo:hi])
        plans.append(F.sens_plan(rows, rows, side="right"))
        vals.append(d_cx[lo:hi])
    d_y = torch.empty((TILE, TILE), dtype=torch.float64, device=dev)
    d_sens = torch.empty(m, dtype=torch.float64, device=dev)

    def sens_route():
        for (r0, t), sp, v in zip(tiles, plans, vals):
            F.sens_solve_dev(sp, v.data_ptr(), v.data_ptr(), d_y.data_ptr(), sh)
            d_sens[r0:r0 + t] = d_y.view(-1)[:t * t].view(t, t).diagonal()

    out["d_sens_ms"] = timed(sens_route, warm=1)
    out["sens_tiles"] = len(tiles)
    out["c_over_d"] = out["c_selinv_normres_ms"] / out["d_sens_ms"]
    r0, t = tiles[len(tiles) // 2]
    got, want = d_t[r0:r0 + t].cpu().numpy(), d_sens[r0:r0 + t].cpu().numpy()
    out["max_err_vs_sens_on_one_tile"] = float(np.abs(got - want).max() / np.abs(want).max())
    for sp in plans:
        sp.close()
plan.close()
F.close()
gain.close()

print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
