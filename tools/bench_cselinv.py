#!/usr/bin/env python3
"""diag(Z-bus), the entries of Z-bus on the pattern of Y-bus and the Thevenin table of all branches from the selected
inverse of the real form, against the route that existed before: one GPU, one JSON line (median event-timed ms over
--reps after warm-up; a short call is issued --inner times between its two events and the time divided).  The matrix is
synth.ybus at --n buses with --edges branches (the one tools/bench_csens.py uses), LU with the rotation, factors held:
  * selinv_ms: cs3_selinv_dev on the real form (order 2 n);
  * entries_ms / entries_t_ms / diag_ms / thevenin_ms: one getter each, ZR held;
  * selinv_diag_ms: selinv + the diagonal getter, timed together, the n driving-point impedances from held factors;
  * sens_diag_ms: the same n entries by ComplexFactorization.sens_solve_dev with unit columns, one plan per tile of 1024
    buses (Y = E' A^-1 E is 1024 x 1024 per tile, its diagonal is kept), and the ratio to selinv_diag_ms;
  * factor_ms: values + one factorisation of the real form, for scale;
  * *_mbytes: what one call of a getter reads and writes, computed from the shapes.  No rate is derived from it: at this
    size a getter takes a few microseconds, the cost of a launch, and --inner repeated calls find their tables in cache;
  * diag_vs_sens_rel: the largest difference of the two routes' diagonals relative to max |Z_ii|.
    python tools/bench_cselinv.py [--reps 20] [--n 50000] [--skip-sens] [--out profiles/cselinv_bench.json]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--edges", type=int, default=None, help="branches; default n + n / 50")
ap.add_argument("--skip-sens", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if hip.device_count() < 1:
    sys.exit("bench_cselinv.py needs a GPU: nothing here is measured without one")
dev = torch.device("cuda", 0)
sh = torch.cuda.current_stream().cuda_stream
TILE = int(hip.cplx_sens_limits().max_tile)


def timed(body, warm=2, inner=1):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for _ in range(warm):
        body()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        for _ in range(inner):
            body()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) / inner


edges = args.edges if args.edges is not None else args.n + args.n // 50
n, Ap, Ai, Az = synth.ybus(args.n, edges, seed=args.n)
nnz = int(Ap[n])
out = {"n": n, "edges": edges, "nnz": nnz, "reps": args.reps, "inner": args.inner}
F = hip.ComplexFactorization(n, Ap, Ai)
d_az = torch.from_numpy(Az).to(dev)
rx = F.plan.workspace_dev(0, 4 * F.nnz)


def refactor():
    F.plan.values_dev(d_az.data_ptr(), rx, sh)
    F.real.factor_dev(rx, 0.0, sh)


out["factor_ms"] = timed(refactor)
F.factor_status(sh)
info = F.real.selinv_info()
out.update(nnz_l_real=int(F.real.info.nnz_l), max_front_real=int(F.real.info.max_front), selinv_launches=int(info.nlaunches),
           zpool_mbytes=info.zpool_doubles * 8 / 1e6)
d_e, d_t, d_th = (torch.empty(nnz, dtype=torch.complex128, device=dev) for _ in range(3))
d_d = torch.empty(n, dtype=torch.complex128, device=dev)

out["selinv_ms"] = timed(lambda: F.selinv(sh))
getters = {"entries": lambda: F.inverse_entries_dev(d_e.data_ptr(), False, sh), "entries_t": lambda: F.inverse_entries_dev(d_t.data_ptr(), True, sh),
           "diag": lambda: F.inverse_diagonal_dev(d_d.data_ptr(), sh), "thevenin": lambda: F.thevenin_dev(d_th.data_ptr(), sh)}
# bytes per output number: the map pair, the index pair (entries, Thevenin), s, the reads of ZR, the store
moved = {"entries": nnz * (16 + 8 + 16 + 16 + 16), "entries_t": nnz * (16 + 8 + 16 + 16 + 16), "diag": n * (16 + 16 + 16 + 16),
         "thevenin": nnz * (2 * 16 + 8 + 2 * 16 + 2 * 16 + 8 * 8 + 16)}
for name, call in getters.items():
    out[name + "_ms"] = timed(call, inner=args.inner)
    out[name + "_mbytes"] = moved[name] / 1e6


def selinv_diag():
    F.selinv(sh)
    F.inverse_diagonal_dev(d_d.data_ptr(), sh)


out["selinv_diag_ms"] = timed(selinv_diag)
out["selinv_over_factor"] = out["selinv_ms"] / out["factor_ms"]
selinv_diag()
torch.cuda.synchronize()
diag = d_d.cpu().numpy()
assert np.array_equal(diag, F.inverse_diagonal())                      # the host form: the same bits

if not args.skip_sens:
    tiles = [(c0, min(TILE, n - c0)) for c0 in range(0, n, TILE)]
    plans = []
    for c0, t in tiles:                                   # B = columns c0 .. c0 + t of I, C = the same rows of I
        unit = (t, np.arange(t + 1, dtype=np.int32), np.arange(c0, c0 + t, dtype=np.int32))
        plans.append(F.sens_plan(unit, unit, side="right"))
    ones = torch.ones(TILE, dtype=torch.complex128, device=dev)
    d_y = torch.empty((TILE, TILE), dtype=torch.complex128, device=dev)
    d_sens = torch.empty(n, dtype=torch.complex128, device=dev)

    def sens_diag():
        for (c0, t), plan in zip(tiles, plans):
            F.sens_solve_dev(plan, ones.data_ptr(), ones.data_ptr(), d_y.data_ptr(), sh)
            d_sens[c0:c0 + t] = d_y.view(-1)[:t * t].view(t, t).diagonal()

    out["sens_diag_ms"] = timed(sens_diag, warm=1)
    out["sens_tiles"] = len(tiles)
    out["sens_over_selinv_diag"] = out["sens_diag_ms"] / out["selinv_diag_ms"]
    want = d_sens.cpu().numpy()
    out["diag_vs_sens_rel"] = float(np.abs(diag - want).max() / np.abs(want).max())
    assert out["diag_vs_sens_rel"] < 1e-9
    for plan in plans:
        plan.close()
F.close()

line = json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in out.items()})
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
        f.write(json.dumps(json.loads(line), indent=1) + "\n")
