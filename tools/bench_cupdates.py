#!/usr/bin/env python3
"""Complex low-rank-modified solves against what they are made of and against what the library allowed before, one GPU,
one JSON line, also written to profiles/cupdates_bench.json (median event-timed ms over --reps after warm-up).
synth.ybus(--n, --n + --cases + 1), rotated LU, factors held, --cases chord outages (branches outside a spanning tree:
none of them islands a bus):
  * cupdates_ms: one ComplexFactorization.solve_updates_dev of the whole list, and per case;
  * solves_ms: the plain solves it is made of -- one k = 1 and one per tile at the tile's width on [2n, w] -- and the
    ratio call / solves (the real path's is 1.185 on its own workload);
  * parts_units_ms (pack + the k = 1 solve + k_cupd_units, from which solve_1_ms is subtracted) and parts_cap_apply_ms
    (k_cupd_capacitance + k_cupd_apply) through the debug call; apply_bytes (Z read once + X written once) over
    parts_cap_apply_ms is a LOWER bound of k_cupd_apply's rate (the capacitance kernel's time is inside);
  * comparator (a), real_route_*: the real plan on F.real -- s read back to the host, every 2 x 2 block of diag(s) dA
    rotated there, twice the columns -- as host preparation ms and device ms;
  * comparator (b), refactor_ms_per_case: values edited in HBM + factor_solve_dev per case, over --refactor-cases cases,
    and the whole list priced from it.
Both comparators run code this path does not touch.
    python tools/bench_cupdates.py [--reps 20] [--cases 1000]"""
import argparse, json, os, sys, time
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--cases", type=int, default=1000)
ap.add_argument("--refactor-cases", type=int, default=64)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cupdates_bench.json"))
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


n, Ap, Ai, Az = synth.ybus(args.n, args.n + args.cases + 1, seed=args.n)
A = sp.csc_matrix((Az, Ai, Ap), shape=(n, n))
upper = sp.triu(A, k=1).tocoo()
tree = csgraph.breadth_first_tree(sp.csr_matrix((np.ones(A.nnz), Ai, Ap), shape=(n, n)), 0, directed=False).tocoo()
in_tree = set(zip(np.minimum(tree.row, tree.col).tolist(), np.maximum(tree.row, tree.col).tolist()))
chords = [(int(i), int(j)) for i, j in zip(upper.row, upper.col) if (int(i), int(j)) not in in_tree][:args.cases]
cases = [(np.array([i, j, i, j]), np.array([j, i, i, j]), np.array([-A[i, j], -A[j, i], A[i, j], A[j, i]])) for i, j in chords]
b = np.random.default_rng(0).standard_normal(n) + 1j * np.random.default_rng(1).standard_normal(n)
d_b = torch.from_numpy(b.copy()).to(dev)
out = {"n": n, "nnz": int(Ap[n]), "cases": len(cases)}
F = hip.ComplexFactorization(n, Ap, Ai)
F.factor(Az)

# ---- this path
pattern = [(c[0], c[1]) for c in cases]
cz = np.concatenate([c[2] for c in cases])
d_cz = torch.from_numpy(cz.copy()).to(dev)
plan = F.updates_plan(pattern)
info, tiles = plan.info, plan.tiles()
out.update(rows_unique=info.nrows_unique, tiles=[[int(v) for v in t] for t in tiles])
d_X = torch.empty((n, len(cases)), dtype=torch.complex128, device=dev)
d_r = torch.empty(len(cases), dtype=torch.float64, device=dev)
call = lambda parts=None: (F.solve_updates_dev(plan, d_cz.data_ptr(), d_b.data_ptr(), d_X.data_ptr(), d_r.data_ptr(), 1e-10, sh)    # noqa: E731
                           if parts is None else
                           F.debug_updates_parts(plan, parts, d_cz.data_ptr(), d_b.data_ptr(), d_X.data_ptr(), d_r.data_ptr(), 1e-10, sh))
out["cupdates_ms"] = timed(call)
out["cupdates_us_per_case"] = 1e3 * out["cupdates_ms"] / len(cases)
X = d_X.cpu().numpy()
assert np.isfinite(X.view(np.float64)).all() and float(d_r.min()) > 1e-6
k = len(cases) // 2                                                 # one case against a sparse direct solve of the modified matrix
import scipy.sparse.linalg as spla
dA = sp.coo_matrix((cases[k][2], (cases[k][0], cases[k][1])), shape=(n, n))
want = spla.splu((A + dA).tocsc()).solve(b)
out["check_rel_err"] = float(np.abs(X[:, k] - want).max() / np.abs(want).max())
d_y = torch.empty(2 * n, dtype=torch.float64, device=dev)
d_y0 = torch.from_numpy(F.plan.pack(b)).to(dev)
solves = timed(lambda: F.real.solve_dev(d_y.data_ptr(), 1, sh), lambda: d_y.copy_(d_y0))
out["solve_1_ms"] = solves
for w in sorted(set(int(t[3]) for t in tiles)):
    d_Z = torch.zeros((2 * n, w), dtype=torch.float64, device=dev)
    d_Z[2 * (torch.arange(w, device=dev) * 7 % n), torch.arange(w, device=dev)] = 1.0
    d_Z0 = d_Z.clone()
    t_w = timed(lambda: F.real.solve_dev(d_Z.data_ptr(), w, sh), lambda: d_Z.copy_(d_Z0))
    out["solve_%d_ms" % w] = t_w
    solves += t_w * sum(1 for t in tiles if int(t[3]) == w)
    del d_Z, d_Z0
out["solves_ms"] = solves
out["cupdates_over_solves"] = out["cupdates_ms"] / solves
out["parts_units_ms"] = timed(lambda: call(1)) - out["solve_1_ms"]
call()                                                               # (a solved tile in the buffer for the next leg)
out["parts_cap_apply_ms"] = timed(lambda: call(4))
out["apply_bytes"] = int(sum(16 * n * (int(t[3]) + int(t[1])) for t in tiles))
out["units_bytes"] = int(sum(16 * n * int(t[3]) for t in tiles))
out["apply_TBps_lower_bound"] = out["apply_bytes"] / (out["parts_cap_apply_ms"] * 1e-3) / 1e12
plan.close()

# ---- comparator (a): the real plan on F.real, s read back, blocks rotated on the host
t0 = time.perf_counter()
s = F.plan.rotation()[0]
real_cases = []
for rows, cols, vals in cases:
    w = s[rows] * vals
    real_cases.append((np.concatenate([2 * rows, 2 * rows, 2 * rows + 1, 2 * rows + 1]),
                       np.concatenate([2 * cols, 2 * cols + 1, 2 * cols, 2 * cols + 1]),
                       np.concatenate([w.real, -w.imag, w.imag, w.real])))
cx = np.concatenate([c[2] for c in real_cases])
d_cx = torch.from_numpy(cx).to(dev)
torch.cuda.synchronize()
out["real_route_host_ms"] = 1e3 * (time.perf_counter() - t0)
rplan = F.real.updates_plan([(c[0], c[1]) for c in real_cases])
out["real_route_tiles"] = [[int(v) for v in t] for t in rplan.tiles()]
d_XR = torch.empty((2 * n, len(cases)), dtype=torch.float64, device=dev)
out["real_route_ms"] = timed(lambda: F.real.solve_updates_dev(rplan, d_cx.data_ptr(), d_y0.data_ptr(), d_XR.data_ptr(), d_r.data_ptr(), 1e-10, sh))
XR = d_XR.cpu().numpy()
out["real_route_max_diff"] = float(np.abs(XR[0::2] + 1j * XR[1::2] - X).max() / np.abs(X).max())
out["real_route_over_cupdates"] = out["real_route_ms"] / out["cupdates_ms"]
rplan.close()
del d_XR

# ---- comparator (b): values edited in HBM + factor_solve_dev per case
cols_of = np.repeat(np.arange(n), np.diff(Ap))
pos = {}
for c in cases[:args.refactor_cases]:
    for i, j in zip(c[0], c[1]):
        p = Ap[j] + int(np.searchsorted(Ai[Ap[j]:Ap[j + 1]], i))
        assert Ai[p] == i and cols_of[p] == j
        pos[(int(i), int(j))] = p
d_az0 = torch.from_numpy(np.asarray(Az).copy()).to(dev)
d_az = d_az0.clone()
d_x = torch.empty(n, dtype=torch.complex128, device=dev)
edits = [(torch.tensor([pos[(int(i), int(j))] for i, j in zip(c[0], c[1])], device=dev), torch.from_numpy(np.asarray(c[2])).to(dev))
         for c in cases[:args.refactor_cases]]


def refactor_all():
    for idx, val in edits:
        d_az.copy_(d_az0)
        d_az.index_add_(0, idx, val)
        F.factor_solve_dev(d_az.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, 0.0, sh)


per_case = timed(refactor_all, reps=5, warm=1) / len(edits)
F.factor_status(sh)
out["refactor_ms_per_case"] = per_case
out["refactor_ms_whole_list"] = per_case * len(cases)
out["refactor_over_cupdates"] = out["refactor_ms_whole_list"] / out["cupdates_ms"]
F.close()
line = json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in out.items()})
with open(args.out, "w") as f:
    f.write(line + "\n")
print(line)
