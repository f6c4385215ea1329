#!/usr/bin/env python3
"""Sparse products on one GPU, one JSON line per product and long-list threshold (median over --reps after a warm-up):
  * G = H' H with H = the config-3 Jacobian (synth.grid_jacobian()), through a transpose_a plan, and J J of the same matrix;
  * plan_ms: SpgemmPlan creation (host validation, uploads, symbolic product on the device), wall clock;
  * values_dev_ms: one refresh of the values on resident arrays, event-timed;
  * oneshot_ms: csc_multiply_ff from host arrays (plan + pattern download + values + free), wall clock;
  * scipy_ms: SciPy's A @ B on the same host, one thread, wall clock -- the product a caller would form today;
  * values_bytes: the algorithmic traffic of the numeric pass, 8 B per pair read (padding included: padded_pairs),
    16 B per product gathered, 8 B per entry of C written; values_gbs = values_bytes / values_dev_ms;
  * --long: long-list thresholds to build the plan with (CS3_SPGEMM_LONG), to place the threshold by measurement;
  * --lists K ...: instead of the above, the sweep that places the threshold (list_length_sweep below).
    python tools/bench_spgemm.py [--reps 20] [--n 50000] [--long 32 128 512] | --lists 16 32 64 128 256 512"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import scipy.sparse as sp
from csparse3_amd import csc_hip as hip, synth
from helpers import csc_to_scipy

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--long", type=int, nargs="+", default=[0])
ap.add_argument("--lists", type=int, nargs="*", default=[])
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


def wall(body, reps, warm=1):
    for _ in range(warm):
        body()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); body(); t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def list_length_sweep():
    """Where should "long" begin?  C = A B with A 1024 x K, B K x 64 dense in CSC form, so that C has 65536 entries in 1024
    slices.  "uniform": every list has K pairs (the sliced path at its best: no padding).  "one_in_64": every row has an
    entry in column 0 of A and only the rows 0, 64, 128, ... have the others, so every slice holds ONE list of K pairs among
    63 lists of one.  Each is timed with the threshold above K (all lists in their slices) and at K (the long ones leave)."""
    rows, ncol = 1024, 64
    for K in args.lists:
        for shape in ("uniform", "one_in_64"):
            tail = np.arange(rows, dtype=np.int32) if shape == "uniform" else np.arange(0, rows, 64, dtype=np.int32)
            cols = [np.arange(rows, dtype=np.int32)] + [tail] * (K - 1)
            Ap = np.zeros(K + 1, dtype=np.int32); Ap[1:] = np.cumsum([len(c) for c in cols])
            Ai = np.concatenate(cols)
            Bp = (np.arange(ncol + 1) * K).astype(np.int32); Bi = np.tile(np.arange(K, dtype=np.int32), ncol)
            rng = np.random.default_rng(K)
            d_ax, d_bx = torch.from_numpy(rng.standard_normal(Ai.size)).to(dev), torch.from_numpy(rng.standard_normal(Bi.size)).to(dev)
            out = dict(sweep=shape, K=K, entries=rows * ncol)
            for label, L in (("sliced_ms", K + 1), ("long_ms", K)):
                os.environ["CS3_SPGEMM_LONG"] = str(L)
                with hip.SpgemmPlan(rows, K, Ap, Ai, K, ncol, Bp, Bi) as plan:
                    inf = plan.info
                    assert inf.entries_long == (0 if L > K else (rows * ncol if shape == "uniform" else rows * ncol // 64))
                    d_cx = torch.empty(plan.nnz, dtype=torch.float64, device=dev)
                    out[label] = timed(lambda: plan.values_dev(d_ax.data_ptr(), d_bx.data_ptr(), d_cx.data_ptr(), sh))
                    out[label.replace("_ms", "_padded")] = int(inf.padded_pairs)
                    out["products"] = int(inf.products)
            os.environ.pop("CS3_SPGEMM_LONG", None)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


if args.lists:
    list_length_sweep()
    sys.exit(0)

m, n, Ap, Ai, Ax = synth.grid_jacobian(n=args.n) if args.n != 50000 else synth.grid_jacobian()
J = csc_to_scipy(m, n, Ap, Ai, Ax)
H = J
arr = lambda M: (M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))   # noqa: E731
products = {"HtH": (arr(H), arr(H), True, lambda: H.T.tocsc() @ H), "JJ": (arr(J), arr(J), False, lambda: J @ J)}

for name, (A, B, ta, scipy_body) in products.items():
    scipy_ms = wall(scipy_body, 5)
    want = scipy_body().tocsc()
    for L in args.long:
        if L:
            os.environ["CS3_SPGEMM_LONG"] = str(L)
        else:
            os.environ.pop("CS3_SPGEMM_LONG", None)
        make = lambda: hip.SpgemmPlan(A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3], transpose_a=ta)   # noqa: E731
        plan_ms = wall(lambda: make().close(), 5)
        out = dict(product=name, n=n, rows_a=A[0], nnz_a=int(A[2][-1]), nnz_b=int(B[2][-1]), scipy_ms=scipy_ms, plan_ms=plan_ms)
        with make() as plan:
            inf = plan.info
            d_ax, d_bx = torch.from_numpy(A[4]).to(dev), torch.from_numpy(B[4]).to(dev)
            d_cx = torch.empty(max(plan.nnz, 1), dtype=torch.float64, device=dev)
            out["values_dev_ms"] = timed(lambda: plan.values_dev(d_ax.data_ptr(), d_bx.data_ptr(), d_cx.data_ptr(), sh))
            nbytes = 8 * int(inf.padded_pairs) + 16 * int(inf.products) + 8 * int(inf.nnz_c)
            out.update(long_list=int(inf.long_list), nnz_c=int(inf.nnz_c), products=int(inf.products),
                       padded_pairs=int(inf.padded_pairs), entries_long=int(inf.entries_long), cols_lds=int(inf.cols_lds),
                       cols_global=int(inf.cols_global), values_bytes=nbytes, values_gbs=nbytes / out["values_dev_ms"] / 1e6)
            Cp, Ci = plan.pattern()
            got = sp.csc_matrix((d_cx.cpu().numpy()[:plan.nnz], Ci, Cp), shape=(plan.m, plan.n))
            out["rel_diff_vs_scipy"] = float(abs(got - want).max() / abs(want).max())
        A1 = arr(sp.csc_matrix((A[4], A[3], A[2]), shape=A[:2]).T.tocsc()) if ta else A      # the one-shot call takes A' itself
        out["oneshot_ms"] = wall(lambda: hip.csc_multiply_ff(*A1, *B), 5)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
