#!/usr/bin/env python3
"""Complex matrices through the real-equivalent plan: a Y-bus of 50 000 buses (synth.ybus) on one GPU -- the values
launches alone, pack + unpack at 1 and 128 right-hand sides, the whole step ComplexFactorization.factor_solve_dev at one
right-hand side -- and, in the same visit, the same step on the real config-3 matrix of bench.py (synth.grid_jacobian,
50 000 unknowns).  Every leg in this process, event-timed, median of --reps.  Writes profiles/cplx_bench.json.
    python tools/bench_cplx.py [--nbus 50000] [--nedges 51000] [--reps 20]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from csparse3_amd import csc_hip as hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("--nbus", type=int, default=50000)
ap.add_argument("--nedges", type=int, default=51000, help="49 999 tree branches + chords: at 51 000 the real form has about the fill of config 3")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cplx_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
TOL = 1e-3


def median_ms(fn):
    """Median over args.reps of the device time of fn(), between two events on the current stream."""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


out = {"nbus": args.nbus, "nedges": args.nedges, "reps": args.reps, "tol": TOL}

# ---- the complex leg
n, Ap, Ai, Az = synth.ybus(args.nbus, args.nedges, seed=args.nbus)
nnz = int(Ap[n])
rng = np.random.default_rng(1)
b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
with hip.ComplexFactorization(n, Ap, Ai) as F:
    inf = F.real.info
    out.update({"n": n, "nnz": nnz, "n_real": int(inf.n), "nnz_real": 4 * nnz, "nnz_l_real": int(inf.nnz_l), "nnz_u_real": int(inf.nnz_u),
                "nsuper_real": int(inf.nsuper), "nlevels_real": int(inf.nlevels), "max_front_real": int(inf.max_front),
                "factor_bytes_real": int(inf.factor_bytes), "analysis_s_real": float(inf.t_order_s + inf.t_symbolic_s)})
    with hip.Factorization(n, n, Ap, Ai) as Fc:                      # the complex pattern itself, analysed only: what a native kernel family would see
        ic = Fc.info
        out.update({"nnz_l_pattern": int(ic.nnz_l), "nsuper_pattern": int(ic.nsuper), "nlevels_pattern": int(ic.nlevels),
                    "max_front_pattern": int(ic.max_front), "factor_bytes_pattern_as_real": int(ic.factor_bytes)})
    d_az, d_b = torch.from_numpy(Az).to(dev), torch.from_numpy(b).to(dev)
    d_x = torch.empty_like(d_b)
    d_rx = torch.empty(4 * nnz, dtype=torch.float64, device=dev)
    F.plan.upload()
    out["values_us"] = 1e3 * median_ms(lambda: F.plan.values_dev(d_az.data_ptr(), d_rx.data_ptr(), st))
    out["values_bytes"] = int(nnz * (16 + 32 + 8) + n * 16)         # values in, blocks out, row and column of every entry; s
    src = d_rx.clone()
    out["values_copy_us"] = 1e3 * median_ms(lambda: d_rx.copy_(src))  # a device-to-device copy of the same output
    for k in (1, 128):
        d_z = torch.from_numpy(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))).to(dev)
        d_y = torch.empty((2 * n, k), dtype=torch.float64, device=dev)

        def pack_unpack():
            F.plan.pack_dev(d_z.data_ptr(), d_y.data_ptr(), k, "N", st)
            F.plan.unpack_dev(d_y.data_ptr(), d_z.data_ptr(), k, "N", False, st)
        out["pack_unpack_k%d_us" % k] = 1e3 * median_ms(pack_unpack)
        out["pack_unpack_k%d_bytes" % k] = int(n * k * 64 + 2 * n * 16)
        del d_z, d_y
    out["complex_step_ms"] = median_ms(lambda: F.factor_solve_dev(d_az.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 1, TOL, st))
    F.factor_status(st)
    rx, y, x2 = F._workspace(1)
    out["complex_step_handle_only_ms"] = median_ms(lambda: F.real.factor_solve_bx_dev(rx, y, x2, 1, TOL, st))
    F.factor_status(st)
    x = d_x.cpu().numpy()
    r = F.residual(Az, b, x)
    col = np.repeat(np.arange(n), np.diff(Ap))
    norm1 = np.bincount(col, weights=np.abs(Az), minlength=n).max()
    out["complex_scaled_residual"] = float(np.abs(r).max() / (norm1 * np.abs(x).max() + np.abs(b).max()))

# ---- the real leg: bench.py's config 3, the same call
m, nr, Rp, Ri, Rx = synth.grid_jacobian(n=50000, seed=50000)
br = synth.grid_rhs(nr, 1, seed=1024)
with hip.Factorization(m, nr, Rp, Ri, hip.CS3_LU, hip.ORDER_AMD) as R:
    inf = R.info
    out.update({"real_n": nr, "real_nnz": int(Rp[nr]), "real_nnz_l": int(inf.nnz_l), "real_nsuper": int(inf.nsuper),
                "real_nlevels": int(inf.nlevels), "real_max_front": int(inf.max_front), "real_factor_bytes": int(inf.factor_bytes)})
    d_ax, d_br = torch.from_numpy(Rx).to(dev), torch.from_numpy(br).to(dev)
    d_xr = torch.empty_like(d_br)
    out["real_step_ms"] = median_ms(lambda: R.factor_solve_bx_dev(d_ax.data_ptr(), d_br.data_ptr(), d_xr.data_ptr(), 1, TOL, st))
    R.factor_status(st)
out["complex_over_real"] = out["complex_step_ms"] / out["real_step_ms"]

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
