#!/usr/bin/env python3
"""AC power flow on the device (csparse3_amd.csc_hip.PowerFlowPlan): the whole Newton solve, one iteration of it against
the one cs3_factor_solve_dev (k = 1) it is made of -- on the same handle and values --, the new kernels alone, and a SciPy
(SuperLU) Newton on the host as the comparator.  Event-timed, median of --reps, one GPU.  Writes profiles/powerflow_bench.json.

Case A: synth.ybus(50 000, 51 001, seed 50 000), 5 000 PV buses, one scenario.  Case B: ybus(5 000, 5 100, seed 5 000), 500 PV
buses, 64 scenarios.  A scenario's injections are PLANTED: the base profile (vm ~ U(0.97, 1.03), va ~ U(-0.1, 0.1)) moved by
dva at pvpq and dvm at pq; the start is the base profile.  (These near-tree networks cannot carry an imbalance to one
reference bus: a flat start, or injections scaled or perturbed themselves, diverge.)  The tool refuses to report a case
whose SciPy Newton does not converge, or takes another number of iterations than the device on the same scenarios.
    python tools/bench_powerflow.py [--cases A B] [--reps 20]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch
from csparse3_amd import csc_hip as hip, synth

CASES = {"A": dict(nbus=50000, nedges=51001, seed=50000, npv=5000, batch=1, dva=0.005, dvm=0.002),
         "B": dict(nbus=5000, nedges=5100, seed=5000, npv=500, batch=64, dva=0.02, dvm=0.01)}
TOL, MAX_ITERS = 1e-8, 20

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["A", "B"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "powerflow_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)


def median_ms(fn, before=None):
    """Median over args.reps of the device time of fn(), between two events on the current stream."""
    for _ in range(3):
        if before: before()
        fn()
    ts = []
    for _ in range(args.reps):
        if before: before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def build(c):
    n, Yp, Yi, Yz = synth.ybus(c["nbus"], c["nedges"], c["seed"])
    rng = np.random.default_rng(c["seed"] + 7)
    vm0, va0 = rng.uniform(0.97, 1.03, size=n), rng.uniform(-0.1, 0.1, size=n)
    va0[0] = 0.0
    pv = np.sort(rng.choice(np.arange(1, n), size=c["npv"], replace=False)).astype(np.int32)
    is_pq = np.ones(n, dtype=bool)
    is_pq[0] = False
    is_pq[pv] = False
    pq = np.flatnonzero(is_pq).astype(np.int32)
    pvpq = np.concatenate([pv, pq])
    S = np.empty((c["batch"], n), dtype=np.complex128)
    for b in range(c["batch"]):
        vm, va = vm0.copy(), va0.copy()
        va[pvpq] += rng.uniform(-c["dva"], c["dva"], size=len(pvpq))
        vm[pq] += rng.uniform(-c["dvm"], c["dvm"], size=len(pq))
        S[b] = synth.pf_planted(n, Yp, Yi, Yz, vm, va)
    return dict(n=n, Yp=Yp, Yi=Yi, Yz=Yz, pv=pv, pq=pq, S=S, vm0=vm0, va0=va0)


def scipy_newton(k, S):
    """The textbook polar Newton (dSbus_dV, the four blocks, SuperLU) for one scenario.  -> (iterations or None, seconds)."""
    n, pv, pq = k["n"], k["pv"], k["pq"]
    Y = sp.csc_matrix((k["Yz"], k["Yi"], k["Yp"]), shape=(n, n))
    pvpq = np.concatenate([pv, pq])
    vm, va = k["vm0"].copy(), k["va0"].copy()
    t0 = time.perf_counter()
    for it in range(MAX_ITERS + 1):
        V = vm * np.exp(1j * va)
        I = Y @ V
        mis = V * np.conj(I) - S
        F = np.concatenate([mis[pvpq].real, mis[pq].imag])
        if not np.isfinite(F).all():
            return None, time.perf_counter() - t0
        if np.abs(F).max() <= TOL:
            return it, time.perf_counter() - t0
        dV, dI, dVn = sp.diags(V), sp.diags(I), sp.diags(V / vm)
        dS_dva = 1j * dV @ np.conj(dI - Y @ dV)
        dS_dvm = dV @ np.conj(Y @ dVn) + np.conj(dI) @ dVn
        J = sp.bmat([[dS_dva[pvpq][:, pvpq].real, dS_dvm[pvpq][:, pq].real],
                     [dS_dva[pq][:, pvpq].imag, dS_dvm[pq][:, pq].imag]], format="csc")
        dx = spla.splu(J).solve(-F)
        va[pvpq] += dx[:len(pvpq)]
        vm[pq] += dx[len(pvpq):]
    return None, time.perf_counter() - t0


out = {"reps": args.reps, "tol": TOL, "limits": {f: int(getattr(hip.pf_limits(), f)) for f in ("block", "grid_cap", "wave_row")}}
for name in args.cases:
    c = CASES[name]
    k = build(c)
    batch, n = c["batch"], k["n"]
    its, secs = zip(*[scipy_newton(k, k["S"][b]) for b in range(min(batch, 4))])
    if any(i is None for i in its):
        sys.exit("case %s: the SciPy Newton does not converge: nothing to report" % name)
    r = {"n": n, "npv": c["npv"], "batch": batch, "scipy_iters": list(its), "scipy_s_per_scenario": float(np.median(secs))}
    t0 = time.perf_counter()
    plan = hip.PowerFlowPlan(n, k["Yp"], k["Yi"], k["pv"], k["pq"], batch=batch)
    r["plan_s"] = time.perf_counter() - t0
    inf, fz = plan.info, plan.factorization
    r.update(nnz_y=int(inf.nnz_y), nj=int(inf.nj), nnz_j=int(inf.nnz_j), rows_wave=int(inf.rows_wave), max_row=int(inf.max_row))
    st = torch.cuda.current_stream().cuda_stream
    yz = torch.from_numpy(k["Yz"].view(np.float64).copy()).to(dev)
    s = torch.from_numpy(k["S"].view(np.float64).copy()).to(dev)
    vm0 = torch.from_numpy(np.tile(k["vm0"], (batch, 1))).to(dev)
    va0 = torch.from_numpy(np.tile(k["va0"], (batch, 1))).to(dev)
    vm, va = vm0.clone(), va0.clone()
    restart = lambda: (vm.copy_(vm0), va.copy_(va0))                 # noqa: E731
    res = {}
    def solve():
        res.update(plan.solve_dev(yz.data_ptr(), s.data_ptr(), vm.data_ptr(), va.data_ptr(), tol=TOL, max_iters=MAX_ITERS, stream=st))
    r["solve_ms"] = median_ms(solve, restart)
    if not (res["flag"] == 0).all():
        sys.exit("case %s: the device Newton does not converge: flags %s" % (name, res["flag"]))
    r["iters"] = [int(res["iters"].min()), int(res["iters"].max())]
    r["iters_of_scipy_scenarios"] = [int(i) for i in res["iters"][:len(its)]]
    if r["iters_of_scipy_scenarios"] != list(its):
        sys.exit("case %s: the device Newton takes %s iterations where the SciPy Newton takes %s on the same scenarios: nothing to report"
                 % (name, r["iters_of_scipy_scenarios"], list(its)))
    r["ms_per_iteration"] = r["solve_ms"] / int(res["iters"].max())
    # one Newton step by hand at the start, leg by leg: the kernels alone, and the factor + solve the step is made of
    f = torch.empty(batch * plan.nj, dtype=torch.float64, device=dev)
    nr = torch.empty(batch, dtype=torch.float64, device=dev)
    jx = torch.empty(batch * plan.nnz_j, dtype=torch.float64, device=dev)
    mis = lambda: plan.mismatch_dev(yz.data_ptr(), s.data_ptr(), vm0.data_ptr(), va0.data_ptr(), f.data_ptr(), nr.data_ptr(), st)   # noqa: E731
    jac = lambda: plan.jacobian_dev(yz.data_ptr(), vm0.data_ptr(), va0.data_ptr(), jx.data_ptr(), st)                             # noqa: E731
    r["mismatch_us"] = 1e3 * median_ms(mis)                           # a clear of the norms and one launch
    r["jacobian_us"] = 1e3 * median_ms(jac)                           # two launches: the currents, then the entries
    jac(); mis()
    rhs = f.clone()
    r["factor_solve_ms"] = median_ms(lambda: fz.factor_solve_dev(jx.data_ptr(), f.data_ptr(), 1, 1e-3, st), lambda: f.copy_(rhs))
    fz.factor_status(st)
    r["step_ms"] = median_ms(lambda: (mis(), jac(), fz.factor_solve_dev(jx.data_ptr(), f.data_ptr(), 1, 1e-3, st)))
    r["iteration_over_factor_solve"] = r["ms_per_iteration"] / r["factor_solve_ms"]
    r["step_over_factor_solve"] = r["step_ms"] / r["factor_solve_ms"]
    r["scipy_over_device_per_scenario"] = 1e3 * r["scipy_s_per_scenario"] / (r["solve_ms"] / batch)
    plan.close()
    out[name] = r

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
