#!/usr/bin/env python3
"""AC state estimation on the device (csparse3_amd.csc_hip.StateEstPlan): the whole Gauss-Newton solve, one iteration of it
against the two existing parts it is made of -- SpgemmPlan.values_dev and factor_solve_dev (k = 1) on the same patterns and
values, timed alone in the same process --, the new kernels alone, the same iteration in SciPy on the host (H by
tests/se_ref.py, splu of G) with its iteration count, and bad_data beside selinv alone.  Event-timed, median of --reps, one
GPU.  Writes one JSON line to profiles/stateest_bench.json.

Case: synth.se_ac_case(nbus, 1.02 nbus, seed nbus, noise 1) at the largest of --sizes whose gain matrix cs3_analyze accepts
(the gain matrix of an AC estimate couples every pair of states that meet in a row of H: about four times the entries of
the DC one of bench_quad.py); a refusal is recorded with its message.  The start is the planted state moved by U(-0.02, 0.02)
in the angles and U(-0.01, 0.01) in the magnitudes, the same for the device and the host.
    python tools/bench_stateest.py [--sizes 50000 20000 10000] [--reps 10]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch
import se_ref as R
from csparse3_amd import csc_hip as hip, synth

TOL, MAX_ITERS, CRIT_TOL = 1e-8, 20, 1e-8

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", nargs="+", type=int, default=[50000, 20000, 10000])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stateest_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)


def median_ms(fn, before=None):
    """Median over args.reps of the device time of fn(), between two events on the current stream."""
    for _ in range(2):
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


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return torch.from_numpy(a.reshape(-1).copy()).to(dev)


def host_newton(P, case, vm, va):
    """The driver's state machine with SciPy: -> (iters, flag, seconds per iteration, vm, va)."""
    vm, va = vm.copy(), va.copy()
    m, ns, na = P["m"], P["ns"], P["na"]
    w, spent, flag = case["w"], [], 1
    for _ in range(MAX_ITERS):
        t0 = time.perf_counter()
        cur = R.measure_ref(P, case["Yz"], case["Ye"], case["z"], vm, va)
        Hr = R.jacobian_ref(P, case["Yz"], case["Ye"], vm, va, cur)[0]
        H = sp.csr_matrix((Hr, P["Hrj"], P["Hrp"]), shape=(m, ns))
        G = (H.T @ sp.diags(w) @ H).tocsc()
        dx = spla.splu(G).solve(H.T @ (w * cur["r"]))
        va[P["sbus"][:na]] += dx[:na]
        vm += dx[na:]
        spent.append(time.perf_counter() - t0)
        step = np.abs(dx).max()
        if not np.isfinite(step):
            flag = 2; break
        if step <= TOL:
            flag = 0; break
    return len(spent), flag, float(np.median(spent)), vm, va


out = {"reps": args.reps, "tol": TOL, "refusals": {}}
for nbus in args.sizes:
    case = synth.se_ac_case(nbus, nbus + nbus // 50, nbus, noise=1.0)
    plan = hip.StateEstPlan(case["n"], case["Yp"], case["Yi"], case["ref"], case["end_from"], case["end_to"], case["kind"], case["where"])
    t0 = time.perf_counter()
    try:
        fz = plan.factorization                                 # builds the product, the analysis, the bilinear-form plan
    except hip.Cs3Error as e:
        out["refusals"][str(nbus)] = str(e)
        plan.close()
        continue
    out["solver_build_s"] = time.perf_counter() - t0
    break
else:
    print(json.dumps(out))
    sys.exit("no size was accepted")

info = plan.info
n, m, ns, na = plan.n, plan.m, plan.ns, plan.na
out.update(nbus=n, nedges=len(case["end_from"]) // 2, m=m, ns=ns, nnz_h=plan.nnz_h, nnz_g=int(info.nnz_g), max_row=int(info.max_row),
           max_col=int(info.max_col), rows_per_kind=[int(getattr(info, "kind%d" % k)) for k in range(5)])
rng = np.random.default_rng(1)
vm0 = case["vm"] + rng.uniform(-0.01, 0.01, size=n)
va0 = case["va"] + rng.uniform(-0.02, 0.02, size=n)
va0[case["ref"]] = 0.0

Yz, Ye, z, w = (to_dev(case[k]) for k in ("Yz", "Ye", "z", "w"))
vm, va, vm_start, va_start = to_dev(vm0), to_dev(va0), to_dev(vm0), to_dev(va0)
ptrs = tuple(t.data_ptr() for t in (Yz, Ye, z, w, vm, va))


def reset():
    vm.copy_(vm_start); va.copy_(va_start)


reset()
res = plan.solve_dev(*ptrs, tol=TOL, max_iters=MAX_ITERS)
x_dev = np.concatenate([va.cpu().numpy(), vm.cpu().numpy()])
out.update(iters=res["iters"], flag=res["flag"], step=res["step"], J=res["J"], J_over_m_minus_ns=res["J"] / (m - ns))
out["solve_ms"] = median_ms(lambda: plan.solve_dev(*ptrs, tol=TOL, max_iters=MAX_ITERS), before=reset)
out["iteration_ms"] = out["solve_ms"] / max(res["iters"], 1)

# the two existing parts alone: the product's values and factor + solve, on the Jacobian at the solution
Hr, Hc, WHc, g = (torch.empty(max(k, 1), dtype=torch.float64, device=dev) for k in (plan.nnz_h, plan.nnz_h, plan.nnz_h, ns))
Gx = torch.empty(int(info.nnz_g), dtype=torch.float64, device=dev)
pat = plan.pattern()
gain = hip.SpgemmPlan(m, ns, pat["Hp"], pat["Hi"], m, ns, pat["Hp"], pat["Hi"], transpose_a=True)
jac = lambda: plan.jacobian_dev(Yz.data_ptr(), Ye.data_ptr(), w.data_ptr(), vm.data_ptr(), va.data_ptr(), Hr.data_ptr(), Hc.data_ptr(), WHc.data_ptr())
jac()


def parts():
    gain.values_dev(Hc.data_ptr(), WHc.data_ptr(), Gx.data_ptr())
    fz.factor_solve_dev(Gx.data_ptr(), g.data_ptr(), k=1, tol=0.0)


def kernels():
    plan.measure_dev(*ptrs)
    jac()
    plan.gradient_dev(Hc.data_ptr(), plan.residuals_dev()[1], g.data_ptr())


kernels()
out["values_ms"] = median_ms(lambda: gain.values_dev(Hc.data_ptr(), WHc.data_ptr(), Gx.data_ptr()))
out["factor_solve_ms"] = median_ms(lambda: fz.factor_solve_dev(Gx.data_ptr(), g.data_ptr(), k=1, tol=0.0), before=kernels)
out["parts_ms"] = median_ms(parts, before=kernels)
out["kernels_ms"] = median_ms(kernels)
out["iteration_over_parts"] = out["iteration_ms"] / out["parts_ms"]
fz.factor_status()

# bad data beside selinv alone (the factors of the last line are those of the solution)
summary = torch.empty(4, dtype=torch.float64, device=dev)
rn = torch.empty(m, dtype=torch.float64, device=dev)
bad = lambda: plan.bad_data_dev(*ptrs, CRIT_TOL, summary.data_ptr(), rn_ptr=rn.data_ptr())
bad()
fz.factor_status()
s = summary.cpu().numpy()
out.update(bad_data_worst=float(s[0]), bad_data_worst_row=int(s[1]), bad_data_critical=int(s[3]))
out["bad_data_ms"] = median_ms(bad)
out["selinv_ms"] = median_ms(lambda: fz.selinv())
out["bad_data_over_selinv"] = out["bad_data_ms"] / out["selinv_ms"]

# the host: the same state machine with SciPy
P = R.plan_ref(case["n"], case["Yp"], case["Yi"], case["ref"], case["end_from"], case["end_to"], case["kind"], case["where"])
h_iters, h_flag, h_iter_s, h_vm, h_va = host_newton(P, case, vm0, va0)
out.update(host_iters=h_iters, host_flag=h_flag, host_iteration_ms=1e3 * h_iter_s, host_over_device=1e3 * h_iter_s / out["iteration_ms"],
           max_state_difference=float(np.abs(x_dev - np.concatenate([h_va, h_vm])).max()))
gain.close()
plan.close()
if (h_iters, h_flag) != (res["iters"], res["flag"]):
    sys.exit("the device took %d iterations (flag %d), the host %d (flag %d): not reported" % (res["iters"], res["flag"], h_iters, h_flag))

print(json.dumps(out))
with open(args.out, "w") as f:
    f.write(json.dumps(out) + "\n")
