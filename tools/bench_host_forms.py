#!/usr/bin/env python3
"""Times the two host-staged paths that allocate device memory on every call: Factorization.solve (cs3_solve: one
right-hand side up, solve, down) and csc_lsolve_f (cs3_csc_lsolve: schedule, six uploads, sweep) on the 2000-column grid
Jacobian of the parity tests.  time.perf_counter around `--calls` calls each, after `--warmup`.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csparse3_amd import csc_hip as hip, synth      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=7)
b = np.random.default_rng(1).standard_normal(n)


def per_call_ms(fn):
    for _ in range(args.warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / args.calls


with hip.Factorization(m, n, Ap, Ai) as F:
    F.factor(Ax, 1e-3)
    Lp, Li, Lx = F.factors()[:3]
    solve_ms = per_call_ms(lambda: F.solve(b))
x = b.copy()
lsolve_ms = per_call_ms(lambda: hip.csc_lsolve_f(n, Lp, Li, Lx, x))
print(json.dumps({"calls": args.calls, "solve_host_ms": round(solve_ms, 4), "csc_lsolve_ms": round(lsolve_ms, 4)}))
