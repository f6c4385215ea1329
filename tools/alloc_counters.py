#!/usr/bin/env python3
"""Prints Factorization.debug_alloc_counters() -- (device allocations incl. graph instantiations, host synchronisations)
-- after every step of the sequence of tests/test_gpu_updates.py::test_dev_form_equals_the_host_form_and_later_calls_do_
not_allocate, plus a second, wider plan.  Two builds of the library that manage device memory the same way print the same
lines:   python tools/alloc_counters.py > a.txt   (in each tree), then diff."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from csparse3_amd import csc_hip as hip, synth      # noqa: E402
import updates_ref as ur                            # noqa: E402

m, n, Ap, Ai, Ax = synth.grid_jacobian(n=2000, seed=7)
A = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
cases = ur.branch_outages(A, 150, seed=103) + [ur.singular_case(A, 17)]
pattern, cx = ur.flatten(cases)
b = np.random.default_rng(107).standard_normal(n)
dev = torch.device("cuda", 0)
d_cx, d_b = torch.from_numpy(cx.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
with hip.Factorization(m, n, Ap, Ai) as F:
    def show(step):
        print("%-28s allocs %3d syncs %3d" % ((step,) + F.debug_alloc_counters()), flush=True)

    show("analysed")
    F.factor(Ax, 1e-3)
    show("factor")
    with F.updates_plan(pattern) as plan:
        F.solve_updates(plan, cx, b, 1e-10)
        show("solve_updates (host form)")
        side = torch.cuda.Stream()
        for k, stream in enumerate((torch.cuda.current_stream(), side, side)):
            d_x = torch.full((n, len(cases)), -7.0, dtype=torch.float64, device=dev)
            d_r = torch.full((len(cases),), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            F.solve_updates_dev(plan, d_cx.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr(), 1e-10, stream.cuda_stream)
            show("solve_updates_dev, call %d" % (k + 1))
            torch.cuda.synchronize()
        F.solve_updates_dev(plan, d_cx.data_ptr(), d_b.data_ptr(), d_x.data_ptr(), 0, 1e-10)
        show("solve_updates_dev, no rpiv")
        torch.cuda.synchronize()
        wide = ur.flatten(ur.branch_outages(A, 600, seed=109))
        with F.updates_plan(wide[0]) as plan2:
            F.solve_updates(plan2, wide[1], b, 1e-10)
            show("a wider plan (Z regrows)")
            F.solve_updates(plan, cx, b, 1e-10)
            show("the first plan again")
    F.solve(np.ones((n, 40)))
    show("solve, 40 right-hand sides")
    F.factor(Ax, 1e-3)
    F.solve(b)
    show("refactor, solve")
