"""Worker of tests/test_launch_plan_cpu.py and tests/golden/make_launch_plans.py: prints the launch plans of the cases of
launch_plan_cases.CASES whose indices are given, as one JSON list of row lists, under the environment it was started with
(the library reads CS3_NO_OVERLAP and CS3_NO_GEMM_SWEEPS once per process)."""
import json
import sys

from csparse3_amd import csc_hip as hip
import launch_plan_cases as lp

out = []
for i in map(int, sys.argv[1:]):
    name, sym, batch, op, nrhs, trans, _, _ = lp.CASES[i]
    with lp.handle(hip, name, batch, sym) as F:
        out.append(lp.plan(hip, F, op, nrhs, trans).tolist())
print(json.dumps(out))
