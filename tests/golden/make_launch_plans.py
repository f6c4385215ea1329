"""Writes tests/golden/launch_plans.json: for every case of tests/launch_plan_cases.py the sequence of launches, event
records and stream waits that the schedulers issue, and the scheduler branch the case takes.

The file was recorded at the commit BEFORE the schedule became a plan (csrc/schedule.cpp), from a build of that commit
patched for the recording: in the launcher section of csrc/kernels.hip a thread-local recorder logged every call of
launch_big_gather, launch_big_block, launch_schur_take, launch_fwd_big_pre / _chunk, launch_bwd_big_pre / _chunk, every
single-launch return of launch_front_group and launch_solve_group, and every hipEventRecord / hipStreamWaitEvent of
run_level and launch_factor_with_forward, as rows of cs3_debug_launch_plan's layout (stream slot from the fake stream
handle, event = its index in ForkJoin's pool); while recording these calls returned hipSuccess without touching HIP.  The
patched build answered cs3_debug_launch_plan itself, by running launch_factor_levels / launch_solve_levels /
launch_factor_with_forward on a DeviceFactor that held only kind, batch, the forest and two distinct fake descriptor
pointers.  Re-record only when the schedule is changed on purpose; with today's library the script merely rewrites what
cs3_debug_launch_plan prints:

  CS3_LIB_PATH=<library> python tests/golden/make_launch_plans.py
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)

import launch_plan_cases as lp  # noqa: E402


def worker(indices, env):
    """The plans of CASES[indices] from a child process under `env` (the switches are read once per process)."""
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    p = subprocess.run([sys.executable, os.path.join(TESTS, "launch_plan_worker.py")] + [str(i) for i in indices], env=e,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    out = {}
    envs = sorted({tuple(sorted(c[6].items())) for c in lp.CASES})
    for env in envs:
        idx = [i for i, c in enumerate(lp.CASES) if tuple(sorted(c[6].items())) == env]
        for i, rows in zip(idx, worker(idx, dict(env))):
            c = lp.CASES[i]
            branch = lp.branch_of(np.array(rows, dtype=np.int32).reshape(-1, 10), c[3])
            assert branch == c[7], (lp.case_id(c), branch, c[7])
            out[lp.case_id(c)] = {"branch": branch, "rows": rows}
    with open(os.path.join(HERE, "launch_plans.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": {"branch": "%s", "rows": %s}' % (k, v["branch"], json.dumps(v["rows"], separators=(",", ":")))
                                   for k, v in out.items()) + "\n}\n")
    print("%d cases" % len(out))
