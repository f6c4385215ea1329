"""Writes the two fixtures of the Schur-complement tests (tests/schur_cases.py).

  python tests/golden/make_schur_fixtures.py schedule   -> schur_schedule.npz
      cs3_debug_schedule of plain cs3_analyze handles.  Recorded at the commit BEFORE Schur handles existed: the test
      pins that their analysis did not change.  Re-record only when the plain schedule is changed on purpose.
  python tests/golden/make_schur_fixtures.py refs       -> schur_refs.npz
      the dense NumPy float64 reference A22 - A21 @ solve(A11, A12) of grid20k with ns = 300 (an interior of 19 700
      variables: a few minutes and 3 GB).  Needs neither the library nor a GPU.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import schur_cases as sc  # noqa: E402


def schedule():
    from csparse3_amd import csc_hip as hip
    out = {}
    for name, batch in sc.SCHEDULE_CASES:
        sched, fr, fw = sc.plain_schedule(hip, name, batch)
        tag = "%s_b%d" % (name, batch)
        out[tag + "_sched"], out[tag + "_r"], out[tag + "_w"] = sched, fr, fw
    np.savez_compressed(os.path.join(HERE, "schur_schedule.npz"), **out)


def refs():
    m, n, Ap, Ai, Ax = sc.matrix("grid20k")
    idx = sc.schur_set("grid20k", 300)
    S = sc.reference(sc.to_scipy(n, Ap, Ai, Ax), idx)
    np.savez(os.path.join(HERE, "schur_refs.npz"), grid20k_idx=idx, grid20k_S=S)


if __name__ == "__main__":
    {"schedule": schedule, "refs": refs}[sys.argv[1]]()
