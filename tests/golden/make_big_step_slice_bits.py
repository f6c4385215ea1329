"""Writes tests/golden/big_step_slice_bits.json: per case of tests/big_step_slice_cases.py the SHA-256 of the bytes of Lx,
Ux and the fused step's x, and their sums.

To be run on the PARENT of a commit that touches k_big_step without meaning to change a bit of its results (the file in
git was recorded from a build of the commit before the elimination went from two column slices of 16 to four of 8), on a
machine with an MI355X, never from the tree under test:

  CS3_LIB_PATH=<the parent's library> python tests/golden/make_big_step_slice_bits.py

Re-record only when the arithmetic of the big-front chain is changed on purpose.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)

import big_step_slice_cases as ss  # noqa: E402
from csparse3_amd import csc_hip as hip  # noqa: E402

if __name__ == "__main__":
    import torch
    torch.cuda.init()
    out = {ss.case_id(c): ss.record(hip, c) for c in ss.CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "big_step_slice_bits.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in out.items()) + "\n}\n")
    print("%d cases" % len(out))
