#!/usr/bin/env python3
"""Generate tests/golden/spgemm.npz from the reference's own csc_multiply_ff (and csc_transpose).

Runs ONLY where the reference source is at hand, in the way make_golden.py does: the module is loaded by path with the
no-op numba stand-in, the bodies that execute are the reference's own.  Only inputs and outputs are saved -- no reference
source travels.  Every case has Am <= Bn: the reference sizes its workspaces by the columns of C and runs off them
otherwise.

Per case <tag>: <tag>_Am, _An, _Ap, _Ai, _Ax, _Bm, _Bn, _Bp, _Bi, _Bx, _ta (1: the product is csc_transpose(A) times B, A
stored untransposed) and the outputs _Cp, _Ci, _Cx.  "cases" lists the tags.

    python tests/golden/make_spgemm_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _load_reference, _random_csc          # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spgemm.npz")


def _shuffled_rows(rng, Ap, Ai, Ax):
    Ai, Ax = Ai.copy(), Ax.copy()
    for j in range(len(Ap) - 1):
        perm = rng.permutation(Ap[j + 1] - Ap[j]) + Ap[j]
        Ai[Ap[j]:Ap[j + 1]] = Ai[perm]
        Ax[Ap[j]:Ap[j + 1]] = Ax[perm]
    return Ai, Ax


def _without_columns(Ap, Ai, Ax, drop):
    keep = np.ones(Ap[-1], dtype=bool)
    counts = np.diff(Ap)
    for j in drop:
        keep[Ap[j]:Ap[j + 1]] = False
        counts[j] = 0
    Np = np.zeros(len(Ap), dtype=np.int32)
    Np[1:] = np.cumsum(counts)
    return Np, Ai[keep].copy(), Ax[keep].copy()


def main():
    ref = _load_reference()
    rng = np.random.default_rng(20251)
    out, tags = {}, []

    def record(tag, Am, An, A, Bm, Bn, B, ta=0):
        (Ap, Ai, Ax), (Bp, Bi, Bx) = A, B
        if ta:
            Tm, Tn, Tp, Ti, Tx = ref.csc_transpose(Am, An, Ap, Ai, Ax)
            Cm, Cn, Cp, Ci, Cx, nz = ref.csc_multiply_ff(Tm, Tn, Tp, Ti[:Tp[Tn]], Tx[:Tp[Tn]], Bm, Bn, Bp, Bi, Bx)
            assert (Cm, Cn) == (An, Bn)
        else:
            Cm, Cn, Cp, Ci, Cx, nz = ref.csc_multiply_ff(Am, An, Ap, Ai, Ax, Bm, Bn, Bp, Bi, Bx)
            assert (Cm, Cn) == (Am, Bn)
        assert Cm <= Cn and nz == Cp[Cn] and len(Ci) == nz and len(Cx) == nz
        out.update({tag + "_Am": np.int64(Am), tag + "_An": np.int64(An), tag + "_Ap": Ap, tag + "_Ai": Ai, tag + "_Ax": Ax,
                    tag + "_Bm": np.int64(Bm), tag + "_Bn": np.int64(Bn), tag + "_Bp": Bp, tag + "_Bi": Bi, tag + "_Bx": Bx,
                    tag + "_ta": np.int64(ta), tag + "_Cp": Cp.astype(np.int32), tag + "_Ci": Ci.astype(np.int32),
                    tag + "_Cx": Cx.astype(np.float64)})
        tags.append(tag)

    # ---- seeded random shapes
    shapes = {"r1": (40, 40, 40, 0.08), "r2": (25, 57, 31, 0.12), "r3": (31, 60, 31, 0.2), "r4": (64, 64, 64, 0.3)}
    mats = {}
    for tag, (Am, An, Bn, dens) in shapes.items():
        mats[tag] = (_random_csc(rng, Am, An, dens), _random_csc(rng, An, Bn, dens))
        record(tag, Am, An, mats[tag][0], An, Bn, mats[tag][1])
    # ---- r3 again with the rows of every column of A and of B shuffled
    (Ap, Ai, Ax), (Bp, Bi, Bx) = mats["r3"]
    Ai2, Ax2 = _shuffled_rows(rng, Ap, Ai, Ax)
    Bi2, Bx2 = _shuffled_rows(rng, Bp, Bi, Bx)
    record("r3s", 31, 60, (Ap, Ai2, Ax2), 60, 31, (Bp, Bi2, Bx2))
    # ---- B with empty columns, and B selecting empty columns of A
    A = _without_columns(*_random_csc(rng, 20, 30, 0.25), drop=range(0, 30, 3))
    B = _without_columns(*_random_csc(rng, 30, 25, 0.25), drop=[0, 7, 8, 24])
    record("emp", 20, 30, A, 30, 25, B)
    # ---- duplicates and unsorted rows: the 4 x 4 matrix of substrate.npz times itself
    dAp = np.array([0, 4, 4, 7, 9], dtype=np.int32)
    dAi = np.array([2, 0, 2, 1, 3, 3, 0, 1, 1], dtype=np.int32)
    dAx = np.array([1.0, 2.0, 0.5, -3.0, 4.0, 0.25, 7.0, -1.5, 2.5])
    record("dup", 4, 4, (dAp, dAi, dAx), 4, 4, (dAp, dAi, dAx))
    # ---- the sign of zero: (-1) * 0 is stored as it is
    one = np.array([0, 1], dtype=np.int32)
    zero = np.array([0], dtype=np.int32)
    record("negzero", 1, 1, (one, zero, np.array([-1.0])), 1, 1, (one, zero.copy(), np.array([0.0])))
    assert np.signbit(out["negzero_Cx"][0])
    # ---- transposed left factor: csc_transpose, then csc_multiply_ff
    record("t1", 57, 25, _random_csc(rng, 57, 25, 0.12), 57, 31, _random_csc(rng, 57, 31, 0.12), ta=1)
    record("tdup", 4, 4, (dAp, dAi, dAx), 4, 4, (dAp, dAi, dAx), ta=1)

    out["cases"] = np.array(tags)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "with", len(out), "arrays,", os.path.getsize(OUT), "bytes")
    for tag in tags:
        Cp, Ci = out[tag + "_Cp"], out[tag + "_Ci"]
        unsorted = sum(1 for j in range(len(Cp) - 1) if np.any(np.diff(Ci[Cp[j]:Cp[j + 1]]) < 0))
        print("  %-8s nnz(C) = %4d, columns with unsorted rows: %d" % (tag, Cp[-1], unsorted))


if __name__ == "__main__":
    main()
