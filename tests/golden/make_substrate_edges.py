#!/usr/bin/env python3
"""Generate tests/golden/substrate_edges.npz: the outputs of the reference's own Python kernels on the small cases of
tests/substrate_cases.py (bucket lengths, scan tiles, csc_add_ff, csc_sub_matrix, csc_norm, find_islands, stacking).

Runs only where the reference is installed; it is loaded as make_golden.py loads it (a stand-in for the numba
decorators, the bodies that run are the reference's own).  Only outputs are saved: the inputs come from the seeded
builders of substrate_cases.py, and tests/test_substrate_cases_cpu.py pins them through the stored checksums.  Cases the
reference cannot run (it raises, or would index past what it allocates) are left out and listed in `skipped`.

    python tests/golden/make_substrate_edges.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden                      # noqa: E402
import substrate_cases as sc            # noqa: E402

OUT = os.path.join(HERE, "substrate_edges.npz")


def checksum(*arrays):
    """CRC of the inputs a recorded output belongs to (the builders are seeded; this notices one that drifted)."""
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.int64(c)


def main():
    ref = make_golden._load_reference()
    out, skipped = {}, []

    def attempt(tag, fn):
        try:
            fn()
        except Exception as e:                                  # the reference cannot run this one
            skipped.append("%s: %s" % (tag, type(e).__name__))

    def transpose_family(tag, m, n, Ap, Ai, Ax):
        def run():
            _, _, Tp, Ti, Tx = ref.csc_transpose(m, n, Ap, Ai, Ax)
            nz = int(Ap[n])
            Rp = np.zeros(m + 1, dtype=np.int32); Ri = np.empty(nz, dtype=np.int32); Rx = np.empty(nz)
            ref.csc_to_csr(m, n, Ap, Ai, Ax, Rp, Ri, Rx)
            out.update({tag + "__in": checksum(Ap, Ai, Ax), tag + "__t_p": Tp, tag + "__t_i": Ti[:nz], tag + "__t_x": Tx[:nz],
                        tag + "__csr_p": Rp, tag + "__csr_i": Ri, tag + "__csr_x": Rx})
        attempt(tag, run)

    def coo_family(tag, m, n, Ti, Tj, Tx):
        def run():
            _, _, Kp, Ki, Kx = ref.coo_to_csc(m, n, Ti.copy(), Tj.copy(), Tx.copy(), len(Ti))
            out.update({tag + "__in": checksum(Ti, Tj, Tx), tag + "__p": Kp, tag + "__i": Ki[:Kp[n]], tag + "__x": Kx[:Kp[n]]})
        attempt(tag, run)

    # 1. bucket lengths
    m, n, Ap, Ai, Ax, _ = sc.bucket_lengths()
    transpose_family("bucket", m, n, Ap, Ai, Ax)
    m, n, Ti, Tj, Tx, _ = sc.bucket_triplets()
    coo_family("bucket_coo", m, n, Ti, Tj, Tx)
    # 2. scan tiles: the transpose scans the rows, coo_to_csc of the transposed triplets the same counts as columns
    for nb in sc.SCAN_BUCKETS:
        m, n, Ap, Ai, Ax, _ = sc.scan_tiles(nb)
        transpose_family("scan%d" % nb, m, n, Ap, Ai, Ax)
        coo_family("scan%d_coo" % nb, n, m, sc.columns_of(Ap), Ai, Ax)
    z = np.zeros(0, dtype=np.int32)
    transpose_family("m0", 0, 4, np.zeros(5, dtype=np.int32), z, np.zeros(0))
    transpose_family("n0", 4, 0, np.zeros(1, dtype=np.int32), z, np.zeros(0))
    coo_family("m0_coo", 0, 4, z, z, np.zeros(0))
    coo_family("n0_coo", 4, 0, z, z, np.zeros(0))
    # 4. csc_add_ff
    for name, (m, n, A, B, alpha, beta, _) in sc.add_cases().items():
        tag = "add_" + name.replace(" ", "_")

        def run():
            _, _, Cp, Ci, Cx = ref.csc_add_ff(m, n, *A, m, n, *B, alpha, beta)
            out.update({tag + "__in": checksum(*A, *B), tag + "__p": Cp, tag + "__i": Ci[:Cp[n]], tag + "__x": Cx[:Cp[n]]})
        attempt(tag, run)
    # 5. csc_sub_matrix
    Am, Ap, Ai, Ax, _ = sc.sub_matrix_source()
    for nrows in sc.SUB_ROW_COUNTS:
        rows, cols = sc.sub_selection(nrows, Ap, Ai)
        tag = "sub%d" % nrows

        def run():
            nz, Bp, Bi, Bx = ref.csc_sub_matrix(Am, int(Ap[-1]), Ap, Ai, Ax, rows, cols)
            out.update({tag + "__in": checksum(Ap, Ai, Ax, rows, cols), tag + "__nz": np.int64(nz), tag + "__p": Bp,
                        tag + "__i": Bi, tag + "__x": Bx})
        attempt(tag, run)

    def run():
        nz, Bp, Bi, Bx = ref.csc_sub_matrix(Am, int(Ap[-1]), Ap, Ai, Ax, np.array([sc.SUB_R0, 5], dtype=np.int32), z)
        out.update({"sub_ncols0__nz": np.int64(nz), "sub_ncols0__p": Bp, "sub_ncols0__i": Bi, "sub_ncols0__x": Bx})
    attempt("sub_ncols0", run)
    # 6. csc_norm
    for name, (n, Ap, Ax, _) in sc.norm_cases().items():
        tag = "norm_" + name.replace(" ", "_")
        attempt(tag, lambda: out.update({tag + "__in": checksum(Ap, Ax), tag: np.float64(ref.csc_norm(n, Ap, Ax))}))
    # 7. find_islands (each island sorted, as CscMat.islands does)
    for name, (n, Ap, Ai, _) in sc.island_cases().items():
        tag = "isl_" + name.replace(" ", "_")

        def run():
            isl = [np.sort(np.array(list(x), dtype=np.int32)) for x in ref.find_islands(n, Ap, Ai)]
            out.update({tag + "__in": checksum(Ap, Ai), tag + "__flat": np.concatenate(isl).astype(np.int32),
                        tag + "__sizes": np.array([len(x) for x in isl], dtype=np.int32)})
        attempt(tag, run)
    # 8. stacking
    for name, (blocks, _) in sc.stack_cases().items():
        tag = "stack_" + name.replace(" ", "_")

        def run():
            sm, sn, Si, Sp, Sx = ref.csc_stack_4_by_4_ff(*[v for b in blocks for v in b])
            out.update({tag + "__in": checksum(*[v for b in blocks for v in b[2:]]), tag + "__m": np.int64(sm), tag + "__n": np.int64(sn),
                        tag + "__i": Si, tag + "__p": Sp, tag + "__x": Sx})
        attempt(tag, run)

    out["skipped"] = np.array(skipped)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "with", len(out), "arrays,", os.path.getsize(OUT), "bytes; skipped:", skipped)


if __name__ == "__main__":
    main()
