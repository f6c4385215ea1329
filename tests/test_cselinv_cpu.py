"""Complex selected inversion (cs3_cplx_selinv_*) without a GPU: the symbols, the limits, every check of the header in its
order on handles that were never factorised, the maps against those of the real handle, and the restatement
(tests/cselinv_ref.py) against numpy.linalg.inv -- so that what the GPU tests compare with bit for bit is itself right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cplx_cases
import cplx_ref as ref
import cselinv_cases as cc
import cselinv_ref as cr

SYMBOLS = ("cs3_cplx_selinv_limits", "cs3_cplx_selinv_entries_dev", "cs3_cplx_selinv_diag_dev", "cs3_cplx_selinv_thevenin_dev",
           "cs3_cplx_selinv_entries", "cs3_cplx_selinv_diag", "cs3_cplx_selinv_thevenin", "cs3_debug_cplx_selinv_maps")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csparse3_amd.h")


def test_the_symbols_are_declared_and_exported(hip):
    with open(HEADER) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), "include/csparse3_amd.h does not declare " + name
        assert hasattr(hip.lib(), name), "libcsparse3_hip.so does not export " + name
    for method in ("selinv", "inverse_entries", "inverse_diagonal", "thevenin", "inverse_entries_dev", "inverse_diagonal_dev",
                   "thevenin_dev"):
        assert callable(getattr(hip.ComplexFactorization, method, None)), method
    assert "complex handles;" not in text                                   # the real section no longer rules them out


def test_limits(hip):
    lim = hip.cplx_selinv_limits()
    assert lim.block > 0 and lim.block % 64 == 0 and lim.block <= 1024       # whole waves, a legal workgroup
    assert lim.grid_cap > 0 and lim.grid_cap * lim.block < 2 ** 31            # the flat index of one pass fits 32 bits with room
    assert C.sizeof(hip.CplxSelinvLimits) == 2 * 8
    assert hip.lib().cs3_cplx_selinv_limits(None) == hip.CS3_ERR_ARG
    buf = (C.c_int64 * 3)(-7, -7, -7)                                          # a guard behind the struct stays
    assert hip.lib().cs3_cplx_selinv_limits(C.cast(buf, C.POINTER(hip.CplxSelinvLimits))) == 0
    assert (buf[0], buf[1], buf[2]) == (lim.block, lim.grid_cap, -7)
    assert cc.gather_edge_orders() == [lim.block - 1, lim.block, lim.block + 1]


# ---- the checks, in the header's order ---------------------------------------------------------------------------------

ALIGNED, MISALIGNED = 0x10000, 0x10008             # device addresses that no check follows


def _calls(hip, p, h, out_dev, out_host):
    """name -> a function returning (status, message): every getter, device forms first."""
    L = hip.lib()
    dev = None if out_dev is None else C.c_void_p(out_dev)
    host = None if out_host is None else hip._pc(out_host)
    fns = {"cs3_cplx_selinv_entries_dev": lambda: L.cs3_cplx_selinv_entries_dev(p, h, 0, dev, None),
           "cs3_cplx_selinv_entries_dev(trans)": lambda: L.cs3_cplx_selinv_entries_dev(p, h, 1, dev, None),
           "cs3_cplx_selinv_diag_dev": lambda: L.cs3_cplx_selinv_diag_dev(p, h, dev, None),
           "cs3_cplx_selinv_thevenin_dev": lambda: L.cs3_cplx_selinv_thevenin_dev(p, h, dev, None),
           "cs3_cplx_selinv_entries": lambda: L.cs3_cplx_selinv_entries(p, h, 0, host),
           "cs3_cplx_selinv_diag": lambda: L.cs3_cplx_selinv_diag(p, h, host),
           "cs3_cplx_selinv_thevenin": lambda: L.cs3_cplx_selinv_thevenin(p, h, host)}

    def wrap(fn):
        return lambda: (fn(), L.cs3_last_error().decode())
    return {name: wrap(fn) for name, fn in fns.items()}


def test_checks_in_their_documented_order(hip):
    """Every call is wrong in everything that comes later as well: a misaligned device output (check 4) and no
    factorisation (check 5) throughout."""
    n, Ap, Ai, Az = cc.matrices()["ybus40"][:4]
    n2, Ap2, Ai2, _ = cplx_cases.hermitian_pd(40, 61, 5)                      # the same order, another entry count
    assert n2 == n and Ap2[n] != Ap[n]
    Rp, Ri = ref.real_pattern(n, Ap, Ai)
    Azr, Azi = ref.split(Az, (1, -1))
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, True)
    Rx = ref.values(n, Ap, Ai, Azr, Azi, sr, si)[0]
    E, S = hip.CS3_ERR_ARG, hip.CS3_ERR_STATE
    host = np.empty(int(Ap[n]) + n, dtype=np.complex128)
    with hip.ComplexFactorization(n, Ap, Ai) as F, hip.ComplexFactorization(n, Ap, Ai, batch=2) as F2, \
            hip.ComplexFactorization(n2, Ap2, Ai2) as G, hip.ComplexFactorization(n, Ap, Ai, schur=[37, 3, 11]) as FS, \
            hip.ComplexFactorization(n, Ap, Ai, batch=128) as FI, hip.Factorization(n, n, Ap, Ai) as R, \
            hip.Factorization(2 * n, 2 * n, Rp, Ri, match_values=Rx) as FM:
        p, h = F.plan._p, F.real._h
        # 1. null plan, handle or output
        for pp, hh, dev, hst in ((None, R._h, MISALIGNED, host), (p, None, MISALIGNED, host), (p, R._h, None, None)):
            for name, call in _calls(hip, pp, hh, dev, hst).items():
                rc, msg = call()
                assert rc == E and "null" in msg, (name, msg)
        # 2. a handle that is not one on the plan's real form: its order, its entries, its batch
        for hh in (R._h, G.real._h, F2.real._h):
            for name, call in _calls(hip, p, hh, MISALIGNED, host).items():
                rc, msg = call()
                assert rc == E and "not one on the real form" in msg and msg.startswith(name.split("(")[0] + ": "), (name, msg)
        rc, msg = _calls(hip, F2.plan._p, h, MISALIGNED, host)["cs3_cplx_selinv_diag_dev"]()
        assert rc == E and "batches differ" in msg
        # 3. the refusals of cs3_selinv_*, in their wording
        for K, word in ((FS, "not available on a Schur handle (cs3_analyze_schur)"), (FI, "matrix-interleaved batch (128 or more matrices)")):
            for name, call in _calls(hip, K.plan._p, K.real._h, MISALIGNED, host).items():
                rc, msg = call()
                assert rc == E and word in msg, (name, msg)
        for name, call in _calls(hip, p, FM._h, MISALIGNED, host).items():
            rc, msg = call()
            assert rc == E and "not available for a matched handle" in msg, (name, msg)
        # 4. a misaligned device output; the host forms have none and go on to 5
        for name, call in _calls(hip, p, h, MISALIGNED, host).items():
            rc, msg = call()
            if name.split("(")[0].endswith("_dev"):
                assert rc == E and "aligned to 16 bytes" in msg, (name, msg)
            else:
                assert rc == S and "factorisation" in msg, (name, msg)
        # 5. no successful factorisation
        for name, call in _calls(hip, p, h, ALIGNED, host).items():
            rc, msg = call()
            assert rc == S and "before a successful factorisation" in msg, (name, msg)
        # the maps need no factorisation, and refuse what checks 1 to 3 refuse
        L = hip.lib()
        assert L.cs3_debug_cplx_selinv_maps(p, h, None, None, None) == 0
        assert L.cs3_debug_cplx_selinv_maps(None, h, None, None, None) == E
        assert L.cs3_debug_cplx_selinv_maps(p, R._h, None, None, None) == E
        assert L.cs3_debug_cplx_selinv_maps(FS.plan._p, FS.real._h, None, None, None) == E


def test_a_handle_on_another_pattern_of_the_same_sizes_is_refused(hip):
    """Checks 1 to 3 pass (order, entries and batch agree); the maps notice."""
    n, Ap, Ai = cplx_cases.structural_cases()["unsorted"]
    Ai2 = Ai.copy()
    Ai2[[0, 1]] = Ai2[[1, 0]]                                                  # two rows of column 0 change places
    with hip.ComplexFactorization(n, Ap, Ai) as F, hip.ComplexFactorization(n, Ap, Ai2) as G:
        with pytest.raises(hip.Cs3Error) as e:
            hip._check(hip.lib().cs3_debug_cplx_selinv_maps(F.plan._p, G.real._h, None, None, None))
        assert e.value.code == hip.CS3_ERR_ARG and "not the real form of the complex plan's" in str(e.value) and "column 0" in str(e.value)
        assert hip.lib().cs3_debug_cplx_selinv_maps(F.plan._p, F.real._h, None, None, None) == 0


# ---- the maps ---------------------------------------------------------------------------------------------------------

def test_a_pattern_with_an_entry_stored_twice_has_no_handle(hip):
    """Why the twice-stored diagonal of cplx_cases is not among the GPU cases: the analysis refuses duplicates, as it always
    has, so the getters never see an entry twice.  (The restatement takes such a pattern: see below.)"""
    n, Ap, Ai = cplx_cases.structural_cases()["diag_twice"]
    with pytest.raises(hip.Cs3Error, match="duplicate entry"):
        hip.ComplexFactorization(n, Ap, Ai)


@pytest.mark.parametrize("name", ["ybus40", "hermitian_pd", "unsorted"])
def test_maps_are_the_real_handles_in_pairs(hip, name):
    case = cc.matrices()[name]
    n, Ap, Ai = case[:3]
    nnz = int(Ap[n])
    lo, hi = ref.positions(n, Ap)
    with hip.ComplexFactorization(n, Ap, Ai, kind=cc.kind_of(case), rotate=case[5]) as F:
        entry, entry_t, diag = F.selinv_maps()
        _, _, emap, dmap = F.real.selinv_plan()
        zpool = F.real.selinv_info().zpool_doubles
    for m in (entry, entry_t, diag):
        assert m.min() >= 0 and m.max() < zpool                                # nothing a kernel reads lies outside Z
    assert np.array_equal(entry[:, 0], emap[lo]) and np.array_equal(entry[:, 1], emap[lo + 1])
    assert np.array_equal(diag[:, 0], dmap[0::2])
    first = cr.first_diagonal_entry(n, Ap, Ai)
    assert (first >= 0).all()
    assert np.array_equal(diag, entry[first])                                  # (ZR(2i, 2i), ZR(2i + 1, 2i)) is the pair of a stored (i, i)
    # the transposed pair of (i, j) is the pair of a stored (j, i)
    col = ref.entry_columns(n, Ap)
    where = {(int(Ai[e]), int(col[e])): e for e in range(nnz)}
    checked = 0
    for e in range(nnz):
        t = where.get((int(col[e]), int(Ai[e])))
        if t is not None:
            assert np.array_equal(entry_t[e], entry[t]), e
            checked += 1
    assert checked >= n


def test_maps_of_a_pattern_without_every_diagonal(hip):
    """Rows 1 and 3 have no stored (i, i): either 2i and 2i + 1 share a supernode and the pair exists, or the call names the
    complex row."""
    n, Ap, Ai = cplx_cases.structural_cases()["absent_diagonal"]
    with hip.ComplexFactorization(n, Ap, Ai) as F:
        try:
            entry, entry_t, diag = F.selinv_maps()
        except hip.Cs3Error as e:
            assert e.code == hip.CS3_ERR_STATE and re.search(r"complex row [13] has no stored diagonal", str(e))
            return
        _, _, _, dmap = F.real.selinv_plan()
        assert diag.min() >= 0 and np.array_equal(diag[:, 0], dmap[0::2]) and not np.array_equal(diag[:, 0], diag[:, 1])


# ---- the restatement against numpy.linalg.inv ---------------------------------------------------------------------------

def _restatement_case(n, Ap, Ai, Az, rotate):
    """The restatement fed with the real form of the dense inverse of M = diag(s) A, against inv(A).  Two dense inversions
    and one rounded product stand between the two sides.  An inverse computed from an LU factorisation satisfies, entry by
    entry, |dZ| <= c eps |Z| |A| |Z| with a modest c that grows with the order (Higham, Accuracy and Stability, ch. 14);
    that bound does not care about the scaling of the rows, which the 1-norm condition number of a matrix with a diagonal
    of 1e16 does.  With c = 64 for n <= 40, |s_j| <= sqrt 2 and four roundings of the product:
        |got - want|_ij <= 64 eps (|Z| |A| |Z| + sqrt 2 |Minv| |M| |Minv|)_ij + 4 eps |Z_ij| + 16 eps max |Z|,
    and the Thevenin entry gets the sum of the bounds of its four terms.  The last term is a floor at the level of one
    rounding of the largest entry: where Z_ij is a structural zero of a reducible matrix the componentwise bound is zero
    too, but a row pivot or the rotation mixes rounding noise of the other entries into it.  -> the largest error over its
    bound."""
    Azr, Azi = ref.split(Az, (1, -1))
    sr, si = ref.rotation(n, Ap, Ai, Azr, Azi, rotate)
    s = ref.join(sr, si)[0]
    A = ref.dense_complex(n, Ap, Ai, Az)
    M = s[:, None] * A
    Z = np.linalg.inv(A)
    Minv = np.linalg.inv(M)
    eps = np.finfo(float).eps
    B = 64 * eps * (np.abs(Z) @ np.abs(A) @ np.abs(Z) + np.sqrt(2.0) * np.abs(Minv) @ np.abs(M) @ np.abs(Minv)) + 4 * eps * np.abs(Z)
    B += 16 * eps * (np.abs(Z).max() if n else 0.0)
    ZRe, ZRt, ZRd = cr.real_handle_outputs(cr.real_form(Minv), n, Ap, Ai)
    got = cr.restate(n, Ap, Ai, ZRe, ZRt, s, ZRd)
    want = cr.dense_results(Z, n, Ap, Ai)
    bound = cr.dense_results(B, n, Ap, Ai)
    row, col = np.asarray(Ai[:Ap[n]], dtype=np.int64), ref.entry_columns(n, Ap)
    bound["thevenin"] = B[row, row] + B[col, col] + B[row, col] + B[col, row]
    worst = 0.0
    for key in ("entries", "entries_t", "diagonal", "thevenin"):
        assert got[key].shape == (1,) + want[key].shape
        if want[key].size:
            ratio = float((np.abs(got[key][0] - want[key]) / bound[key]).max())
            assert ratio <= 1.0, (key, ratio)
            worst = max(worst, ratio)
    if (cr.first_diagonal_entry(n, Ap, Ai) >= 0).all():                       # the default source of the diagonal: the same numbers
        again = cr.restate(n, Ap, Ai, ZRe, ZRt, s)
        assert all(cr.same_bits(again[key], got[key]) for key in got)
    return worst


@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("name", sorted(cplx_cases.structural_cases()))
def test_restatement_reproduces_the_dense_inverse(name, rotate):
    n, Ap, Ai = cplx_cases.structural_cases()[name]
    Az = cplx_cases.values_for(np.random.default_rng(len(name)), int(Ap[n]))[0]
    col = np.repeat(np.arange(n), np.diff(Ap))
    Az[Ai == col] += 6.0j
    if name == "empty_column":                                                 # singular as it stands: the column gets its diagonal
        keep = np.ones(n, dtype=bool)
        keep[np.flatnonzero(np.diff(Ap) == 0)] = False
        idx = np.flatnonzero(keep)
        label = np.full(n, -1)
        label[idx] = np.arange(len(idx))
        sel = keep[Ai] & keep[col]
        Ap = np.concatenate([[0], np.cumsum(np.bincount(label[col[sel]], minlength=len(idx)))]).astype(np.int32)
        n, Ai, Az = len(idx), label[Ai[sel]].astype(np.int32), Az[sel]
    _restatement_case(n, Ap, Ai, Az, rotate)


def test_restatement_on_the_rows_of_the_diag_zoo_with_a_usable_diagonal():
    """The rows of diag_zoo whose stored diagonal is finite and not zero, as a matrix of their own: every branch of the
    rotation that a factorisation can follow (real, imaginary, ties, negative, stored twice)."""
    n, Ap, Ai, Az, kinds = cplx_cases.diag_zoo(np.random.default_rng(11))
    Az = Az[0]
    col = np.repeat(np.arange(n), np.diff(Ap))
    d = np.zeros(n, dtype=np.complex128)
    np.add.at(d, col[Ai == col], Az[Ai == col])
    stored = np.bincount(col[Ai == col], minlength=n) > 0
    keep = stored & np.isfinite(d) & (d != 0)
    assert {kinds[i] for i in np.flatnonzero(keep)} == {"re", "im", "tie", "tie_neg", "neg", "twice"}
    idx = np.flatnonzero(keep)
    label = np.full(n, -1)
    label[idx] = np.arange(len(idx))
    sel = keep[Ai] & keep[col]
    Ap2 = np.concatenate([[0], np.cumsum(np.bincount(label[col[sel]], minlength=len(idx)))]).astype(np.int32)
    Az2 = np.where(np.isfinite(Az[sel]), Az[sel], 0.0)
    _restatement_case(len(idx), Ap2, label[Ai[sel]].astype(np.int32), Az2, True)


def test_trans_and_the_rotation_are_told_apart():
    """On an unsymmetric matrix with a rotation that is not 1, the restatement's four results differ from one another where
    they should: trans is not the plain entries, and dropping s changes the answer."""
    n, Ap, Ai, Az = cc.structural("unsorted")[:4]
    Azr, Azi = ref.split(Az, (1, -1))
    s = ref.join(*ref.rotation(n, Ap, Ai, Azr, Azi, True))[0]
    Minv = np.linalg.inv(s[:, None] * ref.dense_complex(n, Ap, Ai, Az))
    ZRe, ZRt, ZRd = cr.real_handle_outputs(cr.real_form(Minv), n, Ap, Ai)
    got = cr.restate(n, Ap, Ai, ZRe, ZRt, s, ZRd)
    plain = cr.restate(n, Ap, Ai, ZRe, ZRt, np.ones(n, dtype=np.complex128), ZRd)
    assert not np.allclose(got["entries"], got["entries_t"]) and not np.allclose(got["entries"], plain["entries"])
    assert np.allclose(plain["entries"][0], cr.dense_results(Minv, n, Ap, Ai)["entries"])
