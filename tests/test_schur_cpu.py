"""Schur handles (cs3_analyze_schur), the part that needs no GPU: argument checks and the analysis.

The Schur variables are ordered last in the caller's order, form the last supernode [n - ns, n) exactly, and stay out of
the bottom forest; the order of the interior is that of A11 alone; plain handles analyse as before."""
import ctypes as C
import os

import numpy as np
import pytest

import schur_cases as sc

I32P = C.POINTER(C.c_int32)


def _p(a):
    return None if a is None else a.ctypes.data_as(I32P)


def _analyze_raw(hip, n, Ap, Ai, ns, idx, kind=0, order=1, q=None, batch=1):
    """cs3_analyze_schur through ctypes, nothing checked on the Python side: -> (return code, message)."""
    h = C.c_void_p()
    rc = hip.lib().cs3_analyze_schur(kind, order, n, _p(Ap), _p(Ai), _p(q), batch, ns, _p(idx), C.byref(h))
    msg = hip.lib().cs3_last_error().decode()
    if rc == 0:
        hip.lib().cs3_free(h)
    return rc, msg


def _handle(hip, name, idx, **kw):
    m, n, Ap, Ai, _ = sc.matrix(name)
    return hip.Factorization(m, n, Ap, Ai, schur=idx, **kw)


def _debug(hip, F):
    """-> (sched, front_r, front_w, forest supernodes)."""
    lib = hip.lib()
    lib.cs3_debug_schedule.argtypes = [C.c_void_p] + [I32P] * 3
    lib.cs3_debug_forest.argtypes = [C.c_void_p] + [I32P] * 4
    lib.cs3_debug_forest.restype = C.c_int64
    nsup = int(F.info.nsuper)
    sched, fr, fw = (np.empty(nsup, dtype=np.int32) for _ in range(3))
    assert lib.cs3_debug_schedule(F._h, _p(sched), _p(fr), _p(fw)) == 0
    nf = int(lib.cs3_debug_forest(F._h, None, None, None, None))
    sn = np.empty(max(nf, 1), dtype=np.int32)
    assert lib.cs3_debug_forest(F._h, _p(sn), None, None, None) == nf
    return sched, fr, fw, sn[:nf]


def test_argument_errors_in_order(hip):
    m, n, Ap, Ai, _ = sc.matrix("toy10")
    good = np.array([7, 2, 5], dtype=np.int32)
    assert _analyze_raw(hip, n, Ap, Ai, 3, good)[0] == 0
    # the checks of cs3_analyze come first
    bad_Ap = Ap.copy(); bad_Ap[0] = 1
    rc, msg = _analyze_raw(hip, n, bad_Ap, Ai, 3, np.array([7, 7, 99], dtype=np.int32))
    assert rc == hip.CS3_ERR_ARG and "Ap[0]" in msg
    rc, msg = _analyze_raw(hip, n, Ap, Ai, 3, good, batch=0)
    assert rc == hip.CS3_ERR_ARG and "batch" in msg
    # then the Schur set: null list, ns < 1, ns >= n, an index outside [0, n), a repeated index
    rc, msg = _analyze_raw(hip, n, Ap, Ai, 3, None)
    assert rc == hip.CS3_ERR_ARG and "null" in msg
    for ns in (0, -2, n, n + 1):
        rc, msg = _analyze_raw(hip, n, Ap, Ai, ns, np.arange(max(ns, 1), dtype=np.int32))
        assert rc == hip.CS3_ERR_ARG and "ns = %d" % ns in msg, (ns, msg)
    for bad in (-1, n, 12345):
        rc, msg = _analyze_raw(hip, n, Ap, Ai, 3, np.array([4, 4, bad], dtype=np.int32))      # (the repeat comes second)
        assert rc == hip.CS3_ERR_ARG and "index %d" % bad in msg and "outside" in msg, msg
    rc, msg = _analyze_raw(hip, n, Ap, Ai, 4, np.array([4, 8, 1, 8], dtype=np.int32))
    assert rc == hip.CS3_ERR_ARG and "index 8" in msg and "repeated" in msg, msg
    # a given order must be a permutation of the interior
    inter = np.array([0, 1, 3, 4, 6, 8, 9], dtype=np.int32)
    assert _analyze_raw(hip, n, Ap, Ai, 3, good, order=2, q=inter[::-1].copy())[0] == 0
    for q in (np.array([0, 1, 3, 4, 6, 8, 7], dtype=np.int32), np.array([0, 1, 3, 4, 6, 8, 8], dtype=np.int32)):
        rc, msg = _analyze_raw(hip, n, Ap, Ai, 3, good, order=2, q=q)
        assert rc == hip.CS3_ERR_ARG and "interior" in msg, msg
    rc, msg = _analyze_raw(hip, n, Ap, Ai, 3, good, order=2, q=None)
    assert rc == hip.CS3_ERR_ARG


@pytest.mark.parametrize("name,ns", [("toy10", 3), ("grid2k", 1), ("grid2k", 33), ("grid2k", 137), ("spd200", 20),
                                     ("denseblock300", 150)])
@pytest.mark.parametrize("order", ["amd", "natural", "given"])
def test_schur_variables_are_last_in_list_order_and_one_supernode(hip, name, ns, order):
    m, n, Ap, Ai, _ = sc.matrix(name)
    idx = sc.schur_set(name, ns)
    assert ns == 1 or not np.array_equal(idx, np.sort(idx)), "the list is meant to be unsorted"
    inter, _ = sc.split(n, idx)
    kw = {"amd": dict(order=hip.ORDER_AMD), "natural": dict(order=hip.ORDER_NATURAL),
          "given": dict(q=inter[::-1].astype(np.int32))}[order]
    with hip.Factorization(m, n, Ap, Ai, schur=idx, **kw) as F:
        o = F.ordering()
        n1 = n - ns
        for key in ("q_amd", "q"):
            assert np.array_equal(o[key][n1:], idx), key
            assert np.array_equal(np.sort(o[key][:n1]), inter), key
        assert np.array_equal(o["pinv"][o["q"]], np.arange(n))
        if order == "natural":
            assert np.array_equal(o["q_amd"][:n1], inter)
        if order == "given":
            assert np.array_equal(o["q_amd"][:n1], inter[::-1])
        sn_ptr, sn_parent, _ = F.supernodes()
        assert sn_ptr[-2] == n1 and sn_ptr[-1] == n and sn_parent[-1] == -1
        assert np.array_equal(F.schur_info(), idx)
        info = F.info
        assert info.nnz_l == int(o["colcount"][:n1].sum())                 # eliminated columns only, borders included
        assert info.nnz_u == info.nnz_l
        assert info.max_front >= ns
        # no forest front is the Schur supernode; its slot in the schedule is the dense ns x ns front, behind its children
        sched, fr, fw, forest = _debug(hip, F)
        last = len(sn_ptr) - 2
        assert last not in set(forest.tolist())
        slot = int(np.flatnonzero(sched == last)[0])
        assert fr[slot] == ns and fw[slot] == ns
        where = np.empty(len(sched), dtype=np.int64)
        where[sched] = np.arange(len(sched))
        kids = np.flatnonzero(sn_parent == last)
        assert np.all(where[kids] < slot)
    # the flops of a Schur handle leave the Schur block out: fewer than the plain handle in the same order
    if order == "amd":
        with hip.Factorization(m, n, Ap, Ai, q=o["q"]) as P:
            assert info.flops_factor < P.info.flops_factor or ns == 1


def test_last_interior_column_does_not_join_a_single_schur_variable(hip):
    """A path ... - a - s: columns a and s satisfy the fundamental-supernode test (parent[a] = s, counts 2 and 1)."""
    n = 8
    rows, cols = [], []
    for j in range(n):
        for i in (j - 1, j, j + 1):
            if 0 <= i < n:
                rows.append(i); cols.append(j)
    Ap = np.zeros(n + 1, dtype=np.int32)
    np.add.at(Ap, np.asarray(cols) + 1, 1)
    Ap = np.cumsum(Ap).astype(np.int32)
    Ai = np.asarray(rows, dtype=np.int32)
    with hip.Factorization(n, n, Ap, Ai, order=hip.ORDER_NATURAL) as P:
        assert P.supernodes()[0][-2] < n - 1, "the plain analysis is expected to merge the end of the path"
    for order in (hip.ORDER_NATURAL, hip.ORDER_AMD):
        with hip.Factorization(n, n, Ap, Ai, order=order, schur=[n - 1]) as F:
            sn_ptr, sn_parent, _ = F.supernodes()
            assert sn_ptr[-2] == n - 1 and sn_ptr[-1] == n
            assert F.ordering()["q"][-1] == n - 1
            _, fr, fw, forest = _debug(hip, F)
            assert len(sn_ptr) - 2 not in set(forest.tolist())


@pytest.mark.parametrize("name,ns", [("toy10", 3), ("grid2k", 33), ("grid2k", 200), ("spd200", 20)])
def test_interior_order_is_amd_of_a11_bit_for_bit(hip, name, ns):
    m, n, Ap, Ai, _ = sc.matrix(name)
    idx = sc.schur_set(name, ns)
    inter, n1, Ap11, Ai11 = sc.interior_pattern(n, Ap, Ai, idx)
    with hip.Factorization(m, n, Ap, Ai, schur=idx) as F:
        q_amd = F.ordering()["q_amd"]
    assert np.array_equal(q_amd[:n1], inter[hip.csc_amd_f(1, n1, n1, Ap11, Ai11)])


def _block_diag(blocks, links):
    """Tridiagonal blocks of the given sizes on the diagonal plus symmetric entries `links`."""
    n = sum(blocks)
    pairs = set()
    off = 0
    for b in blocks:
        for j in range(b):
            pairs.add((off + j, off + j))
            if j + 1 < b:
                pairs.add((off + j, off + j + 1)); pairs.add((off + j + 1, off + j))
        off += b
    for i, j in links:
        pairs.add((i, j)); pairs.add((j, i))
    pairs = sorted(pairs, key=lambda t: (t[1], t[0]))
    Ap = np.zeros(n + 1, dtype=np.int32)
    for _, j in pairs:
        Ap[j + 1] += 1
    return n, np.cumsum(Ap).astype(np.int32), np.asarray([i for i, _ in pairs], dtype=np.int32)


def test_interior_component_that_does_not_touch_the_schur_set(hip):
    # component A = 0..5 (touches the Schur variables 12, 13), component B = 6..11 (touches nothing else)
    n, Ap, Ai = _block_diag([6, 6, 2], [(5, 12), (2, 13)])
    idx = np.array([13, 12], dtype=np.int32)
    with hip.Factorization(n, n, Ap, Ai, schur=idx) as F:
        o = F.ordering()
        sn_ptr, sn_parent, _ = F.supernodes()
        assert np.array_equal(o["q"][-2:], idx)
        assert sn_ptr[-2] == n - 2
        roots = np.flatnonzero(sn_parent == -1)
        assert len(roots) >= 2 and roots[-1] == len(sn_parent) - 1
        # the other root's columns are all of component B
        other = roots[0]
        assert set(o["q"][sn_ptr[other]:sn_ptr[other + 1]].tolist()) <= set(range(6, 12))


def test_isolated_schur_variable_is_accepted(hip):
    n, Ap, Ai = _block_diag([6, 1, 1], [(3, 7)])               # variable 6 touches nothing
    for idx in ([6], [7, 6], [6, 7]):
        with hip.Factorization(n, n, Ap, Ai, schur=idx) as F:
            assert np.array_equal(F.ordering()["q"][-len(idx):], idx)
            assert F.supernodes()[0][-2] == n - len(idx)
            assert np.array_equal(F.schur_info(), idx)


def test_schur_info_and_refusals_need_no_gpu(hip):
    m, n, Ap, Ai, _ = sc.matrix("toy10")
    lib = hip.lib()
    with hip.Factorization(m, n, Ap, Ai) as P:
        ns = C.c_int64(-5)
        assert lib.cs3_schur_info(P._h, C.byref(ns), None) == hip.CS3_ERR_STATE
        assert "Schur" in lib.cs3_last_error().decode()
    assert lib.cs3_schur_info(None, None, None) == hip.CS3_ERR_ARG
    with hip.Factorization(m, n, Ap, Ai, schur=[7, 2, 5]) as F:
        ns = C.c_int64(0)
        assert lib.cs3_schur_info(F._h, C.byref(ns), None) == 0 and ns.value == 3
        assert lib.cs3_schur_info(F._h, None, None) == 0
        # what would answer for A22 - S + I says so, before anything else is looked at
        with pytest.raises(hip.Cs3Error) as e:
            F.factors(values=False)
        assert e.value.code == hip.CS3_ERR_ARG and "Schur handle" in str(e.value)
        with pytest.raises(hip.Cs3Error) as e:
            F.updates_plan([([0], [1])])
        assert e.value.code == hip.CS3_ERR_ARG and "Schur handle" in str(e.value)
        with pytest.raises(hip.Cs3Error) as e:
            F.solve(np.ones(n))
        assert e.value.code == hip.CS3_ERR_ARG and "Schur handle" in str(e.value)
        # and the Schur calls before a factorisation are a state error
        S = np.zeros((3, 3))
        assert lib.cs3_schur_get(F._h, S.ctypes.data_as(C.POINTER(C.c_double))) == hip.CS3_ERR_STATE
        x = np.zeros(n)
        for fn in (lib.cs3_schur_fwd, lib.cs3_schur_bwd):
            assert fn(F._h, x.ctypes.data_as(C.POINTER(C.c_double)), 1) == hip.CS3_ERR_STATE


@pytest.mark.parametrize("name,batch", sc.SCHEDULE_CASES)
def test_plain_handles_keep_their_schedule(hip, name, batch):
    """The arrays were recorded at the commit before Schur handles existed (tests/golden/make_schur_fixtures.py)."""
    sched, fr, fw = sc.plain_schedule(hip, name, batch)
    tag = "%s_b%d" % (name, batch)
    with np.load(os.path.join(sc.GOLDEN, "schur_schedule.npz")) as z:
        assert np.array_equal(sched, z[tag + "_sched"])
        assert np.array_equal(fr, z[tag + "_r"])
        assert np.array_equal(fw, z[tag + "_w"])
