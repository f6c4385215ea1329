"""Selected inversion (selinv.hip, selinv.cpp) on the GPU at the edges of its chunks, slices, tiles and launch groups: the
cases of tests/selinv_edge_cases.py (pinned from the host analysis by tests/test_selinv_edge_cases_cpu.py) against the
dense inverse.  Beside the checks of tests/test_gpu_selinv.py (entries, transposed entries, diagonal, on the factors:
max |Z - Z_ref| <= 1e-10 max |Z_ref| over all extracted entries) every block Z_PP, Z_CP, Z_PC of every front is held to
the same 1e-10 relative to ITS OWN largest entry (selinv_ref.front_block_errors): Z_CP and Z_PC of these diagonally
dominant matrices are about two orders below the diagonal of Z, and a failure names the front and the block.
The reference itself is within 1e-12 of the float64 restatement by that measure (asserted on the CPU)."""
import numpy as np
import pytest

import selinv_edge_cases as se
import selinv_ref as ref
from test_gpu_selinv import _check_handle

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(name, i, symmetric):
    """(case, Z_ref) of matrix i of a case, computed once; cond_1 <= COND_MAX."""
    key = (name, i, symmetric)
    if key not in _REF:
        case = se.matrix(name, i, symmetric)
        Zref, cond = ref.dense_inverse(case[1], case[2], case[3], case[4])
        assert cond <= ref.COND_MAX, (key, cond)
        Zref.setflags(write=False)
        _REF[key] = case, Zref
    return _REF[key]


def _check_blocks(gpu, F, Zref, what, b=0):
    """Every block of every front of matrix b within BOUND of the dense inverse, relative to the block's largest entry."""
    Zl, Zu = F.inverse_on_factors(b)
    blocks = ref.front_block_errors(gpu, F, Zl, Zu, Zref)
    print("%s: %d blocks, worst %s" % (what, len(blocks), ref.worst_block(blocks)))
    bad = ["Z_%s of front %d (r = %d, w = %d): %.3e" % (blk, s, r, w, err) for s, r, w, blk, err in blocks if not err <= ref.BOUND]
    assert not bad, (what, bad)
    return Zl, Zu


def _kind(gpu, kind):
    return gpu.CS3_CHOLESKY if kind == "chol" else gpu.CS3_LU


@pytest.mark.parametrize("name,kind", se.GPU_CASES)
def test_edge_case(gpu, name, kind):
    case, Zref = _reference(name, 0, kind == "chol")
    with se.analysed(name, kind) as F:
        F.factor(case[4])
        _check_handle(gpu, F, name, case, Zref, " " + kind)
        _check_blocks(gpu, F, Zref, "%s %s" % (name, kind))
        info = F.selinv_info()
    assert info.nfronts_big == sum(se.class_of(r) == "big" for r in [f[0] for f in se.TABLE[name].fronts] + se.TABLE[name].roots)


def _same(a, b):
    return (a is None and b is None) or np.array_equal(a, b)


def _everything(gpu, F, refs, what):
    """Per matrix of a factorised handle: (Zl, Zu, entries, transposed entries, diagonal, factors), each matrix held to its
    own dense inverse by the block measure and over the extracted entries."""
    n, Ap, Ai = refs[0][0][1:4]
    Zx, Zt, d = (np.atleast_2d(a) for a in (F.inverse_entries(), F.inverse_entries(trans=True), F.inverse_diagonal()))
    assert Zx.shape == Zt.shape == (F.batch, int(Ap[n])) and d.shape == (F.batch, n)
    out = []
    for b, (_, Zref) in enumerate(refs):
        Zl, Zu = _check_blocks(gpu, F, Zref, "%s matrix %d of %d" % (what, b, F.batch) if F.batch > 1 else what, b)
        assert ref.max_error(Zx[b], ref.entries_of(Zref, n, Ap, Ai)) <= ref.BOUND, (what, b)
        assert ref.max_error(Zt[b], ref.entries_of(Zref, n, Ap, Ai, True)) <= ref.BOUND, (what, b)
        assert ref.max_error(d[b], Zref.diagonal()) <= ref.BOUND, (what, b)
        out.append((Zl, Zu, Zx[b], Zt[b], d[b], F.factors(b)))
    return out


@pytest.mark.parametrize("kind", ["lu", "chol"])
@pytest.mark.parametrize("name", ["two_trees", "mixed", "mixed0"])
def test_batch_of_two_with_unequal_fronts(gpu, name, kind):
    """Two matrices with values of their own on one handle (work_stride, wk and z_stride with fronts of unequal sizes): each
    against its own inverse by the block measure; each the same bits as in the OTHER slot of a second handle that holds the
    two in reverse order; and each the same bits as on a handle of its own.

    "Same factors, same bits" is the property, and the last comparison has a premise: a single matrix factorises its small
    fronts in the bottom forest, a batch does not, and their factors differ in the last place (measured on `mixed`, LU:
    11 of 50 621 entries of U by 2.8e-17 at the front (19, 6) and its parent, and with them 3 entries of Z_PC by 2e-19;
    neither pool layout can import the other's panels).  So the handle of its own is compared bit for bit on the cases
    without small fronts (two_trees, mixed0: the factors are asserted to be the same bits first); on `mixed` it is held to
    the dense inverse, and what differs is printed."""
    sym = kind == "chol"
    refs = [_reference(name, i, sym) for i in (0, 1)]
    AX = np.stack([case[4] for case, _ in refs])
    assert not np.array_equal(AX[0], AX[1])
    with se.analysed(name, kind, batch=2) as F:
        F.factor(AX)
        got = _everything(gpu, F, refs, "%s %s" % (name, kind))
    with se.analysed(name, kind, batch=2) as F:
        F.factor(AX[::-1])
        swapped = _everything(gpu, F, refs[::-1], "%s %s reversed" % (name, kind))[::-1]
    for b in (0, 1):
        assert all(_same(x, y) for x, y in zip(got[b][5], swapped[b][5])), "matrix %d: factors differ between the slots" % b
        for what, x, y in zip(("Z on L", "Z on U", "entries", "transposed entries", "diagonal"), got[b], swapped[b]):
            assert _same(x, y), "matrix %d: %s differ between slot %d and slot %d" % (b, what, b, 1 - b)
        with se.analysed(name, kind) as F1:
            F1.factor(AX[b])
            alone = _everything(gpu, F1, refs[b:b + 1], "%s %s matrix %d alone" % (name, kind, b))[0]
        equal = [all(_same(x, y) for x, y in zip(got[b][5], alone[5]))] + [_same(x, y) for x, y in zip(got[b][:5], alone[:5])]
        print("matrix %d alone against the batch, the same bits: factors %s, Z on L %s, Z on U %s, entries %s, transposed %s, "
              "diagonal %s" % ((b,) + tuple(equal)))
        if se.TABLE[name].rest == 0:                        # no front of the wave class below a root: nothing for the forest
            assert equal[0], "matrix %d: factors differ from the same matrix alone" % b
            assert all(equal[1:]), "matrix %d differs from the same matrix alone" % b


@pytest.mark.parametrize("kind", ["lu", "chol"])
def test_two_runs_give_the_same_bits(gpu, kind):
    """`mixed`: surplus workgroups in the gather role and returning tiles race with nothing."""
    case, Zref = _reference("mixed", 0, kind == "chol")
    with se.analysed("mixed", kind) as F:
        F.factor(case[4])
        F.selinv()
        first = F.inverse_on_factors() + (F.inverse_entries(), F.inverse_diagonal())
        for _ in range(2):
            F.selinv()
            again = F.inverse_on_factors() + (F.inverse_entries(), F.inverse_diagonal())
            for a, b in zip(first, again):
                assert (a is None and b is None) or np.array_equal(a, b)
        _check_blocks(gpu, F, Zref, "mixed %s, third run" % kind)


@pytest.mark.parametrize("n", se.GETTER_ORDERS)
def test_getter_counts_at_a_workgroup_edge(gpu, n):
    """k_selinv_gather with count = n and count = nnz = 3 n - 2 around its 256 threads, blockIdx.y * count with a batch of 2."""
    cases = [se.tridiagonal(n, i) for i in (0, 1)]
    _, _, Ap, Ai, _ = cases[0]
    assert int(Ap[n]) == 3 * n - 2
    with gpu.Factorization(n, n, Ap, Ai, gpu.CS3_LU, gpu.ORDER_AMD, batch=2) as F:
        F.factor(np.stack([c[4] for c in cases]))
        d, Zx, Zt = F.inverse_diagonal(), F.inverse_entries(), F.inverse_entries(trans=True)
        assert d.shape == (2, n) and Zx.shape == Zt.shape == (2, 3 * n - 2)
        for b in (0, 1):
            Zref, cond = ref.dense_inverse(n, Ap, Ai, cases[b][4])
            assert cond <= ref.COND_MAX
            errs = (ref.max_error(d[b], Zref.diagonal()), ref.max_error(Zx[b], ref.entries_of(Zref, n, Ap, Ai)),
                    ref.max_error(Zt[b], ref.entries_of(Zref, n, Ap, Ai, True)))
            print("n = %d matrix %d: diagonal %.3e entries %.3e transposed %.3e" % ((n, b) + errs))
            assert max(errs) <= ref.BOUND, (b, errs)
            # entry for entry: a getter that reads the other matrix's Z, or one entry beside its own, is far off
            assert np.abs(d[b] - Zref.diagonal()).max() <= ref.BOUND * np.abs(Zref.diagonal()).min()
            _check_blocks(gpu, F, Zref, "tridiagonal %d matrix %d" % (n, b), b)
        assert np.abs(d[0] - d[1]).max() > 1e-3
