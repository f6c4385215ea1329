"""Extra-precise refinement on the GPU (cs3_residual_xp*, cs3_refine_xp*, csrc/refine_xp.hip) on the cases of
tests/xp_cases.py: the doubled residual bit for bit against tests/xp_ref.py, the refined solutions against the 80-digit
solutions of tests/golden/xp_refs.npz, the per-system control and the handle's contracts.

The forward-error threshold 2^-52 is derived, not measured: the returned head is the rounding of a head-plus-tail whose own
error is orders of magnitude smaller (the tail errors are printed by test_accuracy; DESIGN.md section 7 records them)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import xp_cases as xc
import xp_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xp_refs.npz")
CONVERGED = ["chain_4_8", "chain_4_11", "chain_3_13", "chain_3_15", "chain_3_17", "chain_4_11_t", "chain_spd", "permuted",
             "perturbed", "stale", "n1"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def refs():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return xc.refinement_cases()


@pytest.fixture(scope="module")
def held(gpu, cases):
    """One factorised handle per (case, batch), shared by the tests of this module."""
    made = {}

    def get(name, batch=1):
        if (name, batch) not in made:
            case = cases[name]
            kind = gpu.CS3_CHOLESKY if case.kind == "chol" else gpu.CS3_LU
            F = gpu.Factorization(case.n, case.n, case.Ap, case.Ai, kind=kind, order=gpu.ORDER_NATURAL, batch=batch,
                                  match_values=case.Ax if case.kind == "matched" else None)
            if name == "perturbed":
                F.set_perturbation(xc.perturbed()[1])
                F.factor(np.tile(case.Ax, (batch, 1)))
                assert (F.perturbed() >= 1).all(), "the delta of the case must replace a pivot"
            else:
                F.factor(np.tile(case.Ax0, (batch, 1)))
            made[(name, batch)] = F
        return made[(name, batch)]

    yield get
    for F in made.values():
        F.close()


def _true_error(x, xh):
    return float(np.abs(x - xh).max() / np.abs(xh).max())


def _tail_error(x, xt, xh, xth):
    """max |(x + xt) - (xh + xth)| / max |xh| in exact arithmetic."""
    num = max(abs(Fraction(float(a)) + Fraction(float(b)) - Fraction(float(c)) - Fraction(float(d)))
              for a, b, c, d in zip(x, xt, xh, xth))
    return float(num / Fraction(float(np.abs(xh).max())))


# ---- 1. the residual, bit for bit -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_handles(gpu):
    """Analysed (not factorised) handles by name: the residual needs no factors."""
    made = {}

    def get(name, n, Ap, Ai, batch=1):
        if (name, batch) not in made:
            made[(name, batch)] = gpu.Factorization(n, n, Ap, Ai, order=gpu.ORDER_NATURAL, batch=batch)
        return made[(name, batch)]

    yield get
    for F in made.values():
        F.close()


def _check_residual(F, n, Ap, Ai, Ax, b, x, xt, trans):
    r, s = F.residual_xp(Ax, b, x, xt, trans=trans)
    want_r, want_s = xp_ref.resid_xp(n, Ap, Ai, Ax, b, x, xt, trans)
    assert _same_bits(r, want_r) and _same_bits(s, want_s)
    return r, s


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_residual_bits(plain_handles, k, tail, trans):
    case = xc.chain(3, 15)
    rng = np.random.default_rng(100 + k)
    F = plain_handles("chain_3_15", case.n, case.Ap, case.Ai)
    x = rng.standard_normal((case.n, k)) * 10.0 ** rng.integers(-3, 4, (case.n, k))
    b = rng.standard_normal((case.n, k))
    xt = x * 2.0 ** -53 * rng.standard_normal((case.n, k)) if tail else None
    r, _ = _check_residual(F, case.n, case.Ap, case.Ai, case.Ax, b, x, xt, trans)
    if tail:        # the tail is not lost: it moves the residual
        assert not _same_bits(r, F.residual_xp(case.Ax, b, x, None, trans=trans)[0])


@pytest.mark.parametrize("trans", [False, True])
def test_residual_bits_arrowhead_unsorted_rows(plain_handles, trans):
    n, Ap, Ai, Ax = xc.arrowhead()
    rng = np.random.default_rng(7)
    x, b = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    xt = x * 2.0 ** -54
    _check_residual(plain_handles("arrowhead", n, Ap, Ai), n, Ap, Ai, Ax, b, x, xt, trans)


def test_residual_bits_order_one_and_batch(plain_handles):
    c1 = xc.one_by_one()
    F1 = plain_handles("n1", 1, c1.Ap, c1.Ai)
    _check_residual(F1, 1, c1.Ap, c1.Ai, c1.Ax, np.array([1.0]), np.array([1.0 / 3.0]), np.array([2.0 ** -56]), False)
    case = xc.chain(3, 15)
    F2 = plain_handles("chain_3_15", case.n, case.Ap, case.Ai, batch=2)
    rng = np.random.default_rng(8)
    AX = np.stack([case.Ax, case.Ax * (1.0 + 0.1 * rng.standard_normal(case.Ax.size))])
    X, B = rng.standard_normal((2, case.n, 3)), rng.standard_normal((2, case.n, 3))
    XT = X * 2.0 ** -53
    R, S = F2.residual_xp(AX, B, X, XT)
    for m in range(2):
        want_r, want_s = xp_ref.resid_xp(case.n, case.Ap, case.Ai, AX[m], B[m], X[m], XT[m])
        assert _same_bits(R[m], want_r) and _same_bits(S[m], want_s)


def test_residual_nan_stays_in_its_column(plain_handles):
    case = xc.chain(3, 15)
    F = plain_handles("chain_3_15", case.n, case.Ap, case.Ai)
    rng = np.random.default_rng(9)
    x, b = rng.standard_normal((case.n, 3)), rng.standard_normal((case.n, 3))
    clean_r, clean_s = F.residual_xp(case.Ax, b, x)
    x[7, 1] = np.nan
    r, s = F.residual_xp(case.Ax, b, x)
    assert np.isnan(r[:, 1]).any() and np.isnan(s[:, 1]).any()
    assert np.array_equal(np.isnan(r), np.isnan(s)) and not np.isnan(r[:, [0, 2]]).any()
    assert _same_bits(r[:, [0, 2]], clean_r[:, [0, 2]]) and _same_bits(s[:, [0, 2]], clean_s[:, [0, 2]])


def test_residual_bits_past_the_grid_cap(gpu):
    """n * k just above grid_cap * block + block + 1: every thread takes a second grid pass, the last a partial one."""
    lim = gpu.refine_xp_limits()
    base, k = xc.chain(4, 8), 17
    reps = -(-(lim.grid_cap * lim.block + lim.block + 1) // (base.n * k))
    n = reps * base.n
    assert lim.grid_cap * lim.block + lim.block + 1 <= n * k < 2 * lim.grid_cap * lim.block
    nnz = int(base.Ap[-1])
    Ap = np.concatenate([[0], (base.Ap[1:][None, :] + nnz * np.arange(reps)[:, None]).reshape(-1)]).astype(np.int32)
    Ai = (base.Ai[None, :] + base.n * np.arange(reps)[:, None]).reshape(-1).astype(np.int32)
    Ax = np.tile(base.Ax, reps) * (1.0 + 0.01 * np.random.default_rng(10).standard_normal(reps * nnz))
    rng = np.random.default_rng(11)
    x, b = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    xt = x * 2.0 ** -53
    with gpu.Factorization(n, n, Ap, Ai, order=gpu.ORDER_NATURAL) as F:
        _check_residual(F, n, Ap, Ai, Ax, b, x, xt, False)
        _check_residual(F, n, Ap, Ai, Ax, b, x, None, True)


# ---- 2. accuracy ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CONVERGED)
def test_accuracy(held, cases, refs, name):
    case, F = cases[name], held(name)
    x, info = F.refine_xp(case.Ax, case.b, trans=case.trans, want_tail=True)
    xh, xth = refs[name + "_xh"], refs[name + "_xt"]
    err = _true_error(x, xh)
    etail, bound = _tail_error(x, info["xt"], xh, xth), 2.0 ** 6 * float(refs[name + "_etail"]) + 2.0 ** -100
    print("%-13s iters %d flag %d rate %.2e ferr %.2e berr %.2e true %.2e tail %.2e (bound %.2e)"
          % (name, info["iters"][0], info["flag"][0], info["rate"][0], info["ferr"][0], info["berr"][0], err, etail, bound))
    assert info["flag"][0] == 1 and 1 <= info["iters"][0] <= 10
    assert err <= EPS
    assert info["ferr"][0] >= err and np.isfinite(info["ferr"][0])
    assert etail <= bound
    assert _same_bits(info["berr"], xp_ref.berr(case.n, case.Ap, case.Ai, case.Ax, case.b, x, case.trans))
    assert info["berr"][0] <= 4 * EPS


def test_beyond_one_over_eps(held, cases, refs):
    case, F = cases["chain_2_20"], held("chain_2_20")
    x, info = F.refine_xp(case.Ax, case.b)
    err = _true_error(x, refs["chain_2_20_xh"])
    print("chain_2_20: iters %d flag %d rate %.2e ferr %.2e true %.2e" % (info["iters"][0], info["flag"][0], info["rate"][0],
                                                                         info["ferr"][0], err))
    assert info["flag"][0] == 0 and info["iters"][0] == 10
    assert np.isfinite(info["ferr"][0]) and info["ferr"][0] >= err
    assert _same_bits(info["berr"], xp_ref.berr(case.n, case.Ap, case.Ai, case.Ax, case.b, x))


# ---- 3. control -------------------------------------------------------------------------------------------------------

def test_no_iterations(held, cases):
    case, F = cases["chain_3_13"], held("chain_3_13")
    x0 = F.solve(case.b)
    x, info = F.refine_xp(case.Ax, case.b, x=x0, max_iters=0)
    assert _same_bits(x, x0)
    assert info["iters"][0] == 0 and info["flag"][0] == 0 and info["ferr"][0] == np.inf
    assert _same_bits(info["berr"], xp_ref.berr(case.n, case.Ap, case.Ai, case.Ax, case.b, x0))


def test_zero_column(held, cases, refs):
    case, F = cases["chain_4_8"], held("chain_4_8")
    b = np.stack([case.b, np.zeros(case.n), 2.0 * case.b], axis=1)
    x, info = F.refine_xp(case.Ax, b)
    assert not x[:, 1].any()
    assert (info["iters"][1], info["flag"][1], info["ferr"][1], info["berr"][1]) == (1, 1, 0.0, 0.0)
    assert list(info["flag"]) == [1, 1, 1]
    assert _true_error(x[:, 0], refs["chain_4_8_xh"]) <= EPS and _true_error(x[:, 2], 2.0 * refs["chain_4_8_xh"]) <= EPS


def test_batch_of_two_freezes_the_finished_system(gpu):
    n, Ap, Ai, AX, B = xc.padded_pair()
    with gpu.Factorization(n, n, Ap, Ai, order=gpu.ORDER_NATURAL, batch=2) as F2, \
            gpu.Factorization(n, n, Ap, Ai, order=gpu.ORDER_NATURAL) as F1:
        F2.factor(AX)
        F1.factor(AX[0])
        x2, info2 = F2.refine_xp(AX, B, want_tail=True)
        x1, info1 = F1.refine_xp(AX[0], B[0])
        stop = int(info2["iters"][0])
        xs, infos = F2.refine_xp(AX, B, max_iters=stop, want_tail=True)
    print("iters %s flags %s" % (info2["iters"], info2["flag"]))
    assert list(info2["flag"]) == [1, 1] and info2["iters"][0] < info2["iters"][1]
    assert _same_bits(x2[0], x1) and info1["iters"][0] == info2["iters"][0] and info1["flag"][0] == 1
    # the call cut off at the pass in which system 0 stopped: head and tail of system 0 are what the longer call returns
    # (the two batched solves of a batch differ in rounding from a batch-1 solve, so the tails are compared here)
    assert list(infos["flag"]) == [1, 0] and infos["iters"][1] == stop
    assert _same_bits(x2[0], xs[0]) and _same_bits(info2["xt"][0], infos["xt"][0])
    assert not _same_bits(x2[1], xs[1])
    for key in ("ferr", "berr", "rate"):
        assert _same_bits(info2[key][:1], infos[key][:1]), key


def test_hopeless_pair(held, cases):
    case, F = cases["hopeless"], held("hopeless")
    x, info = F.refine_xp(case.Ax, case.b)
    print("hopeless: iters %d flag %d rate %.2e ferr %s" % (info["iters"][0], info["flag"][0], info["rate"][0], info["ferr"][0]))
    assert info["flag"][0] == 2 and info["ferr"][0] == np.inf


def test_nan_right_hand_side_stays_in_its_column(held, cases, refs):
    case, F = cases["chain_4_8"], held("chain_4_8")
    b = np.stack([case.b, case.b, case.b], axis=1)
    b[5, 1] = np.nan
    x, info = F.refine_xp(case.Ax, b)
    assert list(info["flag"]) == [1, 3, 1] and np.isnan(info["ferr"][1]) and info["iters"][1] == 0
    for t in (0, 2):
        assert _true_error(x[:, t], refs["chain_4_8_xh"]) <= EPS and info["ferr"][t] == EPS


# ---- 4. contracts -----------------------------------------------------------------------------------------------------

def test_two_calls_same_bits_and_no_allocation(gpu, held, cases):
    case, F = cases["chain_3_15"], held("chain_3_15")
    b = np.stack([case.b, -3.0 * case.b], axis=1)
    first = F.refine_xp(case.Ax, b, want_tail=True)
    allocs0, _ = F.debug_alloc_counters()
    second = F.refine_xp(case.Ax, b, want_tail=True)
    allocs1, _ = F.debug_alloc_counters()
    assert allocs1 == allocs0
    assert _same_bits(first[0], second[0])
    for key in ("ferr", "berr", "rate", "xt"):
        assert _same_bits(first[1][key], second[1][key]), key
    for key in ("iters", "flag"):
        assert np.array_equal(first[1][key], second[1][key])
    # the device-pointer form gives the host form's bits
    import torch
    ax, bd, xd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (case.Ax, b, F.solve(b)))
    xtd = torch.zeros_like(xd)
    info = F.refine_xp_dev(ax.data_ptr(), bd.data_ptr(), xd.data_ptr(), k=2, xt_ptr=xtd.data_ptr())
    torch.cuda.synchronize()
    assert _same_bits(xd.cpu().numpy(), first[0]) and _same_bits(xtd.cpu().numpy(), first[1]["xt"])
    assert _same_bits(info["ferr"], first[1]["ferr"]) and _same_bits(info["berr"], first[1]["berr"])


def test_work_memory_goes_with_the_handle(gpu):
    case = xc.chain(4, 8)
    before = gpu.debug_live_device_buffers()
    F = gpu.Factorization(case.n, case.n, case.Ap, case.Ai, order=gpu.ORDER_NATURAL)
    F.factor(case.Ax)
    F.refine_xp(case.Ax, case.b)
    F.refine_xp(case.Ax, np.stack([case.b] * 5, axis=1))
    assert gpu.debug_live_device_buffers() > before
    F.close()
    assert gpu.debug_live_device_buffers() == before


def test_lusol_extra(gpu, cases, refs):
    from csparse3_amd import csc
    case = cases["chain_3_13"]
    A = csc.CscMat(case.n, case.n, indptr=case.Ap, indices=case.Ai, data=case.Ax)
    xh = refs["chain_3_13_xh"]
    plain = csc.lusol(A, case.b, order=0)
    extra = csc.lusol(A, case.b, order=0, refine="extra")
    print("lusol: plain %.2e extra %.2e" % (_true_error(plain, xh), _true_error(extra, xh)))
    assert _true_error(extra, xh) <= EPS < _true_error(plain, xh)
