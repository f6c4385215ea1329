"""Schur handles on the GPU at tile, sweep-kind, chunk and batch edges: k_schur_take, the gather into a front that is
never eliminated, and the half-solves (cs3_schur_fwd / cs3_schur_bwd) through the identity left in its place.  The cases,
their references and the restated sweep plans are in tests/schur_edge_cases.py (shapes asserted from the host analysis by
tests/test_schur_edge_cases_cpu.py).

S: entry-wise,  |S - S_ref|_ij <= RTOL W_ij  with  W = |A22| + |A21| |A11^-1| |A12|  for every entry of every matrix of
every batch; Cholesky S symmetric bit for bit; LU S whose every tile differs from its transposed counterpart by more than
1e-2 W (schur_edge_cases.transposed_tile_margin), so a transposed tile cannot pass.
Half-solves: the condensed right-hand side and the full solution within RTOL (helpers.rel_err) of the dense float64
reference per matrix, and -- the factors of the Schur front being the exact identity -- the Schur rows after the backward
half-solve equal the x2 that went in, value for value.
The LDS is poisoned before the numeric calls.  The module's teardown prints the worst figures per kind."""
import ctypes as C

import numpy as np
import pytest

import schur_edge_cases as se
from helpers import RTOL, rel_err

pytestmark = pytest.mark.gpu

KINDS = ("lu", "chol")


@pytest.fixture(scope="module", autouse=True)
def poisoned(gpu):
    import torch
    lib = gpu.lib()
    lib.cs3_debug_poison_lds.argtypes = [C.c_void_p]
    assert lib.cs3_debug_poison_lds(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def worst():
    """Worst figures of the module, printed when it is done."""
    w = {}
    yield w
    for key in sorted(w):
        print("schur edges, worst %s: %.3e" % (key, w[key]))


def _note(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _new_handle(gpu, name, kind, batch):
    m, n, Ap, Ai = se.pattern(name, symmetric=kind == "chol")
    return gpu.Factorization(m, n, Ap, Ai, kind=gpu.CS3_CHOLESKY if kind == "chol" else gpu.CS3_LU, batch=batch, schur=se.schur_set(name))


def _S(F):
    return F.schur().reshape(F.batch, F.ns, F.ns)


@pytest.fixture(scope="module")
def handles(gpu):
    """One handle per (case, kind, batch), factorised with the case's values, and its S [batch, ns, ns]; shared by the tests
    that do not factorise again."""
    held = {}

    def get(name, kind, batch):
        key = (name, kind, batch)
        if key not in held:
            F = _new_handle(gpu, name, kind, batch)
            F.factor(se.values(name, batch, kind == "chol"))
            assert int(F.info.fail_col) == -1
            held[key] = (F, _S(F))
        return held[key]

    yield get
    for F, _ in held.values():
        F.close()


def _check_S(S, name, kind, variant, what, worst):
    """Every entry of every matrix of S [batch, ns, ns] against its own scale."""
    ns = se.NS[name]
    assert S.shape[1:] == (ns, ns), what
    assert np.isfinite(S).all(), what + ": non-finite entries"
    top = 0.0
    for b in range(S.shape[0]):
        ratio = se.entrywise_ratio(S[b], name, b, kind == "chol", variant)
        top = max(top, ratio)
        assert ratio <= RTOL, "%s matrix %d: max |S - S_ref| / W = %.3e > %.1e" % (what, b, ratio, RTOL)
        if kind == "chol":
            assert _bits_equal(S[b], S[b].T), "%s matrix %d: S is not symmetric bit for bit" % (what, b)
        else:
            margin = se.transposed_tile_margin(S[b], se.weight(name, b, False, variant))
            assert margin > 1e-2, "%s matrix %d: a tile of an LU case is meant to differ from its transpose (%.3e)" % (what, b, margin)
    print("%s: max |S - S_ref| / W = %.3e" % (what, top))
    _note(worst, "max |S - S_ref| / W, " + kind, top)


# ---------------------------------------------------------------------------------------------------- S, entry-wise --

S_CASES = [(name, batch) for name in se.CASES for batch in (1,) + se.S_BATCHES.get(name, ())]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,batch", S_CASES, ids=["%s-b%d" % c for c in S_CASES])
def test_schur_complement_entrywise(gpu, handles, worst, name, batch, kind):
    F, S = handles(name, kind, batch)
    assert S.shape == (batch, se.NS[name], se.NS[name]) and int(F.info.fail_col) == -1
    assert np.array_equal(F.schur_info(), se.schur_set(name))
    _check_S(S, name, kind, 0, "%s %s batch %d" % (name, kind, batch), worst)
    if batch > 1:                                                  # every matrix with values of its own
        assert not _bits_equal(S[0], S[batch - 1])


# ----------------------------------------------------------------------------------------------------------- stale S --

@pytest.mark.parametrize("name,kind,batch", [("s65", "chol", 1), ("s65", "chol", 7), ("s257", "lu", 1)])
def test_second_factorisation_rewrites_every_tile(gpu, worst, name, kind, batch):
    """A tile of S that the second factorisation did not write would keep the first matrix's values."""
    sym = kind == "chol"
    v0, v1 = se.values(name, batch, sym), se.values(name, batch, sym, variant=1)
    what = "%s %s batch %d" % (name, kind, batch)
    with _new_handle(gpu, name, kind, batch) as F:
        S0 = _S(F.factor(v0))
        _check_S(S0, name, kind, 0, what + " first", worst)
        S1 = _S(F.factor(v1))
        assert int(F.info.fail_col) == -1
    _check_S(S1, name, kind, 1, what + " second", worst)
    assert (S0 != S1).all(), "entries of the first S survived"
    with _new_handle(gpu, name, kind, batch) as F2:
        assert _bits_equal(_S(F2.factor(v1)), S1), "a fresh handle gives other bits"


# ------------------------------------------------------------------------------------------------------- half-solves --

def _round_trip(F, S, idx, B, k):
    """forward on the device, x2 = solve(S, g) on the host, backward on the device.  B [batch, n, k] -> (Y, Z, X)."""
    import torch
    sh = torch.cuda.current_stream().cuda_stream
    d = torch.from_numpy(B.copy()).to("cuda:0")
    F.schur_forward_dev(d.data_ptr(), k, sh)
    Y = d.cpu().numpy()
    Z = Y.copy()
    for b in range(F.batch):
        Z[b, idx] = np.linalg.solve(S[b], Y[b, idx])
    d2 = torch.from_numpy(Z).to("cuda:0")
    F.schur_backward_dev(d2.data_ptr(), k, sh)
    return Y, Z, d2.cpu().numpy()


def _check_round_trip(name, kind, variant, B, Y, Z, X, what, worst, tag):
    idx = se.schur_set(name)
    assert np.isfinite(Y).all() and np.isfinite(X).all(), what
    for b in range(B.shape[0]):
        want_g, want_x = se.half_solve_reference(name, b, kind == "chol", B[b], variant)
        e_g, e_x = rel_err(Y[b, idx], want_g), rel_err(X[b], want_x)
        _note(worst, "half-solve %s, condensed rhs" % tag, e_g)
        _note(worst, "half-solve %s, solution" % tag, e_x)
        assert e_g <= RTOL, "%s matrix %d: condensed right-hand side %.3e" % (what, b, e_g)
        assert e_x <= RTOL, "%s matrix %d: solution %.3e" % (what, b, e_x)
        # the Schur front holds the exact identity: 1.0 * x2 + 0.0 * (finite values) is x2
        assert Z[b, idx].all() and np.array_equal(X[b, idx], Z[b, idx]), \
            "%s matrix %d: the backward half-solve changed the Schur rows (a stale entry in the front or its inverted blocks)" % (what, b)


HALF = [(name, pair) for name in se.HALF_CASES for pair in se.half_pairs(name)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,pair", HALF, ids=["%s-b%d-k%d" % ((c,) + p) for c, p in HALF])
def test_half_solves(gpu, handles, worst, name, pair, kind):
    batch, k = pair
    F, S = handles(name, kind, batch)
    pl = se.sweep_plan(se.NS[name], batch, k)
    B = np.random.default_rng(1000 * batch + k).standard_normal((batch, F.n, k))
    Y, Z, X = _round_trip(F, S, se.schur_set(name), B, k)
    what = "%s %s batch %d k %d (%s / %s)" % (name, kind, batch, k, pl.kind, pl.path)
    _check_round_trip(name, kind, 0, B, Y, Z, X, what, worst, "%s / %s" % (pl.kind, pl.path))


@pytest.mark.parametrize("name,kind,pair", [("s137", "lu", (2, 3)), ("s65", "chol", (7, 1))])
def test_host_forms_give_the_device_bits(gpu, handles, name, kind, pair):
    batch, k = pair
    F, S = handles(name, kind, batch)
    B = np.random.default_rng(5).standard_normal((batch, F.n, k))
    Y, Z, X = _round_trip(F, S, se.schur_set(name), B, k)
    assert _bits_equal(F.schur_forward(B), Y)
    assert _bits_equal(F.schur_backward(Z), X)


@pytest.mark.parametrize("name,kind,pair", [("s137", "lu", (2, 3)), ("s65", "chol", (16, 1))])
def test_no_allocation_on_a_repeated_call(gpu, handles, name, kind, pair):
    import torch
    batch, k = pair
    F, _ = handles(name, kind, batch)
    sh = torch.cuda.current_stream().cuda_stream
    d = torch.from_numpy(np.random.default_rng(6).standard_normal((batch, F.n, k))).to("cuda:0")
    F.schur_forward_dev(d.data_ptr(), k, sh)
    F.schur_backward_dev(d.data_ptr(), k, sh)
    torch.cuda.synchronize()
    before = F.debug_alloc_counters()
    F.schur_forward_dev(d.data_ptr(), k, sh)
    F.schur_backward_dev(d.data_ptr(), k, sh)
    after = F.debug_alloc_counters()
    torch.cuda.synchronize()
    assert after == before, (before, after)


# ---------------------------------------------------------------------------- half-solves across a refactorisation --

@pytest.mark.parametrize("name,kind,batch", [("s137", "lu", 1), ("s65", "chol", 1), ("s65", "lu", 16)])
def test_half_solves_after_a_refactorisation(gpu, worst, name, kind, batch):
    """With 16 right-hand sides or more the sweeps read inverted diagonal blocks, rebuilt only when a factorisation has
    reset them: factor, sweep, factor other values, sweep -- against the second matrix and a fresh handle."""
    sym = kind == "chol"
    idx = se.schur_set(name)
    v0, v1 = se.values(name, batch, sym), se.values(name, batch, sym, variant=1)
    what = "%s %s batch %d" % (name, kind, batch)
    with _new_handle(gpu, name, kind, batch) as F, _new_handle(gpu, name, kind, batch) as F2:
        B = np.random.default_rng(16).standard_normal((batch, F.n, 16))
        S0 = _S(F.factor(v0))
        _check_round_trip(name, kind, 0, B, *_round_trip(F, S0, idx, B, 16), what + " first, k 16", worst, "refactorised")
        S1 = _S(F.factor(v1))
        Y, Z, X = _round_trip(F, S1, idx, B, 16)
        _check_round_trip(name, kind, 1, B, Y, Z, X, what + " second, k 16", worst, "refactorised")
        S2 = _S(F2.factor(v1))
        assert _bits_equal(S2, S1)
        Y2, _, X2 = _round_trip(F2, S2, idx, B, 16)
        assert _bits_equal(Y2, Y) and _bits_equal(X2, X), "a fresh handle gives other bits"
        B1 = np.random.default_rng(17).standard_normal((batch, F.n, 1))
        _check_round_trip(name, kind, 1, B1, *_round_trip(F, S1, idx, B1, 1), what + " second, k 1", worst, "refactorised")
