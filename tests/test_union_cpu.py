"""Union plans without a GPU: the host side of the plan (cs3_union_plan_create, _info, _pattern, _offsets, _slots) against
the NumPy restatement (tests/union_ref.py), the order of the argument checks, and the claim the feature rests on -- a
matrix padded with explicit zeros to the union pattern has the solution of the unpadded one -- checked with the oracle.

Not covered: the two size limits (a member or a union of 2^31 - 1024 entries or more).  They come after the row-index
check in the stated order, so reaching them takes a valid index array of 8 GiB."""
import ctypes as C

import numpy as np
import pytest

import helpers
import union_cases as cases
import union_ref as ref

STRUCT = cases.structural_cases()


def check_plan(hip, n, patterns):
    Up, Ui, key = ref.union_pattern(n, patterns)
    with hip.UnionPlan(n, patterns) as plan:
        gp, gi = plan.pattern()
        assert gp.dtype == np.int32 and np.array_equal(gp, Up)
        assert gi.dtype == np.int32 and np.array_equal(gi, Ui)
        for j in range(n):
            assert np.all(np.diff(gi[gp[j]:gp[j + 1]]) > 0)                 # ascending, no repeats
        sizes = [int(Ap[n]) for Ap, Ai in patterns]
        assert np.array_equal(plan.offsets(), np.concatenate([[0], np.cumsum(sizes)]))
        sourced = dups = 0
        for b, (Ap, Ai) in enumerate(patterns):
            want = ref.slots(n, key, Ap, Ai)
            got = plan.slots(b)
            assert got.dtype == np.int32 and np.array_equal(got, want), "member %d" % b
            per = np.bincount(want, minlength=len(key))
            sourced += int(np.count_nonzero(per))
            dups += int(np.count_nonzero(per > 1))
        inf = plan.info
        assert (inf.n, inf.nmat, inf.nnz_union, inf.nnz_total) == (n, len(patterns), len(key), sum(sizes))
        assert inf.padded == len(patterns) * len(key) - sourced
        assert inf.dup_slots == dups
        assert inf.distinct_patterns == len({(np.asarray(Ap).tobytes(), np.asarray(Ai).tobytes()) for Ap, Ai in patterns})
        return inf


@pytest.mark.parametrize("name", sorted(STRUCT))
def test_union_and_slots_match_the_restatement(hip, name):
    n, patterns = STRUCT[name]
    inf = check_plan(hip, n, patterns)
    if name == "single_unsorted":                                           # the union of one member: its pattern, rows sorted
        Ap, Ai = patterns[0]
        Up, Ui, key = ref.union_pattern(n, patterns)
        assert np.array_equal(Up, Ap) and np.array_equal(Ui, np.concatenate([np.sort(Ai[Ap[j]:Ap[j + 1]]) for j in range(n)]))
        assert inf.padded == 0
    if name == "disjoint":
        assert inf.nnz_union == inf.nnz_total
    if name == "dup2":
        assert inf.dup_slots == 1
    if name == "dup5":
        assert inf.dup_slots == 3                                            # row 2 of column 1 five times, (0, 2) and member 1's (2, 1) twice
    if name == "six_members_three_identical":
        assert inf.distinct_patterns == 4
    if name == "many_over_three_patterns":
        assert inf.distinct_patterns == 3 and inf.nmat == 130
    if name == "empty_member":
        assert inf.padded >= inf.nnz_union


def test_the_union_does_not_depend_on_member_order(hip):
    n, patterns = STRUCT["unsorted"]
    with hip.UnionPlan(n, patterns) as a, hip.UnionPlan(n, patterns[::-1]) as b:
        assert all(np.array_equal(x, y) for x, y in zip(a.pattern(), b.pattern()))
        for k in range(len(patterns)):
            assert np.array_equal(a.slots(k), b.slots(len(patterns) - 1 - k))


def test_order_zero_follows_cs3_analyze(hip):
    """n = 0 is an empty union if cs3_analyze takes an empty matrix, else CS3_ERR_ARG."""
    h = C.c_void_p()
    Ap = np.zeros(1, dtype=np.int32)
    rc = hip.lib().cs3_analyze(hip.CS3_LU, hip.ORDER_AMD, 0, hip._pi(Ap), None, None, 1, C.byref(h))
    if rc == 0:
        hip.lib().cs3_free(h)
        inf = check_plan(hip, 0, [(Ap, np.empty(0, dtype=np.int32))] * 2)
        assert inf.nnz_union == 0 and inf.distinct_patterns == 1
    else:
        assert rc == hip.CS3_ERR_ARG
        with pytest.raises(hip.Cs3Error) as e:
            hip.UnionPlan(0, [(Ap, np.empty(0, dtype=np.int32))])
        assert e.value.code == hip.CS3_ERR_ARG


def test_the_two_restatements_agree(hip):
    rng = np.random.default_rng(3)
    for name in ("unsorted", "dup2", "dup5", "empty_member", "six_members_three_identical"):
        n, patterns = STRUCT[name]
        vals = cases.values_for(rng, patterns)
        assert np.array_equal(ref.bits(ref.embed(n, patterns, vals)), ref.bits(ref.embed_loop(n, patterns, vals))), name
    n, patterns = STRUCT["dup5"]                                            # left to right: (1e16 + 1) - 1e16 = 0, any other order 1
    vals = [np.array([5.0, 1e16, 7.0, 1.0, -1e16, 9.0, 0.0, 0.0, -0.0, 0.0]), np.array([-0.0, 0.0])]
    out = ref.embed_loop(n, patterns, vals)
    Up, Ui, key = ref.union_pattern(n, patterns)
    s = int(ref.slots(n, key, *patterns[0])[1])
    assert out[0, s] == 0.0 and out[1, s] == 0.0 and not np.signbit(out[1, s])


def _create(hip, n, nmat, Ap, Ai, out=True, null_arrays=False):
    """Raw call: Ap / Ai are lists of arrays or None (a null member pointer)."""
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    Ap, Ai = [i32(a) for a in Ap], [i32(a) for a in Ai]
    aps = (hip._i32p * max(len(Ap), 1))(*[hip._pi(a) for a in Ap])
    ais = (hip._i32p * max(len(Ai), 1))(*[hip._pi(a) for a in Ai])
    plan = C.c_void_p()
    rc = hip.lib().cs3_union_plan_create(n, nmat, None if null_arrays else aps, None if null_arrays else ais,
                                         C.byref(plan) if out else None)
    msg = hip.lib().cs3_last_error().decode()
    if rc == 0:
        hip.lib().cs3_union_plan_free(plan)
    return rc, msg


def test_argument_errors_arrive_in_the_stated_order(hip):
    good = ([0, 1, 2], [0, 1])
    # every call has the fault it is named for AND every later one of the list that can be combined with it
    calls = [
        ("null output", dict(n=-1, nmat=0, Ap=[], Ai=[], out=False, null_arrays=True)),
        ("null array of pattern pointers", dict(n=-1, nmat=0, Ap=[], Ai=[], null_arrays=True)),
        ("nmat must be >= 1", dict(n=-1, nmat=0, Ap=[None], Ai=[None])),
        ("bad order n", dict(n=-1, nmat=2, Ap=[None, good[0]], Ai=[None, good[1]])),
        ("bad order n", dict(n=2 ** 30, nmat=1, Ap=[good[0]], Ai=[good[1]])),
        ("null column pointers of member 1", dict(n=2, nmat=2, Ap=[[1, 1, 2], None], Ai=[[0, 1], [0, 1]])),
        ("Ap[0] != 0 of member 0", dict(n=2, nmat=2, Ap=[[1, 0, 2], [0, 2, 1]], Ai=[[0, 1], [0, 1]])),
        ("decreases at column 1", dict(n=2, nmat=2, Ap=[[0, 2, 1], good[0]], Ai=[None, [0, 5]])),
        ("null row indices of member 0", dict(n=2, nmat=2, Ap=[good[0], good[0]], Ai=[None, [0, 5]])),
        ("row index of member 0 out of range at entry 1", dict(n=2, nmat=2, Ap=[good[0], [0, 2, 1]], Ai=[[0, 2], [0, 1]])),
        ("row index of member 1 out of range at entry 0", dict(n=2, nmat=2, Ap=[good[0], good[0]], Ai=[[0, 1], [-1, 1]])),
    ]
    for want, kw in calls:
        rc, msg = _create(hip, **kw)
        assert rc == hip.CS3_ERR_ARG, want
        assert msg.startswith("cs3_union_plan_create: ") and want in msg, (want, msg)
    assert _create(hip, 2, 2, [good[0], good[0]], [good[1], good[1]])[0] == 0
    assert _create(hip, 2, 1, [[0, 0, 0]], [None])[0] == 0                  # no entries: no index array needed
    with pytest.raises(hip.Cs3Error) as e:
        hip.UnionPlan(2, [good, ([0, 1, 2], [0, 2])])
    assert e.value.code == hip.CS3_ERR_ARG


def test_plan_calls_refuse_null_plans_and_bad_members(hip):
    lib = hip.lib()
    assert lib.cs3_union_plan_info(None, C.byref(hip.UnionInfo())) == hip.CS3_ERR_ARG
    assert lib.cs3_union_plan_pattern(None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_plan_offsets(None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_plan_slots(None, 0, None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_upload(None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_values_dev(None, None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_values(None, None, None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_limits(None) == hip.CS3_ERR_ARG
    assert lib.cs3_union_plan_free(None) == 0
    n, patterns = STRUCT["disjoint"]
    with hip.UnionPlan(n, patterns) as plan:
        slot = np.empty(8, dtype=np.int32)
        for b in (-1, len(patterns)):
            assert lib.cs3_union_plan_slots(plan._p, b, hip._pi(slot)) == hip.CS3_ERR_ARG
        assert lib.cs3_union_plan_pattern(plan._p, None, None) == 0          # either output may be null
        if hip.device_count() < 1:                                            # the numeric calls say that there is no GPU
            with pytest.raises(hip.Cs3Error) as e:
                plan.values(cases.values_for(np.random.default_rng(0), patterns))
            assert e.value.code == hip.CS3_ERR_HIP
            assert lib.cs3_union_values_dev(plan._p, None, None, None) == hip.CS3_ERR_HIP
    lim = hip.union_limits()
    assert lim.block % 64 == 0 and lim.grid_cap >= 1 and lim.entries_per_lane in (1, 2)


def test_cscmat_union_plan_is_the_plan_of_its_patterns(hip):
    from csparse3_amd import csc as csc_mod
    n, patterns = STRUCT["empty_column_filled_by_others"]
    mats = [csc_mod.CscMat(n, n, indptr=Ap, indices=Ai, data=np.ones(len(Ai))) for Ap, Ai in patterns]
    Up, Ui, key = ref.union_pattern(n, patterns)
    with mats[0].union_plan(mats[1:]) as plan:
        assert isinstance(plan, hip.UnionPlan) and plan.nmat == len(mats)
        assert all(np.array_equal(x, y) for x, y in zip(plan.pattern(), (Up, Ui)))


def test_padding_to_the_union_does_not_change_the_solution(hip, orc):
    """The 9-member family (150 buses, 230 branches, member c without c chord edges): the oracle solves every member on
    its own pattern and on the union pattern with host-padded values; the two solutions agree within helpers.RTOL."""
    n, patterns, vals = cases.contingency_family()
    check_plan(hip, n, patterns)
    Up, Ui, key = ref.union_pattern(n, patterns)
    assert len(key) == 610 and [int(Ap[n]) for Ap, Ai in patterns] == [610 - 2 * c for c in range(9)]
    padded = ref.embed_loop(n, patterns, vals)
    worst = 0.0
    for c, ((Ap, Ai), Ax) in enumerate(zip(patterns, vals)):
        b = np.random.default_rng(200 + c).standard_normal(n)
        own = orc.csc_lusol_f(1, n, Ap, Ai, Ax, b, 1e-3)
        uni = orc.csc_lusol_f(1, n, Up, Ui, padded[c], b, 1e-3)
        worst = max(worst, helpers.rel_err(uni, own))
    print("worst relative difference, union against own pattern: %.2e" % worst)
    assert worst <= helpers.RTOL
