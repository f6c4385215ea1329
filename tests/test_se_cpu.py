"""What the GPU tests of the state estimation rest on, checked without a GPU: the NumPy restatement (se_ref.py) against
definitions, the plan's host side (cs3_se_plan_create needs no device) against the restatement, every refusal in the
documented order, and the properties of the cases (se_cases.py) that the GPU tests take for granted."""
import ctypes as C

import numpy as np
import pytest

import quad_ref
import se_cases as sc
import se_ref as R
from csparse3_amd import csc_hip as hip


def _plan(case):
    return hip.StateEstPlan(case["n"], case["Yp"], case["Yi"], case["ref"], case["end_from"], case["end_to"], case["kind"], case["where"])


def _h(P, case, x):
    na = P["na"]
    va = np.zeros(P["n"])
    va[P["sbus"][:na]] = x[:na]
    return R.measure_ref(P, case["Yz"], case["Ye"], np.zeros(P["m"]), x[na:], va)["h"]


@pytest.mark.parametrize("key", sc.EVERY)
def test_jacobian_ref_against_central_differences(key):
    """'To 1e-6 relative' is read per measurement row: a difference quotient of row i may miss H by 1e-6 of the largest
    entry of that row, plus the quotient's own rounding, 4 eps (1 + |h_i|) / step with step = 1e-5 (h is evaluated twice,
    each to about 2 eps of the sum of its terms).  Every column of H where there are at most 600 of them; else 8 random
    sign vectors, where a row's tolerance is that of its entries added up."""
    case, P = sc.case_of(key), sc.plan_of(key)
    vm, va = sc.moved_voltages(case)
    Hr, _ = R.jacobian_ref(P, case["Yz"], case["Ye"], vm, va)
    x0, step, ns = R.state_of(P, vm, va), 1e-5, P["ns"]
    rowmax = np.zeros(P["m"])
    np.maximum.at(rowmax, P["e_row"], np.abs(Hr))
    floor = 4 * R.EPS * (1.0 + np.abs(_h(P, case, x0))) / step
    if ns <= 600:
        H = R.dense_h(P, Hr)
        for j in range(ns):
            e = np.zeros(ns); e[j] = step
            fd = (_h(P, case, x0 + e) - _h(P, case, x0 - e)) / (2 * step)
            assert (np.abs(fd - H[:, j]) <= 1e-6 * rowmax + floor).all(), (key, j)
    else:
        rng = np.random.default_rng(0)
        count = np.diff(P["Hrp"])
        for _ in range(8):
            v = rng.choice([-1.0, 1.0], size=ns)
            Hv = np.bincount(P["e_row"], weights=Hr * v[P["Hrj"]], minlength=P["m"])
            fd = (_h(P, case, x0 + step * v) - _h(P, case, x0 - step * v)) / (2 * step)
            assert (np.abs(fd - Hv) <= 1e-6 * rowmax * count + floor).all(), key


def test_the_branch_ends_of_se_ac_case_are_the_branches_of_y():
    """yft = -y is the off-diagonal entry of Y, at both ends of every branch; the diagonal holds every yff and the shunt."""
    from csparse3_amd import synth
    for key, args in (("ac169", sc.AC_SIZE + (169,)), ("ac_large", sc.AC_LARGE)):
        case = sc.case_of(key)
        n = case["n"]
        Y = np.zeros((n, n), dtype=np.complex128)
        Y[case["Yi"], np.repeat(np.arange(n), np.diff(case["Yp"]))] = case["Yz"]
        f, t = case["end_from"], case["end_to"]
        assert np.array_equal(Y[f, t], case["Ye"][:, 1]) and np.array_equal(Y[t, f], case["Ye"][:, 1])
        assert np.array_equal(case["Ye"][:, 0], -case["Ye"][:, 1])
        assert np.count_nonzero(Y) == n + len(f)
        _, Ap, Ai, Az = synth.ybus(*args)
        assert np.array_equal(Ap, case["Yp"]) and np.array_equal(Ai, case["Yi"]) and np.array_equal(Az, case["Yz"])


def test_measure_ref_is_the_generators_h():
    for key in ("ac169", "both_ends", "no_ends", "one_sided"):
        case, P = sc.case_of(key), sc.plan_of(key)
        h = R.measure_ref(P, case["Yz"], case["Ye"], case["z"], case["vm"], case["va"])
        assert np.abs(h["r"]).max() <= 1e-12 * max(1.0, np.abs(case["z"]).max()), key     # noise-free: z = h(x*)


@pytest.mark.parametrize("key", sc.EVERY)
def test_plan_getters_against_the_restatement(key):
    case, P = sc.case_of(key), sc.plan_of(key)
    with _plan(case) as plan:
        pat, maps, info = plan.pattern(), plan.maps(), plan.info
    for got, want in (("Hp", "Hp"), ("Hi", "Hi"), ("Rp", "Hrp"), ("Rj", "Hrj")):
        assert np.array_equal(pat[got], P[want]), (key, got)
    for name in ("cpos", "upos_a", "upos_m"):
        assert np.array_equal(maps[name], P[name]), (key, name)
    assert (info.n, info.nnz_y, info.nref, info.na, info.ns, info.ne, info.m, info.nnz_h) == \
        (P["n"], P["nnz"], len(case["ref"]), P["na"], P["ns"], P["ne"], P["m"], P["nnz_h"])
    assert [info.kind0, info.kind1, info.kind2, info.kind3, info.kind4] == np.bincount(case["kind"], minlength=5).tolist()
    rows, cols = np.diff(P["Rp"]), np.diff(P["Hp"])
    L = sc.limits()
    assert (info.max_row, info.max_col) == (rows.max(), cols.max())
    assert (info.rows_wave, info.cols_wave, info.nnz_g) == ((rows > L["wave_row"]).sum(), (cols > L["wave_col"]).sum(), 0)
    # inside a column of H the measurements ascend; cpos is a permutation
    for j in np.flatnonzero(cols > 1)[:50]:
        assert (np.diff(P["Hi"][P["Hp"][j]:P["Hp"][j + 1]]) >= 0).all()
    assert np.array_equal(np.sort(maps["cpos"]), np.arange(P["nnz_h"]))


def test_the_cases_sit_where_their_names_say():
    L = sc.limits()
    assert hip.se_limits().block == 256 and L["grid_cap"] * L["block"] + 1 == sc.plan_of("grid_edge")["nnz_h"]
    for key in sc.STARS + ["star_col63", "star_col64", "star_col65"]:
        case, P = sc.case_of(key), sc.plan_of(key)
        cols = np.diff(P["Hp"])
        assert np.diff(P["Rp"])[0] == case["hub_row"] == (int(key[8:]) if key.startswith("star_row") else case["n"])
        hub = [P["upos_m"][0]] + ([P["upos_a"][0]] if P["upos_a"][0] >= 0 else [])
        assert cols[hub].tolist() == [case["hub_mag_col"]] + ([case["hub_angle_col"]] if len(hub) == 2 else [])
        assert (P["upos_a"][0] < 0) == key.startswith("star_row") and case["hub_mag_col"] > L["wave_col"] - 2
        assert sorted(set(np.delete(cols, hub))) == [4, 5]
    assert [sc.case_of("star_col%d" % c)["hub_mag_col"] for c in (63, 64, 65)] == [L["wave_col"] - 1, L["wave_col"], L["wave_col"] + 1]
    for m in (255, 256, 257):
        assert sc.plan_of("chain_m%d" % m)["m"] == m and sc.plan_of("chain_nnz%d" % m)["nnz_h"] == m
    assert sc.plan_of("ac_large")["n"] == 120 and sc.plan_of("two_buses")["n"] == 2 and sc.plan_of("no_ends")["ne"] == 0
    assert len(sc.case_of("two_refs")["ref"]) == 2
    assert [int(sc.case_of(k)["ref"][0]) for k in ("ref_first", "ref_middle", "ref_last")] == [0, 7, 14]
    rep = sc.case_of("repeated")
    assert np.array_equal(rep["kind"][0::2], rep["kind"][1::2]) and np.array_equal(rep["where"][0::2], rep["where"][1::2])
    assert (np.diff(sc.case_of("unsorted")["Yi"][:3]) < 0).any()
    one = sc.case_of("one_sided")
    dense = np.zeros((one["n"], one["n"]), dtype=bool)
    dense[one["Yi"], np.repeat(np.arange(one["n"]), np.diff(one["Yp"]))] = True
    assert (dense != dense.T).any()
    both = sc.case_of("both_ends")
    flows = set(both["where"][both["kind"] == 3].tolist())
    assert any(k + (len(both["end_from"]) // 2) in flows for k in flows)
    for key in ("flows_and_magnitudes", "injections_one_magnitude"):
        kinds = set(sc.case_of(key)["kind"].tolist())
        assert kinds == ({0, 3, 4} if key == "flows_and_magnitudes" else {0, 1, 2})
    assert (sc.case_of("injections_one_magnitude")["kind"] == 0).sum() == 1
    un = sc.plan_of("unobservable")
    assert (np.diff(un["Hp"]) == 0).sum() == 2                      # the pendant bus: its angle and its magnitude


# ---- the refusals of cs3_se_plan_create, in the documented order

def _create(**over):
    """cs3_se_plan_create on a small valid case with some arguments replaced.  -> (rc, message)."""
    base = sc.case_of("both_ends")
    a = dict(n=base["n"], Yp=base["Yp"], Yi=base["Yi"], nref=1, ref=base["ref"], ne=len(base["end_from"]), end_from=base["end_from"],
             end_to=base["end_to"], m=len(base["kind"]), kind=base["kind"], where=base["where"], order=hip.ORDER_AMD, out=True)
    a.update(over)
    ptr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    handle = C.c_void_p()
    rc = hip.lib().cs3_se_plan_create(a["n"], ptr(a["Yp"]), ptr(a["Yi"]), a["nref"], ptr(a["ref"]), a["ne"], ptr(a["end_from"]),
                                      ptr(a["end_to"]), a["m"], ptr(a["kind"]), ptr(a["where"]), a["order"],
                                      C.byref(handle) if a["out"] else None)
    msg = hip.lib().cs3_last_error().decode() if rc else ""
    if rc == 0:
        hip.lib().cs3_se_plan_free(handle)
    return rc, msg


def _changed(key, index, value):
    a = np.array(sc.case_of("both_ends")[key], dtype=np.int32)
    a[index] = value
    return a


def _no_diagonal():
    """both_ends without the stored diagonal of bus 9, and an injection row there."""
    base = sc.case_of("both_ends")
    cols = np.repeat(np.arange(base["n"]), np.diff(base["Yp"]))
    keep = ~((cols == 9) & (base["Yi"] == 9))
    Yp = np.concatenate([[0], np.cumsum(np.bincount(cols[keep], minlength=base["n"]))])
    return dict(Yp=Yp, Yi=base["Yi"][keep], kind=_changed("kind", 0, 1), where=_changed("where", 0, 9))


def _faults():
    """(name, arguments, fragment of the message), in the documented order of the checks."""
    base = sc.case_of("both_ends")
    n, ne = base["n"], len(base["end_from"])
    twice = np.array(base["Yi"], dtype=np.int32)
    twice[1] = twice[0]                                              # column 0 holds its first row twice
    return [
        ("null output", dict(out=False), "null output"),
        ("null Yp", dict(Yp=None), "null column pointers"),
        ("null ref", dict(ref=None), "null reference list"),
        ("null ends", dict(end_to=None), "null branch-end table"),
        ("null rows", dict(kind=None), "null measurement list"),
        ("n", dict(n=-1), "bad order n"),
        ("Yp[0]", dict(Yp=_changed("Yp", 0, 1)), "Yp[0] != 0"),
        ("Yp decreases", dict(Yp=_changed("Yp", 2, 0)), "Yp decreases"),
        ("null Yi", dict(Yi=None), "null row indices"),
        ("row range", dict(Yi=_changed("Yi", 3, n)), "row index out of range"),
        ("order", dict(order=7), "order must be"),
        ("twice", dict(Yi=twice), "stored twice"),
        ("nref", dict(nref=0), "nref < 1"),
        ("ref range", dict(ref=[n]), "ref[0] out of range"),
        ("ref repeats", dict(nref=2, ref=[3, 3]), "ref[1] repeats"),
        ("ne", dict(ne=-1), "bad number of branch ends"),
        ("end range", dict(end_from=_changed("end_from", 2, -1)), "branch end 2 out of range"),
        ("from == to", dict(end_to=_changed("end_to", 4, base["end_from"][4])), "from == to"),
        ("m", dict(m=0), "m < 1"),
        ("kind", dict(kind=_changed("kind", 5, 5)), "kind[5] outside 0..4"),
        ("where bus", dict(kind=_changed("kind", 0, 0), where=_changed("where", 0, n)), "where[0] out of range for a bus"),
        ("where end", dict(where=_changed("where", 0, ne)), "where[0] out of range for a branch end"),
        ("diagonal", _no_diagonal(), "no stored diagonal"),
    ]


def test_every_refusal_of_plan_create():
    assert _create() == (0, "")
    for name, args, fragment in _faults():
        rc, msg = _create(**args)
        assert rc == hip.CS3_ERR_ARG and fragment in msg and msg.startswith("cs3_se_plan_create: "), (name, rc, msg)


def test_the_refusals_come_in_the_documented_order():
    """Two faults at once: the one that is documented first is the one reported."""
    faults = _faults()
    stage = {"null": 1, "n": 2, "Yp[0]": 2, "Yp decreases": 2, "null Yi": 2, "row range": 2, "order": 2, "twice": 2, "nref": 3, "ref range": 3,
             "ref repeats": 3, "ne": 4, "end range": 4, "from == to": 4, "m": 5, "kind": 6, "where bus": 7, "where end": 7, "diagonal": 8}
    level = lambda name: stage[name.split(" ")[0] if name.startswith("null ") and name != "null Yi" else name]
    legal = {("null ref", "nref"), ("null ends", "ne"), ("null rows", "m")}      # a null array of no entries is no fault
    tried = 0
    for i, (na, aa, fa) in enumerate(faults):
        for nb, ab, fb in faults[i + 1:]:
            if level(na) == level(nb) or set(aa) & set(ab) or (na, nb) in legal:
                continue
            rc, msg = _create(**dict(aa, **ab))
            assert rc == hip.CS3_ERR_ARG and fa in msg, (na, nb, msg)
            tried += 1
    assert tried > 100


def test_an_h_of_2_to_the_29_entries_is_refused():
    """Check 9, the last: a star whose hub has 2^14 - 1 leaves, and 2^14 + 1 P injections on the hub: every row holds
    2^15 - 1 entries, 2^29 + 2^14 - 1 in all.  Only the count is made; nothing of that size is built."""
    leaves = (1 << 14) - 1
    n = leaves + 1
    rows = np.concatenate([np.arange(n), np.arange(1, n), np.zeros(leaves, dtype=np.int64)])       # diagonal, column 0, row 0
    cols = np.concatenate([np.arange(n), np.zeros(leaves, dtype=np.int64), np.arange(1, n)])
    order = np.lexsort((rows, cols))
    Yp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))])
    m = (1 << 14) + 1
    args = dict(n=n, Yp=Yp, Yi=rows[order], ref=[1], ne=0, end_from=None, end_to=None, kind=np.ones(m), where=np.zeros(m))
    rc, msg = _create(m=m, **args)
    assert rc == hip.CS3_ERR_ARG and "H has 2^29 - 256 entries or more" in msg, msg
    assert _create(m=16, **dict(args, kind=np.ones(16), where=np.zeros(16))) == (0, "")


# ---- the cases: what the GPU tests take for granted

@pytest.mark.parametrize("key", sc.SOLVED)
def test_the_solved_cases_are_well_posed(key):
    case, P, ref = sc.case_of(key), sc.plan_of(key), sc.reference(key)
    assert ref["spd"] and ref["flag"] == 0 and 2 <= ref["iters"] < sc.MAX_ITERS
    Hr, _ = R.jacobian_ref(P, case["Yz"], case["Ye"], ref["vm"], ref["va"])
    _, G = R.gain_ref(P, Hr, case["w"])
    assert np.linalg.eigvalsh(G).min() > 0
    cond = np.abs(G).sum(axis=0).max() * np.abs(np.linalg.inv(G)).sum(axis=0).max()
    assert cond <= quad_ref.COND_MAX, (key, cond)
    steps = ref["steps"]
    if key != "noisy":
        err = np.abs(R.state_of(P, ref["vm"], ref["va"]) - R.state_of(P, case["vm"], case["va"])).max()
        assert err <= sc.TOL / 100, (key, err)                       # the rounding floor is far below the tolerance
        # quadratic convergence: no step within a factor 3 of the tolerance, so no rounding moves the iteration count
        assert not any(sc.TOL / 3 <= s <= 3 * sc.TOL for s in steps), (key, steps)
    else:
        assert steps[-1] / steps[-2] <= 0.1
        assert steps[-1] <= sc.TOL / 100 and steps[-2] >= 100 * sc.TOL, steps


def test_the_unobservable_case_is_singular_to_rounding():
    case, P = sc.case_of("unobservable"), sc.plan_of("unobservable")
    Hr, _ = R.jacobian_ref(P, case["Yz"], case["Ye"], case["vm0"], case["va0"])
    _, G = R.gain_ref(P, Hr, case["w"])
    assert np.linalg.eigvalsh(G).min() <= P["ns"] * R.EPS * np.abs(G).sum(axis=0).max()
    ref = sc.reference("unobservable")
    assert not ref["spd"] and ref["iters"] == 0
    assert np.array_equal(ref["vm"], case["vm0"]) and np.array_equal(ref["va"], case["va0"])


def test_the_planted_bad_row_is_an_injection_and_stands_out():
    case, bad = sc.bad_data_case()
    assert case["kind"][bad] in (1, 2)
    P = sc.plan_of("noisy")
    ref = R.gauss_newton_ref(P, case["Yz"], case["Ye"], case["z"], case["w"], case["vm0"], case["va0"], sc.TOL, sc.MAX_ITERS)
    assert ref["flag"] == 0
    Hr, _ = R.jacobian_ref(P, case["Yz"], case["Ye"], ref["vm"], ref["va"])
    bd = R.baddata_ref(P, Hr, case["w"], ref["r"])
    assert bd["cond"] <= quad_ref.COND_MAX
    rn = np.where(1.0 - case["w"] * bd["t"] <= sc.CRIT_TOL, 0.0, bd["rn"])
    order = np.argsort(-rn)
    # the GPU test holds the device's rn to 1e-6 of these: a gap of a tenth cannot close
    assert order[0] == bad and rn[order[0]] >= 1.1 * rn[order[1]] and rn[bad] > 5.0, (bad, order[:3], rn[order[:3]])


def test_restated_sums():
    """The trees of se_ref against plain sums, and against the restatement that quad_ref holds to its kernel."""
    rng = np.random.default_rng(3)
    for m in (1, 255, 256, 257, 70000):
        w, r = rng.uniform(1, 2, m), rng.standard_normal(m)
        J = R.cost_ref(w, r)
        assert abs(J - np.sum(w * r * r)) <= 1e-12 * J
        assert J == quad_ref._group_sums(w * (r * r), 256)
    P = sc.plan_of("star_row129")
    Hc, wr = rng.standard_normal(P["nnz_h"]), rng.standard_normal(P["m"])
    g = R.gradient_ref(P, Hc, wr, sc.limits()["wave_col"])
    want = R.dense_h(P, Hc[P["cpos"]]).T @ wr
    assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
