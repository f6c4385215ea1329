"""The launch schedule (csrc/schedule.cpp) as cs3_debug_launch_plan prints it, without a GPU.

1. Every plan of tests/launch_plan_cases.py equals, row for row, the sequence of launches, event records and stream waits
   that the schedulers issued when the schedule was still control flow in kernels.hip (tests/golden/launch_plans.json,
   recorded as tests/golden/make_launch_plans.py says).
2. What the schedule's comments claim holds on the same plans: every group is issued once; under happens-before (the order
   on one stream plus the record -> wait edges) a forward sweep follows the factorisation of its level and the levels
   below -- but for the dense root's chain, where it follows the levels below and chunk c block launch (c + 1) * cwb;
   every stream that got a step is joined into the caller's stream before the plan ends."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import launch_plan_cases as lp
from launch_plan_cases import KIND, SLOT, FIRST, COUNT, CLS, LEVEL, MAX_W, ARG, EVENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [lp.case_id(c) for c in lp.CASES]
_PLANS = {}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
        return json.load(f)


def _plan(hip, c):
    """-> (rows, supernodes of the handle); built once per case.  A case with switches runs in a child process: the
    library reads them once."""
    key = lp.case_id(c)
    if key not in _PLANS:
        name, sym, batch, op, nrhs, trans, env, _ = c
        with lp.handle(hip, name, batch, sym) as F:
            nsuper = int(F.info.nsuper)
            if env:
                e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_plan_worker.py"), str(lp.CASES.index(c))],
                                   env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
                assert p.returncode == 0, p.stderr[-2000:]
                rows = np.array(json.loads(p.stdout.strip().splitlines()[-1])[0], dtype=np.int32).reshape(-1, 10)
            else:
                rows = lp.plan(hip, F, op, nrhs, trans)
        rows.setflags(write=False)
        _PLANS[key] = (rows, nsuper)
    return _PLANS[key]


def test_the_cases_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(IDS) and len(set(IDS)) == len(IDS)
    for c in lp.CASES:
        assert golden[lp.case_id(c)]["branch"] == c[7], lp.case_id(c)
    # what the list is there for: every strategy of the fused step, every count of released chunks, both level schedules
    branches = {c[7] for c in lp.CASES if c[3] == "fused"}
    assert {"no overlap", "levels on aux", "fork"} <= branches
    assert {"root chain, %d released" % k for k in (0, 1, 2, 5, 6)} <= branches


@pytest.mark.parametrize("c", lp.CASES, ids=IDS)
def test_plan_equals_the_recorded_calls(hip, golden, c):
    rows, _ = _plan(hip, c)
    want = np.array(golden[lp.case_id(c)]["rows"], dtype=np.int32).reshape(-1, 10)
    assert lp.branch_of(rows, c[3]) == c[7]
    assert rows.shape == want.shape, (rows.tolist(), want.tolist())
    bad = np.flatnonzero((rows != want).any(axis=1))
    assert len(bad) == 0, (int(bad[0]), rows[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------ invariants --

def _chunk_width(batch, nrhs, max_w):
    """schedule.cpp, big_sweep_plan: columns per chunk launch."""
    return (256 if max_w > 128 else 128) if batch * nrhs < 8 else 64


def _groups(rows, kinds):
    """The launch groups behind the steps of `kinds`: {(first, count): their rows}, in schedule order."""
    out = {}
    for r in rows[np.isin(rows[:, KIND], kinds)]:
        out.setdefault((int(r[FIRST]), int(r[COUNT])), []).append(r)
    return dict(sorted(out.items()))


def _tiles(groups, lo, hi):
    at = lo
    for first, count in groups:
        assert first == at and count > 0, (first, count, at)
        at += count
    return at == hi


def _check_factor(rows, nsuper):
    G = _groups(rows, lp.FACTOR_STEPS)
    assert _tiles(G, 0, nsuper), list(G)
    for key, steps in G.items():
        kinds = [int(s[KIND]) for s in steps]
        if kinds == [lp.FRONT_GROUP]:
            assert steps[0][CLS] != lp.FC_SCHUR
        elif steps[0][CLS] == lp.FC_SCHUR:
            assert kinds == [lp.BIG_GATHER, lp.SCHUR_TAKE], (key, kinds)
        else:                  # a chain of big fronts: the gather, block steps 0 .. nblk (nblk: the closing launch), in order
            nblk = -(-int(steps[0][MAX_W]) // lp.BIG_NB)
            assert steps[0][CLS] == lp.FC_BIG and kinds == [lp.BIG_GATHER] + [lp.BIG_BLOCK] * (nblk + 1), (key, kinds)
            assert [int(s[ARG]) for s in steps[1:]] == list(range(nblk + 1))
        assert len({int(s[SLOT]) for s in steps}) == 1, "a group stays on one stream"


def _check_sweep(rows, kinds, nsuper, batch, nrhs, skip=None):
    group, pre, chunk = kinds
    G = _groups(rows, kinds)
    if skip is not None:       # the forest's forward sweep rode on its factor launch: its fronts come first in the schedule
        assert skip[0] == 0 and skip not in G
        assert _tiles(G, skip[1], nsuper), list(G)
    else:
        assert _tiles(G, 0, nsuper), list(G)
    for key, steps in G.items():
        ks = [int(s[KIND]) for s in steps]
        if ks == [group]:
            continue
        nchunk = -(-int(steps[0][MAX_W]) // _chunk_width(batch, nrhs, int(steps[0][MAX_W])))
        assert steps[0][CLS] == lp.SK_BIG and ks in ([pre] + [chunk] * nchunk, [chunk] * nchunk), (key, ks, nchunk)
        assert ks[0] == pre or kinds == lp.BWD_STEPS, "only the backward sweep of a lone dense root has no preparation launch"
        assert [int(s[ARG]) for s in steps if s[KIND] == chunk] == list(range(nchunk))
        assert len({int(s[SLOT]) for s in steps if s[KIND] != chunk}) <= 1


def _before(rows):
    """before[i] = bit mask of the steps that happen before step i: the earlier steps of its stream, and for a wait what
    happened before the latest record of its event (events count from 0 again in a second plan)."""
    before, last_on, recorded = [], {}, {}
    for i, r in enumerate(rows):
        m = 0
        for j in [last_on.get(int(r[SLOT]))] + ([recorded[int(r[EVENT])]] if r[KIND] == lp.WAIT else []):
            if j is not None:
                m |= before[j] | (1 << j)
        before.append(m)
        last_on[int(r[SLOT])] = i
        if r[KIND] == lp.RECORD:
            recorded[int(r[EVENT])] = i
    return before


@pytest.mark.parametrize("c", lp.CASES, ids=IDS)
def test_every_group_is_issued_once(hip, c):
    rows, nsuper = _plan(hip, c)
    name, sym, batch, op, nrhs, trans, env, _ = c
    if op in ("factor", "fused"):
        _check_factor(rows, nsuper)
    else:
        assert not np.isin(rows[:, KIND], lp.FACTOR_STEPS).any()
    if op in ("bwd", "schur_bwd", "fused"):
        _check_sweep(rows, lp.BWD_STEPS, nsuper, batch, nrhs)
    else:
        assert not np.isin(rows[:, KIND], lp.BWD_STEPS).any()
    if op in ("fwd", "schur_fwd", "fused"):
        # fwd_in_factor = the fused step with one right-hand side on a handle with a forest (SK_SUB in its backward sweep)
        sub = [(int(r[FIRST]), int(r[COUNT])) for r in rows if r[KIND] == lp.SWEEP_BWD and r[CLS] == lp.SK_SUB]
        fwd_in_factor = op == "fused" and nrhs == 1 and len(sub) == 1
        _check_sweep(rows, lp.FWD_STEPS, nsuper, batch, nrhs, skip=sub[0] if fwd_in_factor else None)
        if op == "fused" and name == lp.FOREST_CASE:
            assert fwd_in_factor == (nrhs == 1)
    else:
        assert not np.isin(rows[:, KIND], lp.FWD_STEPS).any()


@pytest.mark.parametrize("c", [c for c in lp.CASES if c[3] == "fused"], ids=[lp.case_id(c) for c in lp.CASES if c[3] == "fused"])
def test_forward_sweep_follows_the_factorisation_it_reads(hip, c):
    rows, _ = _plan(hip, c)
    batch, nrhs = c[2], c[4]
    before = _before(rows)
    factor = [i for i, r in enumerate(rows) if r[KIND] in lp.FACTOR_STEPS]
    chains = 0
    for i, r in enumerate(rows):
        if r[KIND] not in lp.FWD_STEPS:
            continue
        # (a forest handle swept on the level schedule numbers its levels differently, and waits for everything.  The
        #  root chain is the one exception the schedule makes: the sweep of the chain's own group does not wait for the
        #  end of the chain -- its preparation launch reads no factor, chunk c what block launch (c + 1) * cwb leaves)
        own_chain = c[7].startswith("root chain") and r[KIND] != lp.SWEEP_FWD and r[LEVEL] == rows[factor[-1]][LEVEL]
        need = [j for j in factor if rows[j][LEVEL] < r[LEVEL] or (rows[j][LEVEL] == r[LEVEL] and not own_chain) or c[7] == "no overlap"]
        missing = [j for j in need if not before[i] >> j & 1]
        assert not missing, (i, r.tolist(), rows[missing[0]].tolist())
        if r[KIND] == lp.FWD_CHUNK:
            blocks = {int(rows[j][ARG]): j for j in factor if rows[j][KIND] == lp.BIG_BLOCK and rows[j][FIRST] == r[FIRST]}
            if blocks:         # column block b is final after block launch b + 1: chunk c needs launch (c + 1) * cwb
                cwb = _chunk_width(batch, nrhs, int(r[MAX_W])) // lp.BIG_NB
                j = blocks[min((int(r[ARG]) + 1) * cwb, max(blocks))]
                assert before[i] >> j & 1, (i, r.tolist(), rows[j].tolist())
                chains += 1
    assert chains > 0 or not c[7].startswith("root chain")


@pytest.mark.parametrize("c", lp.CASES, ids=IDS)
def test_every_stream_is_joined_into_the_callers(hip, c):
    rows, _ = _plan(hip, c)
    before = _before(rows)
    main = [i for i, r in enumerate(rows) if r[SLOT] == 0]
    assert main, "nothing on the caller's stream"
    for slot in sorted(set(rows[:, SLOT].tolist()) - {0}):
        last = max(i for i, r in enumerate(rows) if r[SLOT] == slot)
        assert before[main[-1]] >> last & 1, (slot, rows[last].tolist())
    # an event is recorded before it is waited for, and numbered in the order of its first record
    seen = -1
    for r in rows:
        if r[KIND] == lp.RECORD and r[EVENT] > seen:
            assert r[EVENT] == seen + 1
            seen = int(r[EVENT])
        if r[KIND] == lp.WAIT:
            assert 0 <= r[EVENT] <= seen
