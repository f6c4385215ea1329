"""bench.py's contract: a plain run times exactly --steps steps and prints the headline alone; --dump-outputs writes
what the last timed step computed (float64, within 64 MB, a fixed sample beyond that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float64_arrays(tmp_path):
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    bench.dump_outputs(str(tmp_path), {"x": x})
    got = np.load(tmp_path / "x.npy")
    assert got.dtype == np.float64 and got.shape == (4, 3)
    assert np.array_equal(got, x)


def test_dump_outputs_samples_beyond_the_budget_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 128 + 8 * 100 + 128 + 8 * 50)
    a, b = np.arange(100.0), np.arange(1000.0) * 0.5
    bench.dump_outputs(str(tmp_path / "one"), {"a": a, "b": b})
    bench.dump_outputs(str(tmp_path / "two"), {"a": a, "b": b})
    assert np.array_equal(np.load(tmp_path / "one" / "a.npy"), a)          # fits: kept whole
    s1, s2 = np.load(tmp_path / "one" / "b.npy"), np.load(tmp_path / "two" / "b.npy")
    assert s1.size == 50 and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, b))              # sorted positions of b's own entries
    total = sum(os.path.getsize(p) for p in (tmp_path / "one").iterdir())
    assert total <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_solution(gpu, tmp_path):
    """A plain run in a process of its own: headline keys only, `steps` as asked, and the dumped x solves A x = b
    (the residual check that --full makes inside the benchmark)."""
    from csparse3_amd import synth
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-1500:])
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res
    assert res["steps"] == 5 and res["ms_per_step"] > 0 and res["dtype"] == "f64"
    assert not {"roofline", "phases", "configs", "cpu_baseline"} & set(res)
    assert sorted(os.listdir(out)) == ["x.npy"]
    x = np.load(out / "x.npy")
    m, n, Ap, Ai, Ax = synth.grid_jacobian(n=50000, seed=50000)
    b = synth.grid_rhs(n, 1, seed=1024)
    assert x.dtype == np.float64 and x.shape == (n,)
    r = bench.csc_matvec_np(n, Ap, Ai, Ax, x) - b
    assert np.abs(r).max() / np.abs(b).max() < 1e-9
