"""Device-memory lifetime: every HBM block of the host layer is held through one owner (csrc/cs3_hipmem.hpp) that counts
the blocks alive, process-wide (cs3_debug_live_device_buffers).  tests/lifetime_worker.py reaches every allocation site
once -- handles with a bottom forest and with the interleaved pool, every lazily built feature, regrowing buffers, plans
and handles closed in both orders, the stand-alone functions and their error returns behind an allocation -- in a process
of its own (handles of other tests that the garbage collector has not closed yet would count too) and asserts the count
is 0 before the first call, above 0 while a factorised handle is open, and 0 again at the end."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_every_device_block_is_freed(gpu):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lifetime_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    assert p.stdout.rstrip().endswith("lifetime ok") and "start" in p.stdout
