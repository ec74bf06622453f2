"""GPU: mcd_loglike_grad_batch on a multi-device context -- three shards on device 0 over the stand-in all-reduce library
(tests/fake_rccl), in a fresh child process (tests/grad_sharded_worker.py) under its own time limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "grad_sharded_worker.py")


def test_three_shards_equal_one_device():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], check=True, capture_output=True)
    res = subprocess.run(["timeout", "-k", "10", "120", sys.executable, WORKER], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "GRAD_SHARDED_OK" in res.stdout
