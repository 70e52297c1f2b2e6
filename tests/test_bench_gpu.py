"""-m gpu: bench.py's two kinds of run on a small workload.  A plain run prints the contract fields and the workload's config and
nothing that takes a run or pass of its own; --full adds those legs, and its parity check finds the timed step's records equal to
the checker's."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "parity_check", "multi_gpu", "e2e", "pcie_inclusive", "cfg5", "engine", "kernels_ms_per_step")
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "20000", "--anchors", "1000"]


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    d = run_bench()
    assert all(k in d for k in CONTRACT) and d["value"] > 0 and (d["steps"], d["warmup"]) == (2, 1)
    assert d["config"]["pairs_per_gpu"] == 20000
    assert [k for k in FULL_ONLY if k in d] == []


@pytest.mark.gpu
def test_full_run_adds_the_side_legs():
    d = run_bench("--full", "--cpu-pairs", "0", "--check-pairs", "2000", "--no-e2e", "--no-pipeline", "--no-cfg5")
    assert all(k in d for k in CONTRACT + FULL_ONLY) and "error" not in d
    assert d["parity_check"]["pairs_checked"] == 2000 and d["parity_check"]["pairs_differing"] == 0
    assert d["engine"]["dp_problems"] > 0 and d["kernels_ms_per_step"]
    assert d["pcie_inclusive"]["reads_per_s"] > 0
