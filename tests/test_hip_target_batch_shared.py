"""TargetBatch with small m on the device: the shared batch builds (a workgroup serves a run of consecutive chains and every
target they touch) give the chains of M separate samplers with chain_offset = t m, bit for bit -- states, kept rows, n_tries,
n_reject and error flags -- for Bingham (diagonal, dense, with b) and vMF mixtures of K = 1, 3, 10, 16 at d = 3, 5, 10, 11, 16
and m = 1, 3, 16, 64, 100, 300; launch splits match one launch; and the launch is gsss_batch_plan's.

Every GPU step is a process of its own (tests/batch_shared_worker.py) under its own timeout.  A step that ends by a signal or by
the timeout stops the module: the steps after it fail without touching the GPU, and nothing is run again."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "batch_shared_worker.py")
_stopped = []


def run_step(timeout, env=None, **args):
    if _stopped:
        pytest.fail(f"not run: an earlier GPU step ended abnormally ({_stopped[0]})")
    try:
        r = subprocess.run([sys.executable, WORKER, json.dumps(args)], capture_output=True, text=True, timeout=timeout,
                           env={**os.environ, **(env or {})})
    except subprocess.TimeoutExpired:
        _stopped.append(f"timeout after {timeout} s: {args}")
        pytest.fail(_stopped[0])
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append(f"exit status {r.returncode}: {args}")
    print(r.stdout[-4000:])
    assert r.returncode == 0, (args, r.stderr[-4000:])
    return r


FAMILIES = ["diag", "dense", "b", "vmf1", "vmf3", "vmf10", "vmf16"]
DIMS = [3, 5, 10, 11, 16]
GRID = [(f, d) for f in FAMILIES for d in DIMS if not (f == "vmf16" and d > 10)]   # (d = 11 .. 16: K <= 10 has a lane kernel)


@pytest.mark.parametrize("family,d", GRID)
def test_batch_is_the_loop(family, d):
    run_step(600, step="family", family=family, d=d, turn=GRID.index((family, d)))


@pytest.mark.parametrize("m", [16, 100])
def test_mixed_diagonal_and_dense_keeps_its_exception(m):
    """A batch that mixes diagonal and dense A runs the dense kernels: 1e-10 against its members alone, integer outputs exact."""
    run_step(300, step="mixed", m=m)


@pytest.mark.parametrize("family,d,m", [("dense", 5, 16), ("vmf3", 3, 100), ("diag", 11, 3)])
def test_launch_splits(family, d, m):
    run_step(600, step="splits", family=family, d=d, M=14, m=m)


@pytest.mark.parametrize("screen", [True, False])
@pytest.mark.parametrize("family,d,M,m", [("dense", 5, 100, 16), ("vmf3", 3, 9, 300), ("vmf10", 10, 50, 64), ("dense", 16, 300, 1),
                                          ("diag", 16, 300, 1), ("vmf3", 11, 40, 100)])
def test_launch_is_the_plan(family, d, M, m, screen):
    r = run_step(300, env={"GSSS_DEBUG_OCCUPANCY": "1"}, step="plan", family=family, d=d, M=M, m=m, screen=screen)
    plan = json.loads(re.search(r"^plan (\{.*\})$", r.stdout, re.M).group(1))
    said = re.findall(r"batch shared: grid (\d+), (\d+) chains and (\d+) targets a workgroup, (\d+) doubles a target, (\d+) B of LDS", r.stderr)
    assert said, r.stderr[-2000:]
    grid, chains, targets, stride, lds = map(int, said[-1])
    assert (grid, chains, targets) == (plan["grid"], plan["chains_per_workgroup"], plan["targets_per_workgroup"])
    assert stride % 2 == 1 and lds == 8 * (130 + targets * stride)    # the draw tables, then the targets at an odd stride
