"""Multi-process distributed-path tests (gloo, world_size=2, CPU).

The driver runs bench.py via torch.distributed.run with one rank per GPU at
round end; this tier proves that exact launch path works with no GPU: two
ranks, two fake nodes, one controller on rank 0, TCP store, max-over-ranks
timing, pooled latency samples.
"""

import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _run_bench(nproc: int, extra=()):
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={nproc}",
        "--master-addr", "127.0.0.1", "--master-port", "29581",
        str(ROOT / "bench.py"),
        "--gpus", str(nproc), "--steps", "10", "--warmup", "2", "--fake",
        *extra,
    ]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=420,
                         env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected one JSON line, got: {lines}"
    return json.loads(lines[0])


def test_bench_two_ranks_gloo():
    res = _run_bench(2)
    assert res["metric"] == "pods_scheduled_per_s"
    assert res["n_gpus"] == 2
    assert res["steps"] == 10
    assert res["value"] > 0
    assert res["scaling"] == "weak"
    import re
    assert re.fullmatch(r"\d+-controller-shards\+2-node-agents",
                        res["config"]["parallelism"])
    assert res["config"]["backend"] == "fake"
    assert res["p50_alloc_latency_ms"] is not None
    # pooled latency samples from both ranks: 2 * 10 recorded steps
    assert res["config"]["global_batch"] == 20


def test_bench_single_rank_no_torchrun():
    """The driver's N=1 invocation: plain `python bench.py`."""
    out = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--steps", "10",
         "--warmup", "2", "--fake"],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 1 and res["value"] > 0


def test_bench_full_dumps_last_step_allocation(tmp_path):
    """--full is accepted, --steps sets the timed step count, ms_per_step
    is the time of one timed step, and --dump-outputs writes the partition
    the last timed step handed out — for the profile the seed dictates."""
    import random
    import re

    import numpy as np

    from instaslice_amd.partition.profiles import parse_profile_name

    import time

    steps, warmup, seed = 7, 3, 4321
    t0 = time.monotonic()
    out = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--gpus", "1",
         "--steps", str(steps), "--warmup", str(warmup), "--fake", "--full",
         "--seed", str(seed), "--dump-outputs", str(tmp_path / "out")],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.monotonic() - t0
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected one JSON line, got: {lines}"
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["config"]["global_batch"] == steps
    assert res["config"]["full"] is True
    # the cpulist a single-rank run confined itself to, or None
    pinned = res["config"]["cpu_affinity"]
    assert pinned is None or re.fullmatch(r"\d+(-\d+)?(,\d+(-\d+)?)*", pinned)
    # one latency sample was taken per timed step: --steps sets their number
    assert res["latency_samples"] == steps
    # value is pods/s over the timed window, ms_per_step its reciprocal
    assert abs(res["ms_per_step"] * res["value"] / 1000.0 - 1.0) < 0.01
    # a step lasts at least as long as its pod took to be scheduled (the
    # step also deletes and drains it), and the timed steps fit in the run
    assert res["ms_per_step"] * steps >= res["p50_alloc_latency_ms"] * (steps // 2 + 1)
    assert res["ms_per_step"] * steps / 1000.0 < wall

    assert [p.name for p in (tmp_path / "out").iterdir()] == ["allocation.npy"]
    arr = np.load(tmp_path / "out" / "allocation.npy")
    assert arr.dtype == np.float64 and arr.shape == (1, 10)
    # the seeded request sequence: one draw per warmup and timed step
    rng = random.Random(seed)
    mix = res["config"]["profile_mix"]
    last = [rng.choice(mix) for _ in range(warmup + steps)][-1]
    mode, xcds, gb = parse_profile_name(last)
    (ordinal, start, size, tgt_parts, _tgt_dom, parts, _dom, rxcds, rgb,
     dev) = arr[0]
    assert size == xcds and rxcds == xcds and rgb == gb
    assert tgt_parts == parts == mode.num_partitions
    assert 0 <= ordinal < parts and start == ordinal * xcds and dev >= 0
