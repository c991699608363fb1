"""bench.py --dump-outputs: the per-genome counts of the last timed step and of all timed steps, as float64 .npy.
The GPU runs use a small tree and few reads.  The two-rank run puts both ranks on device 0 with gloo (bench.py's
PFQ_BENCH_SAME_GPU rehearsal), so the reduction of the counts over the ranks is exercised on a one-GPU box.  A --full
run must compute what a plain run computes and add its extra rates and checks."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES, READS, STEPS, WARMUP = 64, 32768, 3, 1


def _bench(args, env=None, timeout=600):
    """bench.py in its own process group: a run that outlives `timeout` is ended with every rank it started."""
    p = subprocess.Popen([sys.executable, "-s", os.path.join(ROOT, "bench.py"), *args], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        raise
    return p.returncode, out, err


def test_steps_must_be_positive():
    rc, _, err = _bench(["--steps", "0"])
    assert rc == 2 and "--steps must be at least 1" in err


def _last_step_positives(world):
    """Per genome: the positive reads of the last timed step over all ranks (each must hit its source leaf)."""
    n_batches = min(STEPS + WARMUP, 16)
    b = (WARMUP + STEPS - 1) % n_batches
    expect = np.zeros(LEAVES, dtype=np.int64)
    for r in range(world):
        pos, leaf = bench.read_plan(np, bench.READ_SEED, (b * world + r) * READS, READS, LEAVES)
        expect += np.bincount(leaf[pos], minlength=LEAVES)
    return expect


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_dump_outputs(gpu, tmp_path, world):
    env = {k: v for k, v in os.environ.items() if k not in bench.EXPERIMENT_VARS}
    if world > 1:
        env["PFQ_BENCH_SAME_GPU"] = "1"
    rc, out, err = _bench(["--gpus", str(world), "--steps", str(STEPS), "--warmup", str(WARMUP), "--leaves", str(LEAVES),
                           "--reads-per-step", str(READS), "--cpu-seconds", "0", "--dump-outputs", str(tmp_path)], env)
    assert rc == 0, err[-3000:]
    res = json.loads(out.strip().splitlines()[-1])
    assert res["steps"] == STEPS and res["n_gpus"] == world and res["ms_per_step"] > 0
    last = np.load(tmp_path / "leaf_counts_last_step.npy")
    total = np.load(tmp_path / "leaf_counts.npy")
    for a in (last, total):
        assert a.dtype == np.float64 and a.shape == (LEAVES,)
    assert total.sum() == res["hits_total"]
    if world == 1:
        assert last.sum() == res["hits_last_step"]
    # the last step's counts are its positives plus at most a few Bloom false positives, over all ranks
    expect = _last_step_positives(world)
    assert (last >= expect).all()
    assert last.sum() - expect.sum() <= 64
    assert (total >= last).all() and total.sum() > last.sum()


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse_args().full is True


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_full_run_checks_and_matches_plain(gpu, tmp_path, world):
    """--full adds the extra rates, the CPU baseline and the checks; the timed steps compute the same as a plain run's."""
    env = {k: v for k, v in os.environ.items() if k not in bench.EXPERIMENT_VARS}
    if world > 1:
        env["PFQ_BENCH_SAME_GPU"] = "1"
    common = ["--gpus", str(world), "--steps", str(STEPS), "--warmup", str(WARMUP), "--leaves", str(LEAVES),
              "--reads-per-step", str(READS), "--cpu-seconds", "1"]
    lines = {}
    for mode in ("plain", "full"):
        rc, out, err = _bench(common + ["--dump-outputs", str(tmp_path / mode)] + (["--full"] if mode == "full" else []), env)
        assert rc == 0, err[-3000:]
        lines[mode] = json.loads(out.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    extras = ("parity", "cpu_baseline", "host_buffers_reads_per_s", "want_hits_reads_per_s")
    assert not any(k in plain for k in extras)
    assert full["parity"]["oracle_sample"] == "ok" and full["parity"]["timed_region_ground_truth"] == "ok"
    if world == 1:
        assert full["cpu_baseline"]["value"] > 0
        assert full["host_buffers_reads_per_s"] > 0 and full["want_hits_reads_per_s"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "hits_total"):
        assert plain[k] == full[k], k
    for name in ("leaf_counts_last_step", "leaf_counts"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy"))
