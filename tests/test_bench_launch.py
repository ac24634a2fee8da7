"""bench.py --gpus N without a launcher starts N rank processes itself (the
driver's `python bench.py --gpus N` must yield N RCCL ranks): each child gets the
torchrun environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR), and the
parent has not initialised HIP when it starts them (CPU test, --launch-check
stops every rank before any GPU call).  Also the host side of --dump-outputs and
of --full (CPU tests of bench.dump_outputs and bench.want_cpu_baseline)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launch_sets_rank_env():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-check"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines[0] == {"parent_hip_initialized": False}
    ranks = sorted(lines[1:], key=lambda d: int(d["RANK"]))
    assert [(d["RANK"], d["LOCAL_RANK"], d["WORLD_SIZE"], d["MASTER_ADDR"]) for d in ranks] == \
        [(str(i), str(i), "3", "127.0.0.1") for i in range(3)]


def test_bench_rejects_gpus_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--launch-check"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_wait_ranks_fails_fast_and_stops_the_others():
    """A rank that exits non-zero ends the job: the ranks still running (here a
    sleeping child standing in for one blocked in a rendezvous) are terminated and
    the failing code is returned, instead of waiting for the backend timeout."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    hang = subprocess.Popen([sys.executable, "-c", "import time; time.sleep(600)"])
    fail = subprocess.Popen([sys.executable, "-c", "import sys; sys.exit(7)"])
    t0 = time.time()
    assert bench.wait_ranks([hang, fail], time.sleep) == 7
    assert time.time() - t0 < 60 and hang.poll() is not None
    ok = [subprocess.Popen([sys.executable, "-c", "pass"]) for _ in range(2)]
    assert bench.wait_ranks(ok, time.sleep) == 0


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: a small array is written whole as float32; one above the
    budget is cut along its longest axis to the same seeded, sorted indices on
    every call, and what is written stays within the budget."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "a"), {"latents": small})
    got = np.load(tmp_path / "a" / "latents.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    big = torch.arange(3 * 1001 * 2, dtype=torch.float32).reshape(3, 1001, 2)
    bench.dump_outputs(str(tmp_path / "b"), {"fields": big})
    bench.dump_outputs(str(tmp_path / "c"), {"fields": big})
    b, c = np.load(tmp_path / "b" / "fields.npy"), np.load(tmp_path / "c" / "fields.npy")
    assert np.array_equal(b, c) and b.dtype == np.float32 and b.nbytes <= 4000
    assert b.shape == (3, 4000 * 1001 // big.numel() // 4, 2)
    idx = (b[0, :, 0] // 2).astype(int)            # the rows of `big` that were kept
    assert np.all(np.diff(idx) > 0) and np.array_equal(b, big.numpy()[:, idx])


def test_plain_run_skips_the_cpu_baseline():
    """The CPU baseline runs with --full only (and --no-cpu-baseline still drops it)."""
    import argparse
    sys.path.insert(0, ROOT)
    import bench
    ns = argparse.Namespace
    assert not bench.want_cpu_baseline(ns(full=False, no_cpu_baseline=False), 1)
    assert bench.want_cpu_baseline(ns(full=True, no_cpu_baseline=False), 1)
    assert not bench.want_cpu_baseline(ns(full=True, no_cpu_baseline=True), 1)
    assert not bench.want_cpu_baseline(ns(full=True, no_cpu_baseline=False), 2)
