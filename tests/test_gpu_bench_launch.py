"""``python bench.py --gpus N`` the way the driver calls it (no launcher around it): the script starts its own N ranks
(the reference's Trainer spawns its own too, train_script.py:215-218).  On a 1-GPU box the ranks share cuda:0 over gloo
(--dist-backend gloo; the numbers of such a run mean nothing, the code path is what is checked)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout=900):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--dist-backend", "gloo"], env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly ONE JSON line expected (rank 0), got {len(lines)}: {r.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_gpus_2_self_launches_sampling():
    line = _bench("--gpus", "2", "--steps", "5", "--warmup", "2", "--puzzles", "2", "--replays", "2", "--no-cpu-baseline")
    assert line["n_gpus"] == 2 and line["distributed"]["world_size"] == 2 and line["distributed"]["backend"] == "gloo"
    assert len(line["distributed"]["per_rank_ms_per_step"]) == 2
    assert line["config"]["global_puzzles"] == 4 and line["steps"] == 5 and line["value"] > 0
    assert line["metric"].startswith("denoising steps/sec (900-piece dense graph, T=100)")
    # value = whole-job puzzles x steps / median pass time
    assert abs(line["value"] - 4 * 5 / (line["ms_per_step"] * 5e-3)) / line["value"] < 1e-6


@pytest.mark.gpu
def test_bench_gpus_2_self_launches_training():
    line = _bench("--gpus", "2", "--config", "5", "--steps", "3", "--warmup", "1", "--train-puzzles", "4")
    assert line["n_gpus"] == 2 and line["distributed"]["world_size"] == 2
    assert line["config"]["global_puzzles"] == 8 and line["value"] > 0


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_final_poses(tmp_path):
    """Without --full a run times exactly its K steps once and measures nothing else; --dump-outputs writes the poses of the
    timed loop's last step."""
    import numpy as np
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--puzzles", "2", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 3 and line["replay"]["passes"] == 1 and line["replay"]["steps_per_pass"] == 3
    assert abs(line["value"] - 2 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-6
    assert line["roofline"] is None and line["parity_mode"] is None and line["cpu_baseline"] is None
    x = np.load(tmp_path / "x_final.npy")
    assert x.dtype == np.float32 and x.shape == (2 * 900, 4) and np.isfinite(x).all()


def test_dump_outputs_writes_float_arrays_and_a_fixed_row_sample_over_the_cap(tmp_path, monkeypatch):
    import numpy as np
    import torch
    import bench
    bench.dump_outputs(str(tmp_path / "a"), {"x": torch.arange(12.).reshape(6, 2).half(), "y": torch.ones(3)})
    x, y = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert x.dtype == np.float32 and x.shape == (6, 2) and (x.ravel() == np.arange(12)).all() and (y == 1).all()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256)
    big = torch.arange(400.).reshape(200, 2)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"x": big})
    b, c = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert 0 < b.nbytes <= 256 and b.shape[1] == 2 and np.array_equal(b, c)           # same rows in every run
    assert (np.diff(b[:, 0]) > 0).all() and (b[:, 1] == b[:, 0] + 1).all()              # whole rows, in order


def test_bench_rejects_arguments_it_cannot_honour():
    for argv, msg in ((["--steps", "0"], "--steps must be at least 1"), (["--config", "5", "--dump-outputs", "d"], "--dump-outputs")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-2000:]


def test_bench_gpus_n_without_enough_gpus_says_so():
    """No GPU (this container) or fewer than N: a clear message, not an assertion about WORLD_SIZE."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("enough GPUs here")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], env=env,
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0
    assert "GPU(s) visible" in r.stderr and "AssertionError" not in r.stderr
