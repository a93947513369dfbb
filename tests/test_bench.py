"""bench.py's own contract: a plain run prints only the headline line, ``--full`` adds the secondary measurements, and
``--dump-outputs DIR`` writes what the last timed iteration computed (bounded in size, the same env sample for every array)."""

import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("env_step_path", "env_step_path_full", "roofline", "roofline_step", "roofline_large_n", "roofline_mfma", "roofline_producers",
             "cpu_baseline")


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _fake_runner(N, T, D, A, P):
    env_ids = torch.arange(N, dtype=torch.float32)
    per_env = lambda *tail: env_ids.view(1, N, *([1] * len(tail))).expand(T, N, *tail).contiguous()  # noqa: E731  (value = env id)
    st = SimpleNamespace(num_envs=N, observations=per_env(D), privileged_observations=None, actions=per_env(A), rewards=per_env(1),
                         dones=(per_env(1) % 2).to(torch.uint8), values=per_env(1), actions_log_prob=per_env(1), returns=per_env(1),
                         advantages=per_env(1), mu=per_env(A), sigma=per_env(A))
    alg = SimpleNamespace(storage=st, bucket=SimpleNamespace(flat=torch.arange(P + 8, dtype=torch.float32), numel=P),
                          loss_dict=lambda: {"value_function": 0.5, "surrogate": -0.25, "entropy": 17.0, "kl": 0.01}, learning_rate=1e-3 / 1.5)
    return SimpleNamespace(alg=alg, last_obs=env_ids.view(N, 1).expand(N, D).contiguous(), privileged_obs_type=None, last_critic_obs=None)


def test_dump_outputs_samples_the_same_envs_within_64_mb(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    N, T, D, A, P = 4096, 24, 235, 12, 1000
    runner = _fake_runner(N, T, D, A, P)
    info = bench.dump_outputs(runner, str(tmp_path / "a"))
    assert 0 < info["envs_sampled"] < N and info["num_envs"] == N
    files = sorted(os.listdir(tmp_path / "a"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    assert total <= bench.DUMP_BYTES_MAX
    arrays = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for n in ("storage_observations", "storage_actions", "storage_rewards", "storage_dones", "storage_returns", "storage_advantages", "last_obs",
              "policy_params", "loss_kl", "learning_rate"):
        assert n in arrays, n
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    ids = arrays["last_obs"][:, 0]
    assert len(ids) == info["envs_sampled"] and np.all(np.diff(ids) > 0)  # distinct envs, env order kept
    for n, a in arrays.items():
        if n.startswith("storage_") and n != "storage_dones":
            assert a.shape[:2] == (T, len(ids)) and np.array_equal(a[0, :, 0], ids), n
    assert np.array_equal(arrays["storage_dones"][0, :, 0], ids % 2)
    assert np.array_equal(arrays["policy_params"], np.arange(P, dtype=np.float32))
    assert arrays["learning_rate"].dtype == np.float64 and float(arrays["learning_rate"]) == 1e-3 / 1.5
    bench.dump_outputs(runner, str(tmp_path / "b"))  # a fixed sample: a second run writes the very same arrays
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), arrays[f[:-4]]), f


def test_dump_outputs_keeps_every_env_of_a_small_run(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    N, T = 256, 24
    info = bench.dump_outputs(_fake_runner(N, T, 48, 12, 100), str(tmp_path))
    assert info["envs_sampled"] == N
    assert np.array_equal(np.load(tmp_path / "storage_rewards.npy")[0, :, 0], np.arange(N, dtype=np.float32))


def _plain_bench_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--num-envs", "512",
                        "--terrain-tiles", "2", "3", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_line_and_dumps_outputs(tmp_path):
    """A plain run: exactly one JSON line with the headline fields, --steps timed steps, no secondary measurement; the dump holds the
    last step's rollout, returns and policy.  A second run with the same arguments starts from the same inputs and dumps the very
    same arrays."""
    out_dir = tmp_path / "dump"
    r = _plain_bench_run(out_dir)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "env-steps/s"
    assert not any(k in out for k in SECONDARY), sorted(out)
    rew = np.load(out_dir / "storage_rewards.npy")
    ret = np.load(out_dir / "storage_returns.npy")
    obs = np.load(out_dir / "storage_observations.npy")
    assert rew.shape == ret.shape == (24, 512, 1) and obs.shape[:2] == (24, 512) and np.isfinite(obs).all() and np.isfinite(ret).all()
    params = np.load(out_dir / "policy_params.npy")
    assert params.dtype == np.float32 and params.size > 0 and np.isfinite(params).all()
    assert out["dump_outputs"]["envs_sampled"] == 512
    _plain_bench_run(tmp_path / "again")
    files = sorted(os.listdir(out_dir))
    assert files == sorted(os.listdir(tmp_path / "again"))
    for f in files:
        assert np.array_equal(np.load(out_dir / f), np.load(tmp_path / "again" / f)), f
