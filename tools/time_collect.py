"""Rollout time alone: ``runner.collect()`` + ``compute_returns`` between HIP events, for configs ``bench.py`` does not run as they
stand -- an env with a "critic" observation group (bench.py hands the policy rows to ``compute_returns``).

    python tools/time_collect.py --task Isaac-Velocity-Rough-Anymal-C-v0-kitchen [--num-envs 4096] [--steps 20] [--warmup 5] [--split]
    python tools/time_collect.py --task tests/golden/Isaac-Repose-Cube-Allegro-v0.json [--python-normalization]

Prints one JSON line: mean / min / max milliseconds per rollout (T env steps + GAE), the launch path that ran and the device.  ``--split``
sets ``runner.fuse_launches = False``, ``--python-normalization`` ``runner.fuse_normalization = False``.  ``--task`` is a task id or the
path of a fixture file.  The env is built the way bench.py builds it (same terrain, feed and seeds)."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Isaac-Velocity-Rough-Anymal-C-v0-kitchen")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snapshots", type=int, default=4)
    ap.add_argument("--terrain-tiles", type=int, nargs=2, default=(10, 20))
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--split", action="store_true", help="fuse_launches = False")
    ap.add_argument("--python-normalization", action="store_true", help="fuse_normalization = False: an agent with empirical_normalization "
                    "rolls out step by step in Python")
    args = ap.parse_args()

    import torch

    from bench import build_env
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    device = torch.device("cuda", 0)
    torch.manual_seed(42)
    fx, env, _ = build_env(args.task, args.num_envs, device, 42, args.snapshots, tuple(args.terrain_tiles))
    agent = fx["agent"]
    venv = RslRlVecEnvWrapper(env, clip_actions=agent.get("clip_actions"))
    runner = OnPolicyRunner(venv, agent, log_dir=None, device=str(device), use_graph=not args.no_graph)
    if args.split:
        runner.fuse_launches = False
    if args.python_normalization:
        runner.fuse_normalization = False
    venv.episode_length_buf = torch.randint_like(venv.episode_length_buf, high=int(venv.max_episode_length))
    runner.train_mode()

    def rollout():
        runner.collect()
        with torch.inference_mode():
            runner.alg.compute_returns(runner.last_critic_obs)
        runner.alg.storage.clear()

    for _ in range(2 + args.warmup):  # the first collect warms up and captures the graph
        rollout()
    torch.cuda.synchronize(device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record()
    for k in range(args.steps):
        rollout()
        ev[k + 1].record()
    torch.cuda.synchronize(device)
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.steps)]
    infer = getattr(runner, "_infer", None)
    print(json.dumps({"task": args.task, "num_envs": args.num_envs, "T": runner.num_steps_per_env, "rollout": "eager" if args.no_graph else "hipGraph",
                      "collect_plus_gae_ms": {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms)},
                      "privileged_obs_type": runner.privileged_obs_type, "fuse_launches": bool(runner.fuse_launches),
                      "empirical_normalization": runner.empirical_normalization,
                      "fused_normalized_rollout": bool(runner.fuse_normalization and not runner._fusable() and runner._fusable_normalized()),
                      "fused_inference": bool(getattr(infer, "ok", False)), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
