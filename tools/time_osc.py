"""MEASUREMENT (MI355X): ``imx_osc`` under HIP events at 4096 envs, modes 1, 2 and 3, next to ``imx_diff_ik`` (the IK-Abs Reach
fixture) and ``imx_action_process`` (the OSC fixture's 13-column action record).

    python tools/time_osc.py [--num-envs 4096] [--launches 200] [--repeats 7] [--lib another/libimx.so]

Each figure is the median over ``--repeats`` of (event time of ``--launches`` back-to-back launches) / launches, after a warm-up batch:
the launch-to-launch period of a small kernel on one stream as the eager env pays it (host call included); the ``_graph`` figures replay
the same launches from one captured graph, as the captured rollout does.  Prints one JSON line.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaaclab_amd import _lib  # noqa: E402
from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg  # noqa: E402
from isaaclab_amd.robots import FRANKA_PANDA  # noqa: E402
from isaaclab_amd.state_feed import StateFeed  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed(fn, launches: int, repeats: int) -> float:
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1.0e3 / launches)
    return statistics.median(out)


def timed_graph(fn, launches: int, repeats: int) -> float:
    """The same launches captured once into a graph and replayed: the GPU's own back-to-back time, without the host's call overhead."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return timed(g.replay, 3, repeats) / launches


def make_env(task: str, n: int):
    fx = load_task_cfg(os.path.join(GOLDEN, task + ".json"))
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(FRANKA_PANDA, n, "cuda:0", seed=11, num_snapshots=2), seed=11)
    env.reset()
    env.step(torch.randn(n, env.plan.action_dim, device="cuda:0"))
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lib", help="time this build of the library instead of the tree's (for one build against another)")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "num_envs": a.num_envs, "unit": "us per launch", "device": torch.cuda.get_device_name(0)}
    env = make_env("Isaac-Reach-Franka-OSC-v0", a.num_envs)
    for mode in (1, 2, 3):
        res[f"k_osc_mode{mode}"] = round(timed(lambda: env._osc_launch(mode), a.launches, a.repeats), 3)
        res[f"k_osc_mode{mode}_graph"] = round(timed_graph(lambda: env._osc_launch(mode), a.launches, a.repeats), 3)
    act = torch.randn(a.num_envs, env.plan.action_dim, device="cuda:0")
    L, stream = env._lib, _lib.current_stream(env.device)
    st, bufs = env._state(), env._bufs
    res["k_action_13_columns"] = round(timed(lambda: _lib.check(L.imx_action_process(env._plan_h, env.num_envs, act.data_ptr(), math.inf, ctypes.byref(st),
                                                                                       ctypes.byref(bufs), stream)), a.launches, a.repeats), 3)
    env.close()
    env = make_env("Isaac-Reach-Franka-IK-Abs-v0", a.num_envs)
    for mode in (1, 2, 3):
        res[f"k_diff_ik_mode{mode}"] = round(timed(lambda: env._diff_ik(mode), a.launches, a.repeats), 3)
        res[f"k_diff_ik_mode{mode}_graph"] = round(timed_graph(lambda: env._diff_ik(mode), a.launches, a.repeats), 3)
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
