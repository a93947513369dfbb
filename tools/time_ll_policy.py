"""MEASUREMENT (MI355X): one low-level step of ``PreTrainedPolicyAction`` at 4096 envs -- the fused launch (``imx_pretrained_policy``, 16-
and 32-row tiles) next to the chain of existing launches it replaces (masked zero, ``imx_observations`` = k_frame + k_obs,
``imx_mlp_infer``, ``imx_action_process``) and the chain's kernels alone.

    python tools/time_ll_policy.py [--num-envs 4096] [--launches 200] [--repeats 7] [--runs 5] [--out profiles/ll_policy.json]

Each figure is the median over ``--repeats`` of (event time of one replay of a graph holding ``--launches`` low-level steps) / launches,
after warm-up replays: the GPU's own back-to-back time, as the captured rollout pays it.  ``--runs`` alternates the variants that many
times in one session; per variant the JSON holds every run's figure, their median and their minimum.  The noise is drawn in the kernels
(the product path); the chain's two tiny torch ops that set its noise key are part of the chain as the env runs it and are timed with it,
``chain_kernels_only`` leaves them and the masked zero out.  The verdict the default rests on: the fused step's median against the
chain's minimum.  Prints one JSON line and writes it to ``--out``.
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
from isaaclab_amd.robots import ROBOTS  # noqa: E402
from isaaclab_amd.state_feed import StateFeed  # noqa: E402

TASK = os.path.join(ROOT, "tests", "golden", "Isaac-Navigation-Flat-Anymal-C-v0.json")


def timed_graph(fn, launches: int, repeats: int) -> float:
    """``launches`` calls of ``fn`` captured once into a graph; us per call of one replay, median over ``repeats``."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1.0e3 / launches)
    return statistics.median(out)


def make_env(n: int, **kw):
    fx = load_task_cfg(TASK)
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(ROBOTS[fx["robot"]], n, "cuda:0", seed=11, num_snapshots=2), seed=11, noise_seed=11, **kw)
    env.reset()
    env.step(torch.randn(n, 3, device="cuda:0"))
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ll_policy.json"))
    a = ap.parse_args()
    n = a.num_envs
    envs = {"fused_16": make_env(n, low_level_tile_rows=16), "fused_32": make_env(n, low_level_tile_rows=32), "chain": make_env(n, fused_low_level=False)}
    chain = envs["chain"]
    L, stream = chain._lib, lambda: _lib.current_stream(chain.device)  # (per call: a capture runs on a stream of its own)
    st, bufs, N = chain._ll_state(), chain._ll_bufs, chain.num_envs
    seed = (chain.noise_seed ^ chain.LL_SEED_SALT) & 0xFFFFFFFFFFFFFFFF

    def obs():
        _lib.check(L.imx_observations(chain._ll_plan_h, N, ctypes.byref(st), ctypes.byref(bufs), None, None, seed, 1, None, stream()))

    def mlp():
        chain._ll_policy.infer(chain._ll_obs, chain._ll_out)

    def act():
        _lib.check(L.imx_action_process(chain._ll_plan_h, N, chain._ll_out.data_ptr(), math.inf, ctypes.byref(st), ctypes.byref(bufs), stream()))

    def kernels_only():
        obs(), mlp(), act()

    variants = {**{k: e._ll_launch for k, e in envs.items()}, "chain_kernels_only": kernels_only, "chain_observations": obs,
                "chain_mlp_infer": mlp, "chain_action_process": act}
    runs = {k: [] for k in variants}
    for _ in range(a.runs):  # alternated: every variant once per round
        for k, fn in variants.items():
            runs[k].append(round(timed_graph(fn, a.launches, a.repeats), 3))
    res = {"num_envs": n, "launches": a.launches, "repeats": a.repeats, "runs": a.runs, "unit": "us per low-level step, graph replay",
           "device": torch.cuda.get_device_name(0), "mlp_infer_tile_rows_of_the_chain": int(L.imx_pretrained_policy_tile_rows(n)),
           "policy_dims": chain._ll_policy.dims}
    for k, v in runs.items():
        res[k] = {"runs": v, "median": round(statistics.median(v), 3), "min": min(v)}
    best = min(("fused_16", "fused_32"), key=lambda k: res[k]["median"])
    res["fastest_fused"] = best
    res["fused_median_below_chain_min"] = bool(res[best]["median"] < res["chain"]["min"])
    for e in envs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
