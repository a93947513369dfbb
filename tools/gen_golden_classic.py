"""TEST INFRASTRUCTURE (build container only): the Isaac-Ant-v0 and Isaac-Humanoid-v0 fixtures, from the REAL reference.

    python tools/gen_golden_classic.py

Writes, for each task,
  * ``isaaclab_amd/configs/<task>.json`` (``AntEnvCfg()`` / ``HumanoidEnvCfg()`` and their RSL-RL runner cfgs through
    ``oracle.gen_golden.dump_cfg``) and its ``.managers.json`` side file (reset events, robot init state);
  * ``tests/golden/<task>.npz``: ``oracle.gen_golden.run_task`` -- the real action, termination, reward and observation managers with
    the classic/humanoid/mdp terms, the class terms included -- on a feed tweaked so that every branch of those terms is taken, plus
    ``progress_reward.potentials`` after every reset and every compute (``reset/potentials``, ``step<k>/potentials_pre_reset``,
    ``step<k>/potentials``).

Three gaps of the fake scene of ``oracle/gen_golden.py`` are filled here, without editing it: ``ArticulationData.FORWARD_VEC_B``,
``root_physx_view.get_link_incoming_joint_force()`` (the feed's ``link_incoming_joint_force``), and the ``RewardManager.reset`` that the
real ``_reset_idx(all)`` of ``reset()`` runs (run_task only resets the action manager there; without it the potentials start at 0).
Deterministic: a second run reproduces the files bit for bit.
"""

from __future__ import annotations

import functools
import importlib
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)

from isaaclab_amd.robots import ANT, HUMANOID  # noqa: E402
from isaaclab_amd.state_feed import StateFeed, _quat_from_euler  # noqa: E402

_CLASSIC = "isaaclab_tasks.manager_based.classic"
TASKS = {  # task -> (env cfg module:class, agent cfg module:class, robot, minimum_height of the torso_height termination)
    "Isaac-Ant-v0": ("ant.ant_env_cfg:AntEnvCfg", "ant.agents.rsl_rl_ppo_cfg:AntPPORunnerCfg", ANT, 0.31),
    "Isaac-Humanoid-v0": ("humanoid.humanoid_env_cfg:HumanoidEnvCfg", "humanoid.agents.rsl_rl_ppo_cfg:HumanoidPPORunnerCfg", HUMANOID, 0.8),
}


def _load(spec: str):
    mod, _, cls = spec.partition(":")
    return getattr(importlib.import_module(f"{_CLASSIC}.{mod}"), cls)


# ---- the fake scene's missing pieces (class attributes: the managers' constructors already call the observation terms)
gg.FakeArticulationData.FORWARD_VEC_B = property(lambda self: torch.tensor([1.0, 0.0, 0.0]).repeat(self._feed.num_envs, 1))
gg.FakeArticulation.root_physx_view = property(
    lambda self: types.SimpleNamespace(get_link_incoming_joint_force=lambda: self.data._feed["link_incoming_joint_force"]))


def classic_feed_tweak(min_height: float):
    """Push the synthetic feed across every branch of the classic terms (applied to every snapshot): every 5th env tilted by up to
    0.8 rad (up_proj on both sides of 0.93); yaw and roll within 1e-4 of +-pi on a few envs (angles and angle-to-target at the wrap);
    torso heights 0.05 m below ``min_height`` on envs 1 mod 4 when (env + snapshot) is a multiple of 3 (env 1 resets at steps 1 and 4).
    Heading (uniform yaw: heading_proj on both sides of 0.8) and joints beyond the 0.98 / 0.99 limit ratios (soft limits default +- 0.45,
    positions default + U(-0.5, 0.5)) need no push; time-outs come from run_task's episode lengths."""

    def tweak(feed: StateFeed):
        g = torch.Generator().manual_seed(4242)
        N = feed.num_envs
        idx = torch.arange(N)
        st = feed._stack
        for k in range(feed.num_snapshots):
            roll = torch.randn(N, generator=g) * 0.15
            pitch = torch.randn(N, generator=g) * 0.15
            yaw = (torch.rand(N, generator=g) * 2.0 - 1.0) * math.pi
            tilt = idx % 5 == 0
            roll[tilt] = (torch.rand(int(tilt.sum()), generator=g) * 2.0 - 1.0) * 0.8
            pitch[tilt] = (torch.rand(int(tilt.sum()), generator=g) * 2.0 - 1.0) * 0.8
            yaw[idx % 16 == 3] = math.pi - 1.0e-4
            yaw[idx % 16 == 7] = -math.pi + 1.0e-4
            roll[idx % 16 == 11] = math.pi - 1.0e-4
            roll[idx % 16 == 15] = -math.pi + 1.0e-4
            st["root_quat_w"][k] = _quat_from_euler(roll, pitch, yaw)
            low = (idx % 4 == 1) & ((idx + k) % 3 == 0)
            st["root_pos_w"][k][low, 2] = min_height - 0.05
    return tweak


def dump_managers(task: str, env_cfg):
    """Side file as for the velocity tasks: reset events and the robot init state (UNMODIFIED cfg)."""
    base = env_cfg.to_dict()
    ev = {k: v for k, v in base["events"].items() if v is not None and v.get("mode") in ("reset", "interval")}
    side = {"events": ev, "curriculum": base.get("curriculum"),
            "scene": {"robot": {"init_state": {k: list(v) for k, v in base["scene"]["robot"]["init_state"].items()
                                               if k in ("pos", "rot", "lin_vel", "ang_vel")}}}}
    with open(os.path.join(gg.CONFIGS, task + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, indent=1, sort_keys=False)


def run(task: str):
    env_spec, agent_spec, robot, min_height = TASKS[task]
    progress_cls = importlib.import_module(f"{_CLASSIC}.humanoid.mdp.rewards").progress_reward
    events: list[tuple[str, torch.Tensor]] = []
    real_call, real_reset, real_build = progress_cls.__call__, progress_cls.reset, gg.build_ref_env

    @functools.wraps(real_call)  # (the manager inspects the signature of __call__)
    def call(self, *a, **k):
        out = real_call(self, *a, **k)
        events.append(("call", self.potentials.clone()))
        return out

    @functools.wraps(real_reset)
    def reset(self, env_ids):
        real_reset(self, env_ids)
        events.append(("reset", self.potentials.clone()))

    def build(*a, **k):  # ManagerBasedEnv.reset -> _reset_idx(all) also runs RewardManager.reset (after the action manager's reset)
        env = real_build(*a, **k)
        am_reset = env.action_manager.reset
        first = [True]

        def action_reset(env_ids=None):
            out = am_reset(env_ids)
            if first[0]:
                first[0] = False
                env.reward_manager.reset(env_ids)
            return out

        env.action_manager.reset = action_reset
        return env

    progress_cls.__call__, progress_cls.reset, gg.build_ref_env = call, reset, build
    try:
        steps = 5
        gg.run_task(task, _load(env_spec)(), _load(agent_spec)(), robot, N=64, steps=steps, seed=313,
                    kitchen=dict(feed_tweak=classic_feed_tweak(min_height)))
    finally:
        progress_cls.__call__, progress_cls.reset, gg.build_ref_env = real_call, real_reset, real_build
    dump_managers(task, _load(env_spec)())

    # potentials after the initial reset, after each compute and after each step's reset
    path = os.path.join(gg.GOLDEN, task + ".npz")
    z = np.load(path)
    # the per-step tensors no classic term reads are left out (run_task records every EXTRA tensor of a kitchen run)
    unread = ("body_lin_acc_w", "body_pos_w", "command_time_left", "command_counter", "body_quat_w", "object_root_pos_w")
    rec = {k: z[k] for k in z.files if k.rpartition("/")[2] not in unread or "/in/" not in k}
    assert events[0][0] == "reset", events[0][0]
    rec["reset/potentials"] = events[0][1].numpy()
    i = 1
    n_twice = 0
    for t in range(steps):
        assert events[i][0] == "call"
        rec[f"step{t}/potentials_pre_reset"] = events[i][1].numpy()
        i += 1
        if i < len(events) and events[i][0] == "reset":
            i += 1
        rec[f"step{t}/potentials"] = events[i - 1][1].numpy()
        assert len(rec[f"step{t}/reset_env_ids"]) == 0 or events[i - 1][0] == "reset"
    assert i == len(events)
    resets = [set(rec[f"step{t}/reset_env_ids"].tolist()) for t in range(steps)]
    n_twice = sum(1 for e in range(64) if sum(e in r for r in resets) >= 2)
    meta = json.loads(str(rec["meta_json"]))
    jp = torch.stack([torch.from_numpy(rec[f"step{t}/in/joint_pos"]) for t in range(steps)])
    lim = torch.from_numpy(rec["static/soft_joint_pos_limits"])
    s = (2.0 * (jp - 0.5 * (lim[..., 0] + lim[..., 1])) / (lim[..., 1] - lim[..., 0])).abs()
    meta.update(envs_reset_twice=n_twice, joints_beyond_0_98=int((s > 0.98).sum()), resets_per_step=[len(r) for r in resets])
    assert n_twice >= 1 and meta["joints_beyond_0_98"] > 0
    rec["meta_json"] = np.array(json.dumps(meta))
    np.savez_compressed(path, **rec)
    print(f"[golden] {task}: resets per step {meta['resets_per_step']}, {n_twice} envs reset twice, "
          f"{meta['joints_beyond_0_98']} joint samples beyond 0.98")


def main():
    for task in TASKS:
        run(task)


if __name__ == "__main__":
    main()
