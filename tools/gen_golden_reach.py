"""TEST INFRASTRUCTURE (build container only): the Isaac-Reach-Franka-v0 and Isaac-Reach-UR10-v0 fixtures, from the REAL reference.

    python tools/gen_golden_reach.py

Writes, for each task,
  * ``isaaclab_amd/configs/<task>.json`` (``FrankaReachEnvCfg()`` / ``UR10ReachEnvCfg()`` and their RSL-RL runner cfgs through
    ``oracle.gen_golden.dump_cfg``) and its ``.managers.json`` side file (reset events, curriculum, robot init state);
  * ``tests/golden/<task>.npz``: ``oracle.gen_golden.run_task`` -- the real action, termination, reward and observation managers with
    the manipulation/reach/mdp reward terms -- on a feed tweaked so that every branch of those terms is taken, plus the plan blob the
    live cfg object compiles to (``live_cfg/blob``).

Two gaps of the fake scene of ``oracle/gen_golden.py`` are filled here, without editing it: ``ArticulationData.root_state_w`` and
``body_state_w`` (what the reach rewards read: the feed's root pose and ``body_pos_w`` / ``body_quat_w``, zero velocities).  The command
is the feed's (N, 7) pose command, served by the fake command manager.  Deterministic: a second run reproduces the files bit for bit.
"""

from __future__ import annotations

import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)

import isaaclab.utils.math as ref_math  # noqa: E402

from isaaclab_amd.plan import compile_plan  # noqa: E402
from isaaclab_amd.robots import FRANKA_PANDA, UR10  # noqa: E402
from isaaclab_amd.state_feed import StateFeed  # noqa: E402

_REACH = "isaaclab_tasks.manager_based.manipulation.reach.config"
TASKS = {  # task -> (env cfg module:class, agent cfg module:class, robot, end-effector body, the cfg's fixed command pitch)
    "Isaac-Reach-Franka-v0": ("franka.joint_pos_env_cfg:FrankaReachEnvCfg", "franka.agents.rsl_rl_ppo_cfg:FrankaReachPPORunnerCfg",
                              FRANKA_PANDA, "panda_hand", math.pi),
    "Isaac-Reach-UR10-v0": ("ur_10.joint_pos_env_cfg:UR10ReachEnvCfg", "ur_10.agents.rsl_rl_ppo_cfg:UR10ReachPPORunnerCfg",
                            UR10, "ee_link", math.pi / 2),
}


def _load(spec: str):
    mod, _, cls = spec.partition(":")
    return getattr(importlib.import_module(f"{_REACH}.{mod}"), cls)


# ---- the fake scene's missing pieces: the state tensors the reach rewards read (articulation_data.py:366-455)
def _root_state_w(self):
    f = self._feed
    return torch.cat([f["root_pos_w"], f["root_quat_w"], f["root_lin_vel_w"], f["root_ang_vel_w"]], dim=-1)


def _body_state_w(self):
    f = self._feed
    p, q = f["body_pos_w"], f["body_quat_w"]
    return torch.cat([p, q, torch.zeros(*p.shape[:2], 6)], dim=-1)


gg.FakeArticulationData.root_state_w = property(_root_state_w)
gg.FakeArticulationData.body_state_w = property(_body_state_w)


def reach_feed_tweak(robot, ee: str, pitch: float):
    """Push the synthetic feed across every branch of the reach terms (applied to every snapshot):
    * commands: every other env gets the cfg's own orientation draw, quat_from_euler_xyz(0, pitch, U(-3.14, 3.14)); with pitch = pi
      its w is cos(pi / 2) cos(yaw / 2) ~ -4.4e-8 cos(yaw / 2) in fp32: w ~ 0 of either sign;
    * end-effector position: the commanded world position plus a random direction times 0, std / 2, std, 2 std or U(0, 0.5) m;
    * end-effector orientation (k = env mod 8): the commanded world orientation (0: the Taylor branch), its negative (1: w < 0, same
      rotation), a turn of pi - 1e-3 (2) or pi (3) about a random axis, a turn of 1e-3 (4, just outside the Taylor branch), and the
      feed's uniform random quaternions (5-7, half of them w < 0)."""
    b = robot.body_names.index(ee)

    def tweak(feed: StateFeed):
        g = torch.Generator().manual_seed(5151)
        N = feed.num_envs
        idx = torch.arange(N)
        st = feed._stack
        for k in range(feed.num_snapshots):
            cmd = st["command"][k]
            yaw = (torch.rand(N, generator=g) * 2.0 - 1.0) * 3.14
            q = ref_math.quat_from_euler_xyz(torch.zeros(N), torch.full((N,), pitch), yaw)
            even = idx % 2 == 0
            cmd[even, 3:7] = q[even]
            des_p, des_q = ref_math.combine_frame_transforms(st["root_pos_w"][k], st["root_quat_w"][k], cmd[:, :3], cmd[:, 3:7])
            dirn = torch.randn(N, 3, generator=g)
            dirn = dirn / dirn.norm(dim=-1, keepdim=True)
            d = torch.rand(N, generator=g) * 0.5
            for m, v in ((0, 0.0), (1, 0.05), (2, 0.1), (3, 0.2)):
                d[idx % 6 == m] = v
            st["body_pos_w"][k][:, b] = des_p + dirn * d[:, None]
            axis = torch.randn(N, 3, generator=g)
            axis = axis / axis.norm(dim=-1, keepdim=True)
            m8 = idx % 8
            ang = torch.where(m8 == 2, torch.full((N,), math.pi - 1.0e-3), torch.where(m8 == 3, torch.full((N,), math.pi), torch.full((N,), 1.0e-3)))
            turned = ref_math.quat_mul(des_q, ref_math.quat_from_angle_axis(ang, axis))
            bq = st["body_quat_w"][k][:, b].clone()
            bq[m8 == 0] = des_q[m8 == 0]
            bq[m8 == 1] = -des_q[m8 == 1]
            sel = (m8 >= 2) & (m8 <= 4)
            bq[sel] = turned[sel]
            st["body_quat_w"][k][:, b] = bq
    return tweak


def dump_managers(task: str, env_cfg):
    """Side file as for the other tasks: reset events, the curriculum (host-side) and the robot init state (UNMODIFIED cfg)."""
    base = env_cfg.to_dict()
    ev = {k: v for k, v in base["events"].items() if v is not None and v.get("mode") in ("reset", "interval")}
    side = {"events": ev, "curriculum": base.get("curriculum"),
            "scene": {"robot": {"init_state": {k: list(v) for k, v in base["scene"]["robot"]["init_state"].items()
                                               if k in ("pos", "rot", "lin_vel", "ang_vel")}}}}
    with open(os.path.join(gg.CONFIGS, task + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, indent=1, sort_keys=False)


def run(task: str):
    env_spec, agent_spec, robot, ee, pitch = TASKS[task]
    steps = 5
    gg.run_task(task, _load(env_spec)(), _load(agent_spec)(), robot, N=64, steps=steps, seed=431,
                kitchen=dict(feed_tweak=reach_feed_tweak(robot, ee, pitch)))
    dump_managers(task, _load(env_spec)())
    path = os.path.join(gg.GOLDEN, task + ".npz")
    z = np.load(path)
    # the per-step tensors no reach term reads are left out (run_task records every EXTRA tensor of a kitchen run)
    unread = ("body_lin_acc_w", "command_time_left", "command_counter", "link_incoming_joint_force", "object_root_pos_w")
    rec = {k: z[k] for k in z.files if k.rpartition("/")[2] not in unread or "/in/" not in k}
    meta = json.loads(str(rec["meta_json"]))
    b = robot.body_names.index(ee)
    cmd = np.stack([rec[f"step{t}/in/command"] for t in range(steps)])
    bq = np.stack([rec[f"step{t}/in/body_quat_w"][:, b] for t in range(steps)])
    meta.update(ee_body=ee, ee_body_id=b, command_w_near_zero=int((np.abs(cmd[..., 3]) < 1e-6).sum()),
                command_w_negative=int((cmd[..., 3] < 0).sum()), ee_quat_w_negative=int((bq[..., 0] < 0).sum()))
    rec["meta_json"] = np.array(json.dumps(meta))
    # the plan blob of the LIVE cfg object (the configclass instance of the task's gym registry entry): tests/test_reach_plan.py compiles
    # the committed JSON dump and requires the very same blob, without the reference
    rec["live_cfg/blob"] = np.ascontiguousarray(compile_plan(_load(env_spec)(), robot).blob, np.int32)
    np.savez_compressed(path, **rec)
    print(f"[golden] {task}: {meta['command_w_near_zero']} commands with |w| < 1e-6, {meta['command_w_negative']} with w < 0, "
          f"{meta['ee_quat_w_negative']} end-effector quaternions with w < 0")


def main():
    for task in TASKS:
        run(task)


if __name__ == "__main__":
    main()
