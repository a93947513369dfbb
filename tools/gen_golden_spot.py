"""TEST INFRASTRUCTURE (build container only): the Isaac-Velocity-Flat-Spot-v0 fixtures, from the REAL reference.

    python tools/gen_golden_spot.py

Writes
  * ``isaaclab_amd/configs/Isaac-Velocity-Flat-Spot-v0.json`` (``SpotFlatEnvCfg()`` / ``SpotFlatPPORunnerCfg()`` through
    ``oracle.gen_golden.dump_cfg``) and its ``.managers.json`` side file (reset / interval events, curriculum, robot init state);
  * ``tests/golden/Isaac-Velocity-Flat-Spot-v0.npz``: ``oracle.gen_golden.run_task`` -- the real action, termination, reward and
    observation managers with Spot's own 14 reward terms -- on a feed tweaked so that every branch of those terms is taken;
  * ``tests/golden/spot_events.npz``: the real ``reset_joints_around_default`` with its two ``torch.rand`` draws recorded.

Reuses ``oracle/gen_golden.py`` and ``oracle/gen_golden_events.py`` as they are (imported, not edited).  Deterministic: a second run
reproduces the files bit for bit.
"""

from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)
from oracle import gen_golden_events as gge  # noqa: E402

from isaaclab_amd.robots import SPOT  # noqa: E402
from isaaclab_amd.state_feed import StateFeed  # noqa: E402

TASK = "Isaac-Velocity-Flat-Spot-v0"
_SPOT_PKG = "isaaclab_tasks.manager_based.locomotion.velocity.config.spot"


def spot_feed_tweak(feed: StateFeed):
    """Push the synthetic feed across every branch of the Spot terms (applied to every snapshot):
    zero commands on every 4th env, with |v_b,xy| below and above the 0.5 m/s threshold; foot force histories around the 1 N contact
    threshold; foot heights around the 0.1 m clearance target.  Air / contact times already straddle 0.3 s and 0.5 s (U(0, 0.8))."""
    g = torch.Generator().manual_seed(2024)
    N = feed.num_envs
    feet = [i for i, n in enumerate(feed.robot.body_names) if n.endswith("_foot")]
    st = feed._stack
    for k in range(feed.num_snapshots):
        cmd = st["command"][k]
        cmd[0::4] = 0.0
        v = st["root_lin_vel_w"][k]
        slow = torch.arange(N) % 8 == 0  # half of the zero-command envs stand still, the other half drift (|v| ~ 0.5 to 1.1 m/s)
        v[slow] *= 0.2
        fast = torch.arange(N) % 8 == 4
        v[fast] = v[fast] / v[fast].norm(dim=-1, keepdim=True).clamp_min(1e-6) * (0.5 + 0.6 * torch.rand(int(fast.sum()), 1, generator=g))
        F = st["net_forces_w_history"][k]
        near = torch.rand(N, F.shape[1], len(feet), generator=g) < 0.4  # magnitudes rescaled into (0.5, 1.5) N
        for j, b in enumerate(feet):
            f = F[:, :, b]
            mag = 0.5 + torch.rand(N, F.shape[1], generator=g)
            unit = f / f.norm(dim=-1, keepdim=True).clamp_min(1e-6)
            unit[f.norm(dim=-1) == 0] = torch.tensor([0.0, 0.0, 1.0])
            f[near[:, :, j]] = (unit * mag.unsqueeze(-1))[near[:, :, j]]
        bp = st["body_pos_w"][k]
        bp[:, feet, 2] = 0.1 + torch.randn(N, len(feet), generator=g) * 0.05


def dump_managers(env_cfg):
    """Side file as for the other velocity tasks: reset / interval events, curriculum, robot init state (UNMODIFIED cfg)."""
    base = env_cfg.to_dict()
    ev = {k: v for k, v in base["events"].items() if v is not None and v.get("mode") in ("reset", "interval")}
    side = {"events": ev, "curriculum": base["curriculum"],
            "scene": {"robot": {"init_state": {k: list(v) for k, v in base["scene"]["robot"]["init_state"].items()
                                               if k in ("pos", "rot", "lin_vel", "ang_vel")}}}}
    with open(os.path.join(gg.CONFIGS, TASK + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, indent=1, sort_keys=False)


def events_fixture():
    """reset_joints_around_default (spot/mdp/events.py:26-60) on gen_golden_events' fake asset: defaults N(0, 0.6), soft position limits
    of width 1 around N(0, 0.3) centres and velocity limits U(0.05, 0.25) -- so +-0.2 / +-2.5 ranges cross the limits on many joints."""
    import importlib

    from isaaclab.managers import SceneEntityCfg

    spot_events = importlib.import_module(f"{_SPOT_PKG}.mdp.events")
    N, J = 96, SPOT.num_joints
    g = torch.Generator().manual_seed(31)
    asset = gge.FakeAsset(N, J, g)
    env = types.SimpleNamespace(scene=gge.FakeScene(robot=asset))
    mask = torch.rand(N, generator=g) < 0.5
    mask[0], mask[N - 1] = True, False
    ids = mask.nonzero(as_tuple=False).squeeze(-1)
    k = len(ids)
    rec = {"mask": mask.numpy()}
    for name in ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits"):
        rec[name] = getattr(asset.data, name).numpy().copy()
    prange, vrange = (-0.2, 0.2), (-2.5, 2.5)  # flat_env_cfg.py SpotEventCfg.reset_robot_joints
    torch.manual_seed(201)
    spot_events.reset_joints_around_default(env, ids, prange, vrange, SceneEntityCfg("robot"))
    torch.manual_seed(201)  # the same two sample_uniform draws, re-drawn (utils/math.py: torch.rand(*size) * (upper - lower) + lower)
    u_p, u_v = torch.rand(k, J), torch.rand(k, J)
    assert torch.equal(asset.writes["joint_pos"][1], ids)
    rec["u_pos"], rec["u_vel"] = gge.scatter(N, ids, u_p).numpy(), gge.scatter(N, ids, u_v).numpy()
    rec["pos_out"] = gge.scatter(N, ids, asset.writes["joint_pos"][0]).numpy()
    rec["vel_out"] = gge.scatter(N, ids, asset.writes["joint_vel"][0]).numpy()
    rec["ranges"] = np.array([*prange, *vrange], dtype=np.float32)
    dp = asset.data.default_joint_pos[ids]
    lim = asset.data.soft_joint_pos_limits[ids]
    crossing = ((dp - 0.2 < lim[..., 0]) | (dp + 0.2 > lim[..., 1])).sum().item()
    rec["meta"] = np.array(json.dumps(dict(N=N, J=J, reset_envs=k, joints_crossing_a_limit=int(crossing))))
    np.savez_compressed(os.path.join(gg.GOLDEN, "spot_events.npz"), **rec)
    print(f"[golden] spot_events: {k} reset envs, {crossing} (env, joint) ranges cross a soft position limit")


def main():
    import importlib

    env_cfg_cls = importlib.import_module(f"{_SPOT_PKG}.flat_env_cfg").SpotFlatEnvCfg
    agent_cls = importlib.import_module(f"{_SPOT_PKG}.agents.rsl_rl_ppo_cfg").SpotFlatPPORunnerCfg
    gg.run_task(TASK, env_cfg_cls(), agent_cls(), SPOT, N=64, steps=5, seed=111, kitchen=dict(feed_tweak=spot_feed_tweak))
    # run_task records every EXTRA tensor of a kitchen run; the state tensors added to the feed after this fixture (for other tasks'
    # terms, none read by Spot's) are left out, so that the file stays the one committed
    path = os.path.join(gg.GOLDEN, TASK + ".npz")
    z = np.load(path)
    later = ("link_incoming_joint_force", "body_quat_w", "object_root_pos_w")
    rec = {k: z[k] for k in z.files if k.rpartition("/")[2] not in later or "/in/" not in k}
    np.savez_compressed(path, **rec)
    dump_managers(env_cfg_cls())
    events_fixture()


if __name__ == "__main__":
    main()
