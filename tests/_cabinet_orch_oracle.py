"""Test-side only: the fixtures of the Open-Drawer task's ``_reset_idx`` (tools/gen_golden_cabinet_orchestration.py) and a numpy
restatement of its reset events on a scene with two articulations -- ``reset_scene_to_default`` (envs/mdp/events.py:1096-1118) on the robot
AND the cabinet, ``reset_joints_by_offset`` / ``reset_joints_by_scale`` (:987-1049) and ``reset_root_state_uniform`` (:823-868) on either.
fp32 throughout, the reference's association (``dtype=np.float64`` restates the same formulas in fp64).  The root-state pieces are those of
tests/_manip_orch_oracle.py.  The product never imports this file."""

from __future__ import annotations

import json
import os

import numpy as np
import torch

import _manip_orch_oracle as mo
from _util import GOLDEN

F = np.float32
ROBOT_KEYS = ("root_pose", "root_vel", "joint_pos", "joint_vel")
KINDS = ("root_pose", "root_vel", "joint_pos", "joint_vel")


def joints_by(offset: bool, default_pos, default_vel, pos_limits, vel_limits, u2j, position_range, velocity_range, dtype=F):
    """reset_joints_by_offset (``offset``) / reset_joints_by_scale for the rows given: ``u2j`` their (n, 2 J) samples in [0,1).  The range
    width is an fp32 difference, as in the kernel's table of ranges (the fixtures' ranges are symmetric: the same value as the
    reference's Python-float difference rounded to fp32)."""
    J = default_pos.shape[1]
    u = np.asarray(u2j, dtype)
    pr, vr = np.asarray(position_range, F).astype(dtype), np.asarray(velocity_range, F).astype(dtype)
    sp = u[:, :J] * (pr[1] - pr[0]) + pr[0]
    sv = u[:, J:] * (vr[1] - vr[0]) + vr[0]
    dp, dv = np.asarray(default_pos, dtype), np.asarray(default_vel, dtype)
    p, v = (dp + sp, dv + sv) if offset else (dp * sp, dv * sv)
    lim, vl = np.asarray(pos_limits, dtype), np.asarray(vel_limits, dtype)
    return np.clip(p, lim[..., 0], lim[..., 1]).astype(dtype), np.clip(v, -vl, vl).astype(dtype)


def write_keys(second: str | None) -> list:
    return list(ROBOT_KEYS) + ([f"{second}_{k}" for k in KINDS] if second else [])


def new_sim_writes(N: int, J: int, second: str | None = None, J2: int = 0, fill=0.0) -> dict:
    shape = {"root_pose": (N, 7), "root_vel": (N, 6)}
    sw = {k: np.full(shape.get(k, (N, J)), fill, F) for k in ROBOT_KEYS}
    if second:
        sw.update({f"{second}_{k}": np.full(shape.get(k, (N, J2)), fill, F) for k in KINDS})
    return sw


def apply_reset_events(events: dict, ids, step_count, sim_writes: dict, trigger: dict, static: dict, draws: dict, second: str | None):
    """EventManager.apply("reset", ids, step_count) of the cfg's reset terms, in cfg order, on the rows ``ids`` of ``sim_writes``.
    ``static``: env_origins and, for the robot ("") and the second articulation ("<name>_"), ``<prefix>default_root_state``,
    ``<prefix>default_joint_pos`` / ``_vel`` and ``<prefix>soft_joint_pos_limits`` / ``_vel_limits``."""
    ids = np.asarray(ids)
    org = static["env_origins"][ids]
    for k, (name, term) in enumerate(events.items()):
        trigger["last"][k, ids], trigger["once"][k, ids] = step_count, True  # (min_step_count_between_reset = 0 on this task)
        fn, p = term["func"].rsplit(":", 1)[-1], term["params"]
        ent = (p.get("asset_cfg") or {}).get("name", "robot")
        assert ent in ("robot", second), ent
        pre = "" if ent == "robot" else f"{second}_"
        if fn == "reset_scene_to_default":
            for q in [""] + ([f"{second}_"] if second else []):  # scene.articulations, the cfg's order
                sim_writes[q + "root_pose"][ids], sim_writes[q + "root_vel"][ids] = mo.root_state_default(static[q + "default_root_state"][ids], org)
                sim_writes[q + "joint_pos"][ids], sim_writes[q + "joint_vel"][ids] = static[q + "default_joint_pos"][ids], static[q + "default_joint_vel"][ids]
        elif fn == "reset_root_state_uniform":
            sim_writes[pre + "root_pose"][ids], sim_writes[pre + "root_vel"][ids] = mo.root_state_uniform(
                static[pre + "default_root_state"][ids], org, draws[name][ids], p.get("pose_range"), p.get("velocity_range"))
        elif fn in ("reset_joints_by_offset", "reset_joints_by_scale"):
            sim_writes[pre + "joint_pos"][ids], sim_writes[pre + "joint_vel"][ids] = joints_by(
                fn.endswith("offset"), static[pre + "default_joint_pos"][ids], static[pre + "default_joint_vel"][ids],
                static[pre + "soft_joint_pos_limits"][ids], static[pre + "soft_joint_vel_limits"][ids], draws[name][ids], p["position_range"],
                p["velocity_range"])
        else:
            raise NotImplementedError(fn)


class CabinetOrchGolden:
    """tests/golden/cabinet[_events]_orchestration.{npz,_in.npz,json}: the REAL ``_reset_idx`` of the Franka cabinet cfg over recording
    assets for the robot and the cabinet, ``reset()`` + 40 steps."""

    def __init__(self, which: str):
        from isaaclab_amd.robots import ROBOTS

        self.name = {"shipped": "cabinet_orchestration", "events": "cabinet_events_orchestration"}[which]
        self.z = np.load(os.path.join(GOLDEN, self.name + ".npz"))
        self.zi = np.load(os.path.join(GOLDEN, self.name + "_in.npz"))
        self.meta = json.loads(str(self.z["meta_json"]))
        with open(os.path.join(GOLDEN, self.name + ".json")) as f:
            self.fixture = json.load(f)
        self.robot = ROBOTS[self.fixture["robot"]]
        self.N, self.steps, self.second = self.meta["num_envs"], self.meta["steps"], self.meta["second_articulation"]
        self.events = {k: v for k, v in self.fixture["env"]["events"].items() if v is not None and v.get("mode") == "reset"}
        self.tags = ["reset"] + [f"step{s}" for s in range(self.steps)]
        self.write_keys = write_keys(self.second)
        self.J2 = len(self.meta["cabinet"]["joint_names"])

    def a(self, key) -> np.ndarray:
        return np.ascontiguousarray((self.zi if key in self.zi.files else self.z)[key])

    def t(self, key) -> torch.Tensor:
        return torch.from_numpy(self.a(key))

    def static(self) -> dict:
        return {k[len("static/"):]: self.a(k) for k in self.zi.files if k.startswith("static/")}

    def draws(self, slot: int) -> dict:
        """The uniform tables of ``slot`` (0 = env.reset(), 1 + t = step t)."""
        return {n: self.a("draws/" + n)[slot] for n in self.events}

    def reset_ids(self, t: int) -> np.ndarray:
        return self.a(f"step{t}/reset_env_ids")

    def feed(self, device="cpu", num_snapshots=None):
        """A generated feed with the fixture's static tensors: nothing the reset events write reads the per-step state, and the only
        termination of the task is the time-out."""
        from isaaclab_amd.state_feed import STATIC, StateFeed

        feed = StateFeed(self.robot, self.N, device, seed=self.meta["seed"], num_snapshots=num_snapshots or self.steps + 1)
        for n in STATIC:
            feed[n].copy_(self.t("static/" + n))
        return feed


def replay(g: CabinetOrchGolden):
    """The restatement over a fixture's inputs: yields (tag, reset ids, sim_writes, trigger, common_step_counter) after ``reset()`` and
    after every step.  The reset ids are derived, not read: a time-out when the episode length reaches the limit."""
    st, N = g.static(), g.N
    sw = new_sim_writes(N, st["default_joint_pos"].shape[1], g.second, g.J2)
    trig = {"last": np.zeros((len(g.events), N), np.int64), "once": np.zeros((len(g.events), N), bool)}
    ids = np.arange(N)
    apply_reset_events(g.events, ids, 0, sw, trig, st, g.draws(0), g.second)
    yield "reset", ids, sw, trig, 0
    ep = g.a("reset/episode_length_buf").copy()
    for t in range(g.steps):
        ep += 1
        ids = np.nonzero(ep >= g.meta["max_episode_length"])[0]
        if len(ids):
            apply_reset_events(g.events, ids, t + 1, sw, trig, st, g.draws(1 + t), g.second)
        ep[ids] = 0
        yield f"step{t}", ids, sw, trig, t + 1
