"""Test-side only: the fixtures of the manipulation tasks' ``_reset_idx`` (tools/gen_golden_manip_orchestration.py) and a numpy
restatement of its three pieces -- ``reset_scene_to_default`` (envs/mdp/events.py:1096-1118), ``reset_root_state_uniform`` on any asset
(:823-868) and ``modify_reward_weight`` (envs/mdp/curriculums.py:21-36) -- plus ``reset_joints_by_scale`` (:987-1015), which the Reach
fixture needs.  fp32 throughout, the reference's association.  The product never imports this file."""

from __future__ import annotations

import json
import os

import numpy as np
import torch

from _pose_command_cases import full_body_tensors
from _util import GOLDEN

F = np.float32
AXES = ("x", "y", "z", "roll", "pitch", "yaw")


# ---------------------------------------------------------------------------------------------------- the restatement
def axis_ranges(d) -> np.ndarray:
    d = d or {}
    return np.array([d.get(k, (0.0, 0.0)) for k in AXES], F)  # (6, 2)


def quat_from_euler_xyz(roll, pitch, yaw):
    cy, sy, cr, sr = np.cos(yaw * F(0.5)), np.sin(yaw * F(0.5)), np.cos(roll * F(0.5)), np.sin(roll * F(0.5))
    cp, sp = np.cos(pitch * F(0.5)), np.sin(pitch * F(0.5))
    return np.stack([cy * cr * cp + sy * sr * sp, cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp], -1).astype(F)


def quat_mul(q1, q2):
    w1, x1, y1, z1 = (q1[..., i] for i in range(4))
    w2, x2, y2, z2 = (q2[..., i] for i in range(4))
    ww, yy, zz = (z1 + x1) * (x2 + y2), (w1 - y1) * (w2 + z2), (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = F(0.5) * (xx + (z1 - x1) * (x2 - y2))
    return np.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                     qq - zz + (z1 + y1) * (w2 - x2)], -1).astype(F)


def root_state_uniform(default13, origins, u12, pose_range, velocity_range):
    """Rows of (pose (n,7), vel (n,6)) for the envs given: ``u12`` their (n,12) samples in [0,1)."""
    d, o, u = np.asarray(default13, F), np.asarray(origins, F), np.asarray(u12, F)
    pr, vr = axis_ranges(pose_range), axis_ranges(velocity_range)
    rs = u[:, :6] * (pr[:, 1] - pr[:, 0]) + pr[:, 0]
    vs = u[:, 6:] * (vr[:, 1] - vr[:, 0]) + vr[:, 0]
    pos = d[:, 0:3] + o + rs[:, 0:3]
    quat = quat_mul(d[:, 3:7], quat_from_euler_xyz(rs[:, 3], rs[:, 4], rs[:, 5]))
    return np.concatenate([pos, quat], -1).astype(F), (d[:, 7:13] + vs).astype(F)


def root_state_default(default13, origins):
    d = np.asarray(default13, F).copy()
    d[:, 0:3] += np.asarray(origins, F)
    return d[:, :7], d[:, 7:]


def joints_by_scale(default_pos, default_vel, pos_limits, vel_limits, u2j, position_range, velocity_range):
    J = default_pos.shape[1]
    u = np.asarray(u2j, F)
    p = default_pos * (u[:, :J] * F(position_range[1] - position_range[0]) + F(position_range[0]))
    v = default_vel * (u[:, J:] * F(velocity_range[1] - velocity_range[0]) + F(velocity_range[0]))
    return np.clip(p, pos_limits[..., 0], pos_limits[..., 1]).astype(F), np.clip(v, -vel_limits, vel_limits).astype(F)


def modify_reward_weight(weights: dict, common_step_counter: int, any_reset: bool, terms) -> dict:
    """CurriculumManager.compute inside ``_reset_idx``: only when an env resets; ``terms``: (term_name, weight, num_steps) in cfg order."""
    out = dict(weights)
    if any_reset:
        for term_name, weight, num_steps in terms:
            if common_step_counter > num_steps:
                out[term_name] = weight
    return out


def apply_reset_events(events: dict, ids, step_count, sim_writes: dict, trigger: dict, static: dict, draws: dict, object_name=None):
    """EventManager.apply("reset", ids, step_count) of the cfg's reset terms, in cfg order, on the rows ``ids`` of ``sim_writes``."""
    ids = np.asarray(ids)
    org = static["env_origins"][ids]
    for k, (name, term) in enumerate(events.items()):
        trigger["last"][k, ids], trigger["once"][k, ids] = step_count, True  # (min_step_count_between_reset = 0 on these tasks)
        fn, p = term["func"].rsplit(":", 1)[-1], term["params"]
        if fn == "reset_scene_to_default":
            if object_name is not None:
                sim_writes["object_root_pose"][ids], sim_writes["object_root_vel"][ids] = root_state_default(static["default_object_root_state"][ids], org)
            sim_writes["root_pose"][ids], sim_writes["root_vel"][ids] = root_state_default(static["default_root_state"][ids], org)
            sim_writes["joint_pos"][ids], sim_writes["joint_vel"][ids] = static["default_joint_pos"][ids], static["default_joint_vel"][ids]
        elif fn == "reset_root_state_uniform":
            ent = (p.get("asset_cfg") or {}).get("name", "robot")
            pre, d = ("object_", static["default_object_root_state"]) if ent == object_name else ("", static["default_root_state"])
            assert ent in ("robot", object_name)
            sim_writes[pre + "root_pose"][ids], sim_writes[pre + "root_vel"][ids] = root_state_uniform(d[ids], org, draws[name][ids], p.get("pose_range"), p.get("velocity_range"))
        elif fn == "reset_joints_by_scale":
            sim_writes["joint_pos"][ids], sim_writes["joint_vel"][ids] = joints_by_scale(
                static["default_joint_pos"][ids], static["default_joint_vel"][ids], static["soft_joint_pos_limits"][ids],
                static["soft_joint_vel_limits"][ids], draws[name][ids], p["position_range"], p["velocity_range"])
        else:
            raise NotImplementedError(fn)


# ---------------------------------------------------------------------------------------------------- the fixtures
class ManipOrchGolden:
    """tests/golden/<reach|lift>_manip_orchestration.{npz,_in.npz,json}: the REAL ``_reset_idx`` with the tasks' own event and curriculum
    terms over recording assets, ``reset()`` + 40 steps."""

    def __init__(self, which: str):
        from isaaclab_amd.robots import ROBOTS

        self.name = f"{which}_manip_orchestration"
        self.z = np.load(os.path.join(GOLDEN, self.name + ".npz"))
        self.zi = np.load(os.path.join(GOLDEN, self.name + "_in.npz"))
        self.meta = json.loads(str(self.z["meta_json"]))
        with open(os.path.join(GOLDEN, self.name + ".json")) as f:
            self.fixture = json.load(f)
        self.robot = ROBOTS[self.fixture["robot"]]
        self.N, self.steps, self.body_idx = self.meta["num_envs"], self.meta["steps"], self.meta["body_idx"]
        self.object = self.meta["object"]
        self.events = {k: v for k, v in self.fixture["env"]["events"].items() if v is not None and v.get("mode") == "reset"}
        self.curriculum = [(c["term_name"], c["weight"], c["num_steps"]) for c in self.meta["curriculum"].values()]
        self.tags = ["reset"] + [f"step{s}" for s in range(self.steps)]
        self.write_keys = ["root_pose", "root_vel", "joint_pos", "joint_vel"] + (["object_root_pose", "object_root_vel"] if self.object else [])

    def a(self, key) -> np.ndarray:
        return np.ascontiguousarray((self.zi if key in self.zi.files else self.z)[key])

    def t(self, key) -> torch.Tensor:
        return torch.from_numpy(self.a(key))

    def log(self, tag: str) -> dict:
        return json.loads(str(self.z[f"{tag}/log_json"]))

    def static(self) -> dict:
        return {k[len("static/"):]: self.a(k) for k in self.zi.files if k.startswith("static/")}

    def draws(self, slot: int) -> dict:
        """The uniform tables of ``slot`` (0 = env.reset(), 1 + t = step t)."""
        out = {n: self.t("draws/" + n)[slot] for n in self.events}
        out["command"] = self.t("draws/command")[slot]
        return out

    def weights(self, tag) -> dict:
        return dict(zip(self.meta["reward_terms"], self.a(f"{tag}/weights").tolist()))

    def feed(self, device="cpu"):
        from isaaclab_amd.state_feed import STATIC, StateFeed

        NB = self.robot.num_bodies
        snaps = []
        for k, tag in enumerate(self.tags):
            d = {n: self.t(f"{tag}/in/{n}") for n in ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w", "joint_pos", "joint_vel")}
            d["body_pos_w"], d["body_quat_w"] = full_body_tensors(self.t(f"{tag}/in/ee_pos_w"), self.t(f"{tag}/in/ee_quat_w"), NB, self.body_idx, 3000 + k)
            d["command"] = torch.zeros(self.N, 7)  # unused: the env owns its command term
            d["net_forces_w_history"] = torch.zeros(self.N, 1, NB, 3)  # (no term of these tasks reads a contact sensor)
            if self.object:
                d["object_root_pos_w"] = self.t(f"{tag}/in/object_root_pos_w")
            d.update({n: self.t(f"static/{n}") for n in STATIC})
            snaps.append(d)
        return StateFeed.from_tensors(self.robot, snaps, device=device, gravity_dir=self.meta["gravity_dir"])

    def reset_ids(self, t: int) -> np.ndarray:
        return self.a(f"step{t}/reset_env_ids")


def replay(g: ManipOrchGolden):
    """The restatement over a fixture's inputs: yields (tag, reset ids, sim_writes, trigger, weights) after ``reset()`` and after every step.
    The reset ids are derived, not read: a time-out when the episode length reaches the limit, Lift's ``object_dropping`` (the object's z
    below its ``minimum_height``)."""
    st, N = g.static(), g.N
    J = st["default_joint_pos"].shape[1]
    sw = {"root_pose": np.zeros((N, 7), F), "root_vel": np.zeros((N, 6), F), "joint_pos": np.zeros((N, J), F), "joint_vel": np.zeros((N, J), F)}
    if g.object:
        sw.update(object_root_pose=np.zeros((N, 7), F), object_root_vel=np.zeros((N, 6), F))
    trig = {"last": np.zeros((len(g.events), N), np.int64), "once": np.zeros((len(g.events), N), bool)}
    weights = {n: t["weight"] for n, t in g.fixture["env"]["rewards"].items() if t is not None}
    ids = np.arange(N)
    weights = modify_reward_weight(weights, 0, True, g.curriculum)
    apply_reset_events(g.events, ids, 0, sw, trig, st, {k: v.numpy() for k, v in g.draws(0).items()}, g.object)
    yield "reset", ids, sw, trig, weights
    ep = g.a("reset/episode_length_buf").copy()
    drop = None
    for name, term in g.fixture["env"]["terminations"].items():
        if term is not None and term["func"].endswith("root_height_below_minimum"):
            drop = float(term["params"]["minimum_height"])
    for t in range(g.steps):
        ep += 1
        reset = ep >= g.meta["max_episode_length"]
        if drop is not None:
            reset |= g.a(f"step{t}/in/object_root_pos_w")[:, 2] < F(drop)
        ids = np.nonzero(reset)[0]
        weights = modify_reward_weight(weights, t + 1, len(ids) > 0, g.curriculum)
        if len(ids):
            apply_reset_events(g.events, ids, t + 1, sw, trig, st, {k: v.numpy() for k, v in g.draws(1 + t).items()}, g.object)
        ep[ids] = 0
        yield f"step{t}", ids, sw, trig, weights
