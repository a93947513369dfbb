"""fp64 statements of the manipulation/inhand/mdp terms (isaaclab_tasks .../manipulation/inhand/mdp: observations.py:20-38, rewards.py:20-96,
terminations.py:18-83) and of the root observations on the rigid object, the feed tweak that takes each of their branches, and the branch
counts -- shared by tests/test_inhand_plan.py, tests/test_inhand_gpu.py and tools/gen_golden_inhand.py (which applies the same tweak to
the feed the reference's managers run on).  The formulas restate the reference's utils/math.py helpers (quat_mul :464-500, quat_conjugate
:225-236, axis_angle_from_quat :646-675, quat_error_magnitude :678-690) in float64 on the fp32 inputs."""

from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

TASK = "Isaac-Repose-Cube-Allegro-v0"
TASK_NOVEL = "Isaac-Repose-Cube-Allegro-NoVelObs-v0"
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROBOT = "allegro_hand"
INHAND = "isaaclab_tasks.manager_based.manipulation.inhand.mdp"
MDP = "isaaclab.envs.mdp"
A, J = 16, 16
# policy group columns: joint_pos 16, joint_vel 16, object_pos 3, object_quat 4, object_lin_vel 3, object_ang_vel 3, goal_pose 7,
# goal_quat_diff 4, last_action 16; NoVelObs drops joint_vel, object_lin_vel, object_ang_vel
D, D_NOVEL = 72, 50
COLS = {"joint_pos": (0, 16), "joint_vel": (16, 32), "object_pos": (32, 35), "object_quat": (35, 39), "object_lin_vel": (39, 42),
        "object_ang_vel": (42, 45), "goal_pose": (45, 52), "goal_quat_diff": (52, 56), "last_action": (56, 72)}
COLS_NOVEL = {"joint_pos": (0, 16), "object_pos": (16, 19), "object_quat": (19, 23), "goal_pose": (23, 30), "goal_quat_diff": (30, 34),
              "last_action": (34, 50)}
SUCCESS_THRESHOLD, ROT_EPS, NUM_SUCCESS, REACH = 0.1, 0.1, 50, 0.3  # the cfg's orientation_success_threshold, rot_eps, num_success, threshold
GOAL_REACH = 0.25  # threshold of the object_away_from_goal termination the tests add (the task cfg does not use the term)
ANGLE_MARGIN, DIST_MARGIN = 1.0e-4, 1.0e-4  # how far the tweak keeps orientation errors / distances from the thresholds
FAR_SHIFT = (400.0, -300.0, 0.0)  # where the "far from the origin" envs are moved: fp32 rounds world coordinates there at 3e-5 m
NAMES = ("root_pos_w", "command", "env_origins", "object_root_pos_w", "object_root_quat_w", "object_root_lin_vel_w",
         "object_root_ang_vel_w", "command_consecutive_success")
SUCCESS_COUNTS = (0.0, 49.0, 50.0, 51.0)


def f32(x: float) -> float:
    return float(np.float32(x))


def fixture_path(task: str = TASK) -> str:
    return os.path.join(GOLDEN_DIR, task + ".json")


# ---- quaternions w, x, y, z in whatever dtype they come
def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def quat_conj(q: torch.Tensor) -> torch.Tensor:
    return torch.cat([q[..., :1], -q[..., 1:]], dim=-1)


def quat_about(angle: torch.Tensor, axis: torch.Tensor) -> torch.Tensor:
    """The unit quaternion of a rotation by ``angle`` about the unit vectors ``axis``."""
    h = (angle / 2).unsqueeze(-1)
    return torch.cat([torch.cos(h), axis * torch.sin(h)], dim=-1)


def quat_error_magnitude(q1: torch.Tensor, q2: torch.Tensor) -> torch.Tensor:
    """The rotation angle of q1 * conj(q2) in [0, pi]: 2 atan2(||xyz||, |w|) (what ||axis_angle_from_quat|| amounts to)."""
    d = quat_mul(q1, quat_conj(q2))
    return 2.0 * torch.atan2(d[..., 1:].norm(dim=-1), d[..., 0].abs())


def inhand_terms(s: dict) -> dict:
    """Every in-hand term's raw value in fp64 from the feed tensors ``s`` (current snapshot); the thresholds the comparisons use are the
    fp32 roundings the fp32 reference compares against."""
    d = lambda n: s[n].double()  # noqa: E731
    oq, goal = d("object_root_quat_w"), d("command")[:, 3:7]
    obj_e = d("object_root_pos_w") - d("env_origins")
    dth = quat_error_magnitude(oq, goal)
    d_goal = (d("command")[:, :3] - obj_e).norm(dim=-1)
    d_robot = (d("root_pos_w") - d("object_root_pos_w")).norm(dim=-1)
    return {"dtheta": dth, "track_orientation_inv_l2": 1.0 / (dth + f32(ROT_EPS)), "success_bonus": (dth <= f32(SUCCESS_THRESHOLD)).double(),
            "track_pos_l2": d_goal, "goal_distance": d_goal, "robot_distance": d_robot,
            "max_consecutive_success": d("command_consecutive_success") >= float(NUM_SUCCESS),
            "object_away_from_robot": d_robot > f32(REACH), "object_away_from_goal": d_goal > f32(GOAL_REACH),
            "object_pos": obj_e, "object_quat": oq, "object_lin_vel": d("object_root_lin_vel_w"), "object_ang_vel": d("object_root_ang_vel_w"),
            "goal_quat_diff": quat_mul(oq, quat_conj(goal))}


def quat_unique(q: torch.Tensor) -> torch.Tensor:
    return torch.where(q[..., 0:1] < 0, -q, q)


def position_rounding(s: dict) -> torch.Tensor:
    """Per-env allowance for the fp32 rounding of world positions far from the origin: two roundings of the largest coordinate involved
    (the env-frame subtraction, then the difference to the goal), which the fp32 reference has as well."""
    big = torch.stack([s[n].double().abs().amax(-1) for n in ("root_pos_w", "object_root_pos_w", "env_origins")]).amax(0) + 1.0
    return 2.0 * big * 2.0 ** -24 * 2.0


def inhand_tweak(feed, gen: torch.Generator) -> None:
    """Every branch of the in-hand terms on a random feed, applied to every snapshot (the feed serves the object state from here on).
    Env e, with p = e mod 16 and r = (e // 16) mod 4:
    * p = 7: the whole env (origin, robot root, object) moved by FAR_SHIFT, far from the world origin;
    * orientation, goal = command[:, 3:7] against the object's quaternion q -- p = 0: goal = q bit for bit (error exactly 0); p = 1 / 2:
      an error of 0.1 rad minus / plus a margin in [1e-4, 0.02] rad (both sides of orientation_success_threshold); p = 3: within 2e-3 rad
      of pi; p = 4: goal = -q (the opposite sign, error 0); p = 5: the negated goal of a p = 1 / 2 construction; other p: the feed's
      random pair (one that falls within 2e-4 rad of the threshold gets goal = q);
    * position, command[:, :3] (the env frame) against the object -- p = 8: on the object; p = 9 / 10: GOAL_REACH minus / plus a margin
      in [2e-3, 0.05] m from it; other p: 0.02 m away in a random direction;
    * p = 12 / 13: the object REACH minus / plus a margin in [2e-3, 0.05] m from the robot root in a random direction (any other env
      whose object lies within 2e-3 m of REACH is moved 4e-3 m beyond it);
    * p = 14 / 15: command_consecutive_success = SUCCESS_COUNTS[r] (0, 49, 50, 51 around num_success = 50)."""
    feed.ensure_object_state()
    st, N = feed._stack, feed.num_envs
    dev = st["object_root_pos_w"].device
    idx = torch.arange(N)
    p, r = (idx % 16).to(dev), ((idx // 16) % 4).to(dev)
    far = p == 7
    shift = torch.tensor(FAR_SHIFT, device=dev)
    feed._static["env_origins"][far] += shift
    origins = feed._static["env_origins"]
    for k in range(feed.num_snapshots):
        for n in ("root_pos_w", "object_root_pos_w"):
            st[n][k][far] += shift
        u = lambda lo, hi: (torch.rand(N, generator=gen, dtype=torch.float64) * (hi - lo) + lo).to(dev)  # noqa: E731
        unit = lambda: torch.nn.functional.normalize(torch.randn(N, 3, generator=gen, dtype=torch.float64), dim=-1).to(dev)  # noqa: E731
        root, obj, oq, cmd = st["root_pos_w"][k], st["object_root_pos_w"][k], st["object_root_quat_w"][k], st["command"][k]
        # the object against the robot root (before the goal position is placed against the object)
        side = torch.where(p == 12, -1.0, 1.0).double()
        sel = (p == 12) | (p == 13)
        obj[sel] = (root.double() + unit() * (f32(REACH) + side * u(2.0e-3, 0.05)).unsqueeze(-1)).float()[sel]
        # (an untweaked env whose object happens to lie within 2e-3 m of REACH is moved 4e-3 m beyond it: no env sits on the threshold)
        d = root.double() - obj.double()
        near = ((d.norm(dim=-1) - f32(REACH)).abs() < 2.0e-3) & ~sel
        obj[near] = (root.double() - torch.nn.functional.normalize(d, dim=-1) * (f32(REACH) + 4.0e-3)).float()[near]
        # the goal position in the env frame
        dist = torch.full((N,), 0.02, dtype=torch.float64, device=dev)
        dist = torch.where(p == 8, torch.zeros_like(dist), dist)
        m = u(2.0e-3, 0.05)
        dist = torch.where(p == 9, f32(GOAL_REACH) - m, torch.where(p == 10, f32(GOAL_REACH) + m, dist))
        cmd[:, :3] = ((obj - origins).double() + unit() * dist.unsqueeze(-1)).float()
        # the goal orientation: conj(rot) * q is at the angle of rot from q
        margin = u(ANGLE_MARGIN, 0.02)
        angle = torch.where(r % 2 == 0, f32(SUCCESS_THRESHOLD) - margin, f32(SUCCESS_THRESHOLD) + margin)  # (p = 5: either side)
        angle = torch.where(p == 1, f32(SUCCESS_THRESHOLD) - margin, torch.where(p == 2, f32(SUCCESS_THRESHOLD) + margin, angle))
        angle = torch.where(p == 3, math.pi - u(1.0e-4, 2.0e-3), angle)
        placed = quat_mul(quat_conj(quat_about(angle, unit())), oq.double()).float()
        goal = cmd[:, 3:7].clone()
        for case, val in ((0, oq), (1, placed), (2, placed), (3, placed), (4, -oq), (5, -placed)):
            goal[p == case] = val[p == case]
        # (likewise an untweaked pair within 2e-4 rad of the threshold: its goal becomes the object's quaternion)
        near = ((quat_error_magnitude(oq.double(), goal.double()) - f32(SUCCESS_THRESHOLD)).abs() < 2.0e-4) & (p > 5)
        goal[near] = oq[near]
        cmd[:, 3:7] = goal
        cs = st["command_consecutive_success"][k]
        for case, v in enumerate(SUCCESS_COUNTS):
            cs[(p >= 14) & (r == case)] = v


def branch_counts(snaps: list[dict]) -> dict:
    """How often each branch occurs over the snapshots ``snaps`` (dicts of feed tensors), and how far the tweaked cases stay from the
    thresholds (fp64, on the fp32 tensors) -- what the golden's ``meta_json`` records and the tests require."""
    c = dict.fromkeys(("dtheta_zero", "dtheta_below_threshold", "dtheta_above_threshold", "dtheta_near_pi", "goal_opposite_sign", "object_w_negative",
                       "object_w_positive", "diff_w_negative", "diff_w_positive", "success_0", "success_49", "success_50", "success_51",
                       "within_reach", "out_of_reach", "on_goal", "near_goal", "away_from_goal", "far_from_origin"), 0)
    min_angle = min_dist = math.inf
    for s in snaps:
        s = {n: v.cpu() for n, v in s.items()}
        t = inhand_terms(s)
        dth = t["dtheta"]
        c["dtheta_zero"] += int((dth == 0.0).sum())
        c["dtheta_below_threshold"] += int(((dth > 0.05) & (dth <= f32(SUCCESS_THRESHOLD))).sum())
        c["dtheta_above_threshold"] += int(((dth > f32(SUCCESS_THRESHOLD)) & (dth < 0.15)).sum())
        c["dtheta_near_pi"] += int((dth > math.pi - 3.0e-3).sum())
        c["goal_opposite_sign"] += int((s["command"][:, 3:7] == -s["object_root_quat_w"]).all(-1).sum())
        c["object_w_negative"] += int((s["object_root_quat_w"][:, 0] < 0).sum())
        c["object_w_positive"] += int((s["object_root_quat_w"][:, 0] > 0).sum())
        c["diff_w_negative"] += int((t["goal_quat_diff"][:, 0] < 0).sum())
        c["diff_w_positive"] += int((t["goal_quat_diff"][:, 0] > 0).sum())
        for v in SUCCESS_COUNTS:
            c[f"success_{int(v)}"] += int((s["command_consecutive_success"] == v).sum())
        c["within_reach"] += int((~t["object_away_from_robot"]).sum())
        c["out_of_reach"] += int(t["object_away_from_robot"].sum())
        c["on_goal"] += int((t["goal_distance"] < 1.0e-4).sum())
        c["near_goal"] += int(((t["goal_distance"] > 0.15) & ~t["object_away_from_goal"]).sum())
        c["away_from_goal"] += int(t["object_away_from_goal"].sum())
        c["far_from_origin"] += int((s["root_pos_w"].abs().amax(-1) > 100.0).sum())
        nz = dth > 0.0
        if bool(nz.any()):
            min_angle = min(min_angle, float((dth[nz] - f32(SUCCESS_THRESHOLD)).abs().min()))
        min_dist = min(min_dist, float((t["robot_distance"] - f32(REACH)).abs().min()), float((t["goal_distance"] - f32(GOAL_REACH)).abs().min()))
    c["min_angle_margin"], c["min_distance_margin"] = min_angle, min_dist
    return c


def load_fixture(task: str = TASK) -> dict:
    """The committed cfg dump (tests/golden/<task>.json + .managers.json), through the path form of ``load_task_cfg``."""
    from isaaclab_amd.env import load_task_cfg

    return load_task_cfg(fixture_path(task))


def golden():
    """``_util.Golden`` of the in-hand fixture (its cfg dump lies under tests/golden; its snapshots also carry the object state)."""
    from _util import Golden
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import DYNAMIC, EXTRA, OBJECT_STATE, STATIC, StateFeed

    class _Golden(Golden):
        def snapshots(self):
            out = []
            for tag in ["reset"] + [f"step{k}" for k in range(self.steps)]:
                d = {n: self.t(f"{tag}/in/{n}") for n in DYNAMIC + EXTRA + OBJECT_STATE if f"{tag}/in/{n}" in self.z}
                d.update({n: self.t(f"static/{n}") for n in STATIC})
                out.append(d)
            return out

        def feed(self, device="cpu"):
            return StateFeed.from_tensors(self.robot, self.snapshots(), device=device, gravity_dir=self.meta["gravity_dir"])

    g = _Golden.__new__(_Golden)
    g.task = TASK
    g.z = np.load(os.path.join(GOLDEN_DIR, TASK + ".npz"))
    g.meta = json.loads(str(g.z["meta_json"]))
    g.fixture = load_fixture()
    g.robot = ROBOTS[g.fixture["robot"]]
    g.steps, g.N = g.meta["steps"], g.meta["num_envs"]
    return g


# ---- the command term's fixtures (tests/golden/inhand_command.npz / inhand_command_in.npz, tools/gen_golden_inhand.py)
COMMAND_KEYS = ("command", "time_left", "orientation_error", "position_error", "consecutive_success", "command_counter")
HOST_MAGIC = 0x31434849  # "IHC1" (tools/inhand_command_host.cpp)


class CommandGolden:
    """The real ``InHandReOrientationCommand`` over call 0 = ``reset`` on every env and calls 1.. = ``reset`` on a mask, then
    ``compute(step_dt)``; every draw recorded."""

    def __init__(self):
        self.out = np.load(os.path.join(GOLDEN_DIR, "inhand_command.npz"))
        self.inp = np.load(os.path.join(GOLDEN_DIR, "inhand_command_in.npz"))
        self.meta = json.loads(str(self.out["meta"]))
        self.N, self.calls, self.step_dt, self.cfg = self.meta["N"], self.meta["calls"], self.meta["step_dt"], self.meta["cfg"]

    def const(self, key) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(self.inp[key]))

    def inputs(self, t: int) -> dict:
        return {k: torch.from_numpy(np.ascontiguousarray(self.inp[f"call{t}/{k}"])) for k in ("object_root_pos_w", "object_root_quat_w", "uniforms", "reset_mask")}

    def expected(self, t: int) -> dict:
        return {k: torch.from_numpy(np.ascontiguousarray(self.out[f"call{t}/{k}"])) for k in COMMAND_KEYS}

    def host_file(self, path: str) -> None:
        """The input file of tools/inhand_command_host.cpp for all calls."""
        c = self.cfg
        with open(path, "wb") as f:
            f.write(np.asarray([HOST_MAGIC, self.N, self.calls, int(c["make_quat_unique"]), int(c["update_goal_on_success"]), 0, 0, 0], np.int32).tobytes())
            f.write(np.asarray([*c["resampling_time_range"], c["orientation_success_threshold"], 0.0], np.float32).tobytes())
            f.write(np.asarray([self.step_dt], np.float32).tobytes())
            f.write(self.inp["pos_command_e"].astype(np.float32).tobytes())
            f.write(self.inp["pos_command_w"].astype(np.float32).tobytes())
            for t in range(self.calls):
                d = self.inputs(t)
                f.write(np.asarray([int(t > 0)], np.int32).tobytes())
                f.write(d["object_root_pos_w"].numpy().astype(np.float32).tobytes())
                f.write(d["object_root_quat_w"].numpy().astype(np.float32).tobytes())
                f.write(d["reset_mask"].numpy().astype(np.int32).tobytes())
                f.write(d["uniforms"].numpy().astype(np.float32).tobytes())

    def read_host_output(self, path: str) -> list:
        raw, N, out, off = open(path, "rb").read(), self.N, [], 0
        for _ in range(self.calls):
            d = {}
            for k, w in (("command", 7), ("time_left", 1), ("orientation_error", 1), ("position_error", 1), ("consecutive_success", 1)):
                d[k] = torch.from_numpy(np.frombuffer(raw, np.float32, N * w, off).copy()).reshape((N, w) if w > 1 else (N,))
                off += 4 * N * w
            d["command_counter"] = torch.from_numpy(np.frombuffer(raw, np.int64, N, off).copy())
            off += 8 * N
            out.append(d)
        assert off == len(raw)
        return out


def assert_command_close(got: dict, ref: dict, tol: float, what: str) -> None:
    """Counters bit for bit; the goal quaternion within ``tol`` up to nothing (its sign is fixed by the construction); time_left and the
    metrics within ``tol`` (relative above 1); consecutive_success bit for bit (whole numbers)."""
    assert torch.equal(got["command_counter"].cpu(), ref["command_counter"]), f"{what}: command_counter"
    assert torch.equal(got["consecutive_success"].cpu(), ref["consecutive_success"]), f"{what}: consecutive_success"
    for k in ("command", "time_left", "orientation_error", "position_error"):
        a, b = got[k].cpu().double(), ref[k].double()
        err = (a - b).abs()
        assert bool((err <= tol * b.abs().clamp(min=1.0)).all()), f"{what}: {k} max err {float(err.max()):.3e}"
