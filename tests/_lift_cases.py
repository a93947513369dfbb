"""fp64 statements of the manipulation/lift/mdp terms (isaaclab_tasks .../manipulation/lift/mdp: observations.py:19-31, rewards.py:20-67,
terminations.py:25-53) and of ``root_height_below_minimum`` on the object, the feed tweak that takes each of their branches, and the
branch counts -- shared by tests/test_lift_plan.py, tests/test_lift_gpu.py and tools/gen_golden_lift.py (which applies the same tweak to the
feed the reference's managers run on).  The formulas restate the reference's utils/math.py helpers (quat_apply :546-566, quat_inv
:239-248, combine_frame_transforms :750-786, subtract_frame_transforms :785-816) in float64 on the fp32 inputs."""

from __future__ import annotations

import os

import numpy as np
import torch

from _reach_cases import quat_apply

TASK = "Isaac-Lift-Cube-Franka-v0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TASK + ".json")
ROBOT, EE_BODY, EE_OFFSET = "franka_panda", "panda_hand", (0.0, 0.0, 0.1034)
A, PA, D = 8, 9, 36
GRIPPER_COL, GRIPPER_PCOLS = 7, (7, 8)
MIN_HEIGHT, DROP_HEIGHT = 0.04, -0.05  # object_is_lifted / object_goal_distance minimal_height; object_dropping minimum_height
STD_EE, STD_GOAL, STD_GOAL_FINE = 0.1, 0.3, 0.05
LIFT = "isaaclab_tasks.manager_based.manipulation.lift.mdp"
FAR_SHIFT = (400.0, -300.0, 0.0)  # where the "far from the origin" envs are moved: fp32 rounds world coordinates there at 3e-5 m

# the gripper column's edge actions (env mod 8; the other envs keep their draw): everything not < 0 opens the gripper
GRIPPER_EDGES = (0.0, -0.0, -float(np.float32(1.0e-45)), -1.0e-30)


def f32(x: float) -> float:
    return float(np.float32(x))


def ee_pos_w(s: dict, b: int) -> torch.Tensor:
    """``ee_frame.data.target_pos_w[:, 0]`` (frame_transformer.py:358): body_pos + quat_apply(body_quat, offset.pos), fp64."""
    off = torch.tensor(EE_OFFSET, dtype=torch.float64, device=s["body_pos_w"].device).expand(s["body_pos_w"].shape[0], 3)
    return s["body_pos_w"][:, b].double() + quat_apply(s["body_quat_w"][:, b].double(), off)


def des_pos_w(s: dict) -> torch.Tensor:
    return s["root_pos_w"].double() + quat_apply(s["root_quat_w"].double(), s["command"][:, :3].double())


def lift_terms(s: dict, b: int) -> dict:
    """Every lift term's raw value in fp64 from the feed tensors ``s`` (current snapshot); thresholds are the fp32 roundings the fp32
    reference compares against."""
    d = lambda n: s[n].double()  # noqa: E731
    obj, rp, rq = d("object_root_pos_w"), d("root_pos_w"), d("root_quat_w")
    q_inv = torch.cat([rq[:, :1], -rq[:, 1:]], dim=-1) / rq.norm(dim=-1, keepdim=True).clamp(min=1.0e-9)
    lifted = obj[:, 2] > f32(MIN_HEIGHT)
    d_ee = (obj - ee_pos_w(s, b)).norm(dim=-1)
    d_goal = (des_pos_w(s) - obj).norm(dim=-1)
    return {"object_position": quat_apply(q_inv, obj - rp),
            "object_is_lifted": lifted.double(),
            "object_ee_distance": 1.0 - torch.tanh(d_ee / STD_EE),
            "object_goal_distance": lifted.double() * (1.0 - torch.tanh(d_goal / STD_GOAL)),
            "object_goal_distance_fine": lifted.double() * (1.0 - torch.tanh(d_goal / STD_GOAL_FINE)),
            "object_dropping": obj[:, 2] < f32(DROP_HEIGHT),
            "goal_distance": d_goal, "ee_distance": d_ee}


def position_rounding(s: dict, b: int) -> torch.Tensor:
    """Per-env allowance for the fp32 rounding of world positions far from the origin, as ``_reach_cases.position_rounding``: two roundings
    of the largest coordinate involved (des_pos_w = root + R cmd or ee_w = body + R offset, then the difference to the object), which
    the fp32 reference has as well.  Divide by std for a tanh kernel (|d/dx tanh| <= 1)."""
    big = torch.stack([s[n].double().abs().amax(-1) for n in ("root_pos_w", "object_root_pos_w")] + [s["body_pos_w"][:, b].double().abs().amax(-1)]).amax(0) + 1.0
    return 2.0 * big * 2.0 ** -24 * 2.0


def lift_tweak(feed, b: int, gen: torch.Generator, ee_fn=None, des_fn=None) -> None:
    """Every branch of the lift terms on a random feed, applied to every snapshot.  Env e, with p = e mod 8 and z = (e // 8) mod 8:
    * e mod 16 == 7: the whole env (root, bodies, object) moved by FAR_SHIFT, far from the origin;
    * p = 0: the object at the end-effector point (distance 0); p = 1: at STD_EE from it in a random direction;
    * p = 2: the object at the commanded world position; p = 3 / 4: at STD_GOAL_FINE / STD_GOAL from it;
    * p >= 5: the feed's object (far from both points), its height set for z < 6 to exactly f32(0.04), the next float above, the next
      below, and the same three around f32(-0.05).
    ``ee_fn(body_pos, body_quat)`` / ``des_fn(root_pos, root_quat, cmd_pos)``: the fp32 functions that place the object ON the two points
    (the generator passes the reference's own ``combine_frame_transforms``); default: the fp64 formulas rounded to fp32."""
    st, N = feed._stack, feed.num_envs
    dev = st["object_root_pos_w"].device
    idx = torch.arange(N)
    p, zc = (idx % 8).to(dev), ((idx // 8) % 8).to(dev)
    far = (idx % 16 == 7).to(dev)
    shift = torch.tensor(FAR_SHIFT, device=dev)
    off = torch.tensor(EE_OFFSET, device=dev).expand(N, 3)
    if ee_fn is None:
        ee_fn = lambda bp, bq: (bp.double() + quat_apply(bq.double(), off.double())).float()  # noqa: E731
    if des_fn is None:
        des_fn = lambda rp, rq, c: (rp.double() + quat_apply(rq.double(), c.double())).float()  # noqa: E731
    one = np.float32
    zvals = [one(MIN_HEIGHT), np.nextafter(one(MIN_HEIGHT), one(1)), np.nextafter(one(MIN_HEIGHT), one(-1)),
             one(DROP_HEIGHT), np.nextafter(one(DROP_HEIGHT), one(1)), np.nextafter(one(DROP_HEIGHT), one(-1))]
    for k in range(feed.num_snapshots):
        for n in ("root_pos_w", "object_root_pos_w"):
            st[n][k][far] += shift
        st["body_pos_w"][k][far] += shift
        obj = st["object_root_pos_w"][k]
        dirn = torch.randn(N, 3, generator=gen)
        dirn = (dirn / dirn.norm(dim=-1, keepdim=True)).to(dev)
        ee = ee_fn(st["body_pos_w"][k][:, b], st["body_quat_w"][k][:, b])
        des = des_fn(st["root_pos_w"][k], st["root_quat_w"][k], st["command"][k][:, :3])
        for case, base, dist in ((0, ee, 0.0), (1, ee, STD_EE), (2, des, 0.0), (3, des, STD_GOAL_FINE), (4, des, STD_GOAL)):
            sel = p == case
            obj[sel] = base[sel] + dirn[sel] * dist
        for case, zv in enumerate(zvals):
            sel = (p >= 5) & (zc == case)
            obj[sel, 2] = float(zv)


def gripper_edges(action: torch.Tensor) -> torch.Tensor:
    """The gripper column of ``action`` (N, 8) with the edge values on envs e mod 8 < 4 (in place; returns ``action``)."""
    m = torch.arange(action.shape[0], device=action.device) % 8
    for case, v in enumerate(GRIPPER_EDGES):
        action[m == case, GRIPPER_COL] = v
    return action


def branch_counts(snaps: list[dict], b: int, actions: list[torch.Tensor] | None = None) -> dict:
    """How often each branch occurs over the snapshots ``snaps`` (dicts of feed tensors) and the gripper actions -- what the golden's
    ``meta_json`` records and the tests require to be non-zero."""
    c = dict.fromkeys(("z_at_min_height", "z_above_min_height", "z_below_min_height", "z_at_drop_height", "z_above_drop_height",
                       "z_below_drop_height", "lifted", "not_lifted", "dropped", "at_ee", "ee_near_std", "ee_far", "at_goal",
                       "goal_near_std_fine", "goal_near_std", "goal_far", "far_from_origin"), 0)
    one = np.float32
    for s in snaps:
        z = s["object_root_pos_w"][:, 2].cpu().numpy()
        for name, ref in (("min_height", one(MIN_HEIGHT)), ("drop_height", one(DROP_HEIGHT))):
            c[f"z_at_{name}"] += int((z == ref).sum())
            c[f"z_above_{name}"] += int((z == np.nextafter(ref, one(1))).sum())
            c[f"z_below_{name}"] += int((z == np.nextafter(ref, one(-1))).sum())
        t = lift_terms({n: v.cpu() for n, v in s.items()}, b)
        c["lifted"] += int((t["object_is_lifted"] > 0).sum())
        c["not_lifted"] += int((t["object_is_lifted"] == 0).sum())
        c["dropped"] += int(t["object_dropping"].sum())
        de, dg = t["ee_distance"], t["goal_distance"]
        c["at_ee"] += int((de < 1.0e-6).sum())
        c["ee_near_std"] += int(((de - STD_EE).abs() < 1.0e-3).sum())
        c["ee_far"] += int((de > 3.0 * STD_EE).sum())
        c["at_goal"] += int((dg < 1.0e-6).sum())
        c["goal_near_std_fine"] += int(((dg - STD_GOAL_FINE).abs() < 1.0e-3).sum())
        c["goal_near_std"] += int(((dg - STD_GOAL).abs() < 1.0e-3).sum())
        c["goal_far"] += int((dg > 2.0 * STD_GOAL).sum())
        c["far_from_origin"] += int((s["root_pos_w"].abs().amax(-1) > 100.0).sum())
    if actions is not None:
        g = torch.cat([a[:, GRIPPER_COL].cpu() for a in actions]).numpy()
        bits = g.view(np.uint32)
        c.update(gripper_pos_zero=int((bits == 0).sum()), gripper_neg_zero=int((bits == 0x80000000).sum()),
                 gripper_neg_subnormal=int((bits == 0x80000001).sum()), gripper_neg_tiny=int((g == one(-1.0e-30)).sum()),
                 gripper_neg=int((g < -1.0e-3).sum()), gripper_pos=int((g > 1.0e-3).sum()), gripper_nan=int(np.isnan(g).sum()))
    return c


def load_fixture() -> dict:
    """The committed cfg dump (tests/golden/<task>.json + .managers.json), through the path form of ``load_task_cfg``."""
    from isaaclab_amd.env import load_task_cfg

    return load_task_cfg(FIXTURE)


def golden():
    """``_util.Golden`` of the lift fixture (its cfg dump lies under tests/golden, not in the package's configs)."""
    import json

    from _util import GOLDEN, Golden
    from isaaclab_amd.robots import ROBOTS

    g = Golden.__new__(Golden)
    g.task = TASK
    g.z = np.load(os.path.join(GOLDEN, TASK + ".npz"))
    g.meta = json.loads(str(g.z["meta_json"]))
    g.fixture = load_fixture()
    g.robot = ROBOTS[g.fixture["robot"]]
    g.steps, g.N = g.meta["steps"], g.meta["num_envs"]
    return g
