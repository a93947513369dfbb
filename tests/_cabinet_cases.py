"""Isaac-Open-Drawer-Franka-v0: the fixture's constants, the feed tweak that takes every branch of the manipulation/cabinet/mdp terms
while keeping each compared quantity a margin away from its threshold, the branch counts and the fixture loaders -- shared by
tests/test_cabinet_plan.py, tests/test_cabinet_gpu.py and tools/gen_golden_cabinet.py (which applies the same tweak to the feed the
reference's managers run on).  The formulas themselves are tests/_cabinet_oracle.py's, evaluated here in float64 on the fp32 tensors."""

from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

import _cabinet_oracle as co

TASK = "Isaac-Open-Drawer-Franka-v0"
TASK_IK_ABS, TASK_IK_REL = "Isaac-Open-Drawer-Franka-IK-Abs-v0", "Isaac-Open-Drawer-Franka-IK-Rel-v0"
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROBOT = "franka_panda_cabinet"
CABINET = "isaaclab_tasks.manager_based.manipulation.cabinet.mdp"
MDP = "isaaclab.envs.mdp"
# The cabinet articulation (Props/Sektion_Cabinet/sektion_cabinet_instanceable.usd) as the fixtures' side files state it.  The USD is not
# available offline: the joints are the four the task cfg names, the bodies the ones its prim paths and body_names refer to plus the
# links those joints move, in an ASSUMED breadth-first order.  Nothing depends on the order beyond consistency with the state feed.
CABINET_JOINTS = ["door_left_joint", "door_right_joint", "drawer_bottom_joint", "drawer_top_joint"]
CABINET_BODIES = ["sektion", "door_left_link", "door_right_link", "drawer_bottom", "drawer_top", "door_left_nob_link", "door_right_nob_link",
                  "drawer_handle_bottom", "drawer_handle_top"]
A, PA, D = 8, 9, 31  # raw action columns (7 arm + 1 gripper), processed columns (7 + 2 finger joints), policy observation width
DIMS = {TASK: (A, PA, D), TASK_IK_ABS: (8, 9, 31), TASK_IK_REL: (7, 8, 30)}  # the IK variants: a 7- / 6-wide pose command for the arm
COLS = {"joint_pos": (0, 9), "joint_vel": (9, 18), "cabinet_joint_pos": (18, 19), "cabinet_joint_vel": (19, 20), "rel_ee_drawer_distance": (20, 23),
        "actions": (23, 31)}
REWARDS = ("approach_ee_handle", "align_ee_handle", "approach_gripper_handle", "align_grasp_around_handle", "grasp_handle", "open_drawer_bonus",
           "multi_stage_open_drawer", "action_rate_l2", "joint_vel")
WEIGHTS = {"approach_ee_handle": 2.0, "align_ee_handle": 0.5, "approach_gripper_handle": 5.0, "align_grasp_around_handle": 0.125,
           "grasp_handle": 0.5, "open_drawer_bonus": 7.5, "multi_stage_open_drawer": 1.0}
APPROACH_THRESHOLD, GRASP_THRESHOLD, OFFSET, OPEN_JOINT_POS = 0.2, 0.03, 0.04, 0.04  # the cfg's params
STAGES = (0.01, 0.2, 0.3)  # multi_stage_open_drawer's drawer positions
# How far the tweak keeps the tcp-handle distance, the fingertip-handle height gaps and the drawer position from the thresholds they are
# compared with (the margin rule of tests/_inhand_cases.py: the placed cases at least this far, an untouched env that happens to lie
# within NEAR of a threshold is moved beyond it).  The compared quantities are differences of world coordinates of a few tens of
# metres at most: fp32 rounds those at 2e-6 m, and a frame is three such operations deep.
DIST_MARGIN, GAP_MARGIN, JOINT_MARGIN, NEAR = 1.0e-4, 1.0e-4, 1.0e-4, 2.0e-3
NAMES = ("body_pos_w", "body_quat_w", "joint_pos", "env_origins", "articulation_joint_pos", "articulation_joint_vel", "articulation_body_pos_w",
         "articulation_body_quat_w")


def f32(x: float) -> float:
    return float(np.float32(x))


def fixture_path(task: str = TASK) -> str:
    return os.path.join(GOLDEN_DIR, task + ".json")


def load_fixture(task: str = TASK) -> dict:
    """The committed cfg dump (tests/golden/<task>.json + .managers.json), through the path form of ``load_task_cfg``."""
    from isaaclab_amd.env import load_task_cfg

    return load_task_cfg(fixture_path(task))


def scene_of(fx: dict | None = None):
    """``(plan, second articulation, ee sensor, cabinet sensor, drawer joint id, gripper joint ids)`` of the fixture: what the oracle's
    ``terms`` takes beside the tensors."""
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS, SceneEntityResolver

    fx = fx or load_fixture()
    robot = ROBOTS[fx["robot"]]
    plan = compile_plan(fx["env"], robot)
    res = SceneEntityResolver(robot, fx["env"]["scene"])
    second = res.second
    return (plan, second, co.frames_of(plan.frame_tables["ee_frame"]), co.frames_of(plan.frame_tables["cabinet_frame"]),
            second.joint_names.index("drawer_top_joint"), [robot.joint_names.index(j) for j in ("panda_finger_joint1", "panda_finger_joint2")])


def cabinet_terms(s: dict, scene=None) -> dict:
    """Every cabinet term in float64 on the fp32 tensors ``s``."""
    _, second, ee, cab, drawer, gripper = scene or scene_of()
    d = {n: s[n].double().cpu() for n in NAMES}
    return co.terms(d, ee, cab, drawer, gripper, APPROACH_THRESHOLD, GRASP_THRESHOLD, OFFSET, OPEN_JOINT_POS,
                    (second.default_joint_pos[drawer], second.default_joint_vel[drawer]))


def cabinet_tweak(feed, gen: torch.Generator, scene=None) -> None:
    """Every branch of the cabinet terms on a random feed, with margins, applied to every snapshot (the feed serves the second
    articulation's state from here on).  The drawer handle's body is placed so that its FRAME lands where the case wants it.  Env e, with
    p = e mod 16 and r = (e + e // 16) mod 8:
    * p = 0 / 1: the handle GRASP_THRESHOLD minus / plus a margin in [1e-3, 0.02] m from the tool centre point, in a random direction;
      p = 2 / 3: APPROACH_THRESHOLD minus / plus a margin in [2e-3, 0.05] m (a direction that brings the handle's height within
      2 GAP_MARGIN of a fingertip's is drawn again);
    * p = 5: graspable -- the two finger bodies are swapped where the right fingertip is the upper one (and the left one is lifted by
      0.01 m where the two are within NEAR), the handle's height lies between the fingertips', 10 % .. 90 % of the way; p = 6 / 7: the
      handle a margin in [2 GAP_MARGIN, 0.01] m above the upper / below the lower fingertip; both 0.05 .. 0.35 m beside the tool centre point;
    * every other env keeps the generator's placement; one whose handle lies within 2 GAP_MARGIN of a fingertip's height is lifted by NEAR,
      then one whose distance lies within NEAR of a threshold is moved horizontally by 0.007 m until it does not;
    * the drawer joint: r = 0 .. 5: STAGES[r // 2] minus / plus a margin in [JOINT_MARGIN, 5e-3] m; otherwise the generator's draw, moved
      up by NEAR where it lies within 2 JOINT_MARGIN of a stage."""
    scene = scene or scene_of()
    plan, second, ee, cab, drawer, _ = scene
    feed.ensure_articulation_state(second, plan.frame_tables)
    st, N = feed._stack, feed.num_envs
    dev = st["body_pos_w"].device
    idx = torch.arange(N)
    p, r = idx % 16, (idx + idx // 16) % 8
    hb, hoff = cab[1][0][0], torch.tensor(cab[1][0][1], dtype=torch.float64)
    lb, rb = ee[1][1][0], ee[1][2][0]
    u = lambda lo, hi: torch.rand(N, generator=gen, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    unit = lambda: torch.nn.functional.normalize(torch.randn(N, 3, generator=gen, dtype=torch.float64), dim=-1)  # noqa: E731
    for k in range(feed.num_snapshots):
        bp, bq = st["body_pos_w"][k].cpu(), st["body_quat_w"][k].cpu()
        ap, aq, jp = st["articulation_body_pos_w"][k].cpu(), st["articulation_body_quat_w"][k].cpu(), st["articulation_joint_pos"][k].cpu()

        def tips():
            return co.frame_transformer(ee, bp.double(), bq.double())["target_pos_w"]

        def handle():
            return co.frame_pose(cab[1][0], ap.double(), aq.double())[0]

        def place(want, sel):  # the handle body that puts the handle frame at `want` (fp64) for the envs of `sel`
            body = want - co.quat_apply(aq[:, hb].double(), hoff.expand(N, 3))
            ap[sel, hb] = body[sel].float()

        # -- the fingers of the graspable envs
        t = tips()
        swap = (p == 5) & (t[:, 1, 2] <= t[:, 2, 2])
        for x in (bp, bq):
            left, right = x[:, lb].clone(), x[:, rb].clone()
            x[swap, lb], x[swap, rb] = right[swap], left[swap]
        t = tips()
        close = (p == 5) & ((t[:, 1, 2] - t[:, 2, 2]) < NEAR)
        bp[close, lb, 2] += 0.01
        t = tips()
        tcp, lz, rz = t[:, 0], t[:, 1, 2], t[:, 2, 2]
        # -- the distance cases
        dist = torch.where(p == 0, f32(GRASP_THRESHOLD) - u(1.0e-3, 0.02), torch.where(p == 1, f32(GRASP_THRESHOLD) + u(1.0e-3, 0.02),
                           torch.where(p == 2, f32(APPROACH_THRESHOLD) - u(2.0e-3, 0.05), f32(APPROACH_THRESHOLD) + u(2.0e-3, 0.05))))
        sel = p < 4
        want = tcp + unit() * dist.unsqueeze(-1)
        for _ in range(64):
            bad = sel & (((want[:, 2] - lz).abs() < 2.0 * GAP_MARGIN) | ((want[:, 2] - rz).abs() < 2.0 * GAP_MARGIN))
            if not bool(bad.any()):
                break
            want = torch.where(bad.unsqueeze(-1), tcp + unit() * dist.unsqueeze(-1), want)
        place(want, sel)
        # -- the height cases
        ang, rad = u(0.0, 2.0 * math.pi), u(0.05, 0.35)
        hi, lo = torch.maximum(lz, rz), torch.minimum(lz, rz)
        z = torch.where(p == 5, rz + u(0.1, 0.9) * (lz - rz), torch.where(p == 6, hi + u(2.0 * GAP_MARGIN, 0.01), lo - u(2.0 * GAP_MARGIN, 0.01)))
        sel = (p >= 5) & (p <= 7)
        place(torch.stack([tcp[:, 0] + rad * torch.cos(ang), tcp[:, 1] + rad * torch.sin(ang), z], dim=-1), sel)
        # -- the untouched envs: off the fingertips' heights, then every env but the distance cases off the distance thresholds
        free = (p == 4) | (p > 7)
        for _ in range(8):
            h = handle()
            bad = free & (((h[:, 2] - lz).abs() < 2.0 * GAP_MARGIN) | ((h[:, 2] - rz).abs() < 2.0 * GAP_MARGIN))
            if not bool(bad.any()):
                break
            ap[bad, hb, 2] += NEAR
        for _ in range(64):
            d = (handle() - tcp).norm(dim=-1)
            bad = (p > 3) & (((d - f32(GRASP_THRESHOLD)).abs() < NEAR) | ((d - f32(APPROACH_THRESHOLD)).abs() < NEAR))
            if not bool(bad.any()):
                break
            ap[bad, hb, 0] += 0.007
        # -- the drawer joint
        m = u(JOINT_MARGIN, 5.0e-3)
        q = jp[:, drawer].double()
        for case in range(6):
            q = torch.where(r == case, f32(STAGES[case // 2]) + (m if case % 2 else -m), q)
        for s_ in STAGES:
            q = torch.where((r > 5) & ((q - f32(s_)).abs() < 2.0 * JOINT_MARGIN), q + NEAR, q)
        jp[:, drawer] = q.float()
        for name, x in (("body_pos_w", bp), ("body_quat_w", bq), ("articulation_body_pos_w", ap), ("articulation_joint_pos", jp)):
            st[name][k].copy_(x.to(dev))


def branch_counts(snaps: list, scene=None) -> dict:
    """How often each branch occurs over the snapshots ``snaps`` (dicts of feed tensors), and how far every env stays from each
    threshold (float64, on the fp32 tensors) -- what the golden's ``meta_json`` records and the tests require."""
    scene = scene or scene_of()
    c = dict.fromkeys(("graspable", "not_graspable", "within_approach_threshold", "beyond_approach_threshold", "within_grasp_threshold",
                       "beyond_grasp_threshold", "drawer_below_0.01", "drawer_above_0.01", "drawer_below_0.2", "drawer_above_0.2", "drawer_below_0.3",
                       "drawer_above_0.3", "align_z_positive", "align_z_negative", "align_x_positive", "align_x_negative",
                       "graspable_and_drawer_above_0.2", "graspable_and_drawer_above_0.3"), 0)
    m_dist = m_gap = m_joint = math.inf
    for s in snaps:
        t = cabinet_terms(s, scene)
        g, d, q = t["is_graspable"], t["distance"], t["drawer"]
        c["graspable"] += int(g.sum())
        c["not_graspable"] += int((~g).sum())
        c["within_approach_threshold"] += int((d <= f32(APPROACH_THRESHOLD)).sum())
        c["beyond_approach_threshold"] += int((d > f32(APPROACH_THRESHOLD)).sum())
        c["within_grasp_threshold"] += int((d <= f32(GRASP_THRESHOLD)).sum())
        c["beyond_grasp_threshold"] += int((d > f32(GRASP_THRESHOLD)).sum())
        for s_ in STAGES:
            c[f"drawer_below_{s_}"] += int((q <= f32(s_)).sum())
            c[f"drawer_above_{s_}"] += int((q > f32(s_)).sum())
            m_joint = min(m_joint, float((q - f32(s_)).abs().min()))
        c["graspable_and_drawer_above_0.2"] += int((g & (q > f32(0.2))).sum())
        c["graspable_and_drawer_above_0.3"] += int((g & (q > f32(0.3))).sum())
        for a in ("align_z", "align_x"):
            c[f"{a}_positive"] += int((t[a] > 0).sum())
            c[f"{a}_negative"] += int((t[a] < 0).sum())
        m_dist = min(m_dist, float((d - f32(APPROACH_THRESHOLD)).abs().min()), float((d - f32(GRASP_THRESHOLD)).abs().min()))
        m_gap = min(m_gap, float(t["finger_gaps"].abs().min()))
    c["min_distance_margin"], c["min_gap_margin"], c["min_joint_margin"] = m_dist, m_gap, m_joint
    return c


def margins_hold(c: dict) -> bool:
    return c["min_distance_margin"] >= DIST_MARGIN and c["min_gap_margin"] >= GAP_MARGIN and c["min_joint_margin"] >= 0.99 * JOINT_MARGIN


def golden(task: str = TASK):
    """``_util.Golden`` of a cabinet step fixture (its cfg dump lies under tests/golden; its snapshots also carry the second
    articulation's state)."""
    from _util import Golden
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import ARTICULATION_STATE, DYNAMIC, EXTRA, STATIC, StateFeed

    class _Golden(Golden):
        def snapshots(self):
            out = []
            for tag in ["reset"] + [f"step{k}" for k in range(self.steps)]:
                d = {n: self.t(f"{tag}/in/{n}") for n in DYNAMIC + EXTRA + ARTICULATION_STATE + ("jacobians",) if f"{tag}/in/{n}" in self.z}
                d.update({n: self.t(f"static/{n}") for n in STATIC})
                out.append(d)
            return out

        def feed(self, device="cpu"):
            return StateFeed.from_tensors(self.robot, self.snapshots(), device=device, gravity_dir=self.meta["gravity_dir"])

    g = _Golden.__new__(_Golden)
    g.task = task
    g.z = np.load(os.path.join(GOLDEN_DIR, task + ".npz"))
    g.meta = json.loads(str(g.z["meta_json"]))
    g.fixture = load_fixture(task)
    g.robot = ROBOTS[g.fixture["robot"]]
    g.steps, g.N = g.meta["steps"], g.meta["num_envs"]
    return g


# ---- the FrameTransformer fixture (tests/golden/frame_transformer.npz, tools/gen_golden_cabinet.py)
FT_OUTPUTS = ("source_pos_w", "source_quat_w", "target_pos_w", "target_quat_w", "target_pos_source", "target_quat_source")
FT_CASES = ("ee_frame", "cabinet_frame", "ee_frame_source_offset")
HOST_MAGIC = 0x31544649  # "IFT1" (tools/frame_transformer_host.cpp)


class FrameGolden:
    """The reference's combine_frame_transforms / subtract_frame_transforms in the order of frame_transformer.py:337-384 on recorded body
    poses: per case the frames (body ids, offsets), the body poses and the six outputs."""

    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN_DIR, "frame_transformer.npz"))
        self.meta = json.loads(str(self.z["meta_json"]))

    def sensor(self, case: str):
        ids, pos, rot = (self.z[f"{case}/frames/{k}"] for k in ("body_ids", "pos", "rot"))
        frames = [(int(b), tuple(float(x) for x in p), tuple(float(x) for x in q)) for b, p, q in zip(ids, pos, rot)]
        return frames[0], frames[1:]

    def bodies(self, case: str):
        return tuple(torch.from_numpy(np.ascontiguousarray(self.z[f"{case}/{k}"])) for k in ("body_pos_w", "body_quat_w"))

    def expected(self, case: str) -> dict:
        return {k: torch.from_numpy(np.ascontiguousarray(self.z[f"{case}/{k}"])) for k in FT_OUTPUTS}

    def frame_words(self, case: str) -> np.ndarray:
        """(1 + T, 9) int32: the frames as ``imx_frame_transformer`` and the host program take them."""
        src, tg = self.sensor(case)
        w = np.zeros((1 + len(tg), 9), np.int32)
        for row, (b, pos, rot) in zip(w, [src] + tg):
            row[0] = b
            row[2:] = np.asarray([*pos, *rot], np.float32).view(np.int32)
        return w

    def host_file(self, path: str, case: str) -> None:
        """The input file of tools/frame_transformer_host.cpp: magic, N, T, B, the frame words, the body positions, the body quaternions."""
        bp, bq = self.bodies(case)
        w = self.frame_words(case)
        with open(path, "wb") as f:
            f.write(np.asarray([HOST_MAGIC, bp.shape[0], w.shape[0] - 1, bp.shape[1]], np.int32).tobytes())
            f.write(w.tobytes())
            f.write(bp.numpy().astype(np.float32).tobytes())
            f.write(bq.numpy().astype(np.float32).tobytes())

    def read_host_output(self, path: str, case: str) -> dict:
        bp, _ = self.bodies(case)
        N, T = bp.shape[0], self.frame_words(case).shape[0] - 1
        raw, off, out = open(path, "rb").read(), 0, {}
        for k, shape in zip(FT_OUTPUTS, ((N, 3), (N, 4), (N, T, 3), (N, T, 4), (N, T, 3), (N, T, 4))):
            n = int(np.prod(shape))
            out[k] = torch.from_numpy(np.frombuffer(raw, np.float32, n, off).copy()).reshape(shape)
            off += 4 * n
        assert off == len(raw)
        return out
