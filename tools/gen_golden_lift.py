"""TEST INFRASTRUCTURE (build container only): the Isaac-Lift-Cube-Franka-v0 fixtures, from the REAL reference.

    python tools/gen_golden_lift.py

Writes, all under ``tests/golden/`` (data derived from the reference lives there only),
  * ``Isaac-Lift-Cube-Franka-v0.json`` (``FrankaCubeLiftEnvCfg()`` and ``LiftCubePPORunnerCfg()`` through ``oracle.gen_golden.dump_cfg``)
    and its ``.managers.json`` side file: reset events, curriculum, robot init state, and the two scene entities the lift terms read --
    the ``object`` RigidObject and the ``ee_frame`` FrameTransformer (class, prim paths, target frames, offsets);
  * ``Isaac-Lift-Cube-Franka-v0.npz``: ``oracle.gen_golden.run_task`` -- the real ActionManager with the real ``BinaryJointPositionAction``,
    the real termination, reward and observation managers with the manipulation/lift/mdp terms -- N = 64, 5 steps, on a feed tweaked so
    that every branch of those terms is taken (``tests/_lift_cases.lift_tweak``; the counts go to ``meta_json``), plus the plan blob the
    live cfg object compiles to (``live_cfg/blob``).

Gaps of the fake scene of ``oracle/gen_golden.py`` are filled here, without editing it: ``ArticulationData.root_state_w`` /
``body_state_w``; an ``object`` entity whose ``data.root_pos_w`` serves the feed's ``object_root_pos_w``; an ``ee_frame`` entity whose
``data.target_pos_w`` is the reference's own ``combine_frame_transforms`` on the feed's hand pose (frame_transformer.py:358).  The
gripper column of every step's action is overwritten with the edge values (+0.0, -0.0, the smallest negative subnormal, -1e-30) on
half of the envs before the real ``ActionManager.process_action`` sees it.  Deterministic: a second run reproduces the files bit for bit.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)

import isaaclab.utils.math as ref_math  # noqa: E402
from isaaclab.managers import ActionManager  # noqa: E402
from isaaclab_tasks.manager_based.manipulation.lift.config.franka.agents.rsl_rl_ppo_cfg import LiftCubePPORunnerCfg  # noqa: E402
from isaaclab_tasks.manager_based.manipulation.lift.config.franka.joint_pos_env_cfg import FrankaCubeLiftEnvCfg  # noqa: E402

import _lift_cases as lc  # noqa: E402
from isaaclab_amd.plan import compile_plan  # noqa: E402
from isaaclab_amd.robots import FRANKA_PANDA  # noqa: E402

TASK = lc.TASK
HAND = FRANKA_PANDA.body_names.index(lc.EE_BODY)


# ---- the fake scene's missing pieces
def _root_state_w(self):
    f = self._feed
    return torch.cat([f["root_pos_w"], f["root_quat_w"], f["root_lin_vel_w"], f["root_ang_vel_w"]], dim=-1)


def _body_state_w(self):
    f = self._feed
    p, q = f["body_pos_w"], f["body_quat_w"]
    return torch.cat([p, q, torch.zeros(*p.shape[:2], 6)], dim=-1)


gg.FakeArticulationData.root_state_w = property(_root_state_w)
gg.FakeArticulationData.body_state_w = property(_body_state_w)


class _ObjectData:
    """RigidObjectData: the root position is the feed's."""

    def __init__(self, feed):
        self._feed = feed

    @property
    def root_pos_w(self):
        return self._feed["object_root_pos_w"]


class _FrameData:
    """FrameTransformerData.target_pos_w (N, 1, 3) of the cfg's one target frame, on the feed's hand pose (frame_transformer.py:358)."""

    def __init__(self, feed, frame_cfg):
        self._feed = feed
        t = frame_cfg.target_frames[0]
        assert t.prim_path.endswith("/" + lc.EE_BODY), t.prim_path
        self._pos = torch.tensor(t.offset.pos, dtype=torch.float32)
        self._rot = torch.tensor(t.offset.rot, dtype=torch.float32)

    @property
    def target_pos_w(self):
        f, N = self._feed, self._feed.num_envs
        pos, _ = ref_math.combine_frame_transforms(f["body_pos_w"][:, HAND], f["body_quat_w"][:, HAND], self._pos.expand(N, 3), self._rot.expand(N, 4))
        return pos.unsqueeze(1)


_scene_init = gg.FakeScene.__init__


def _scene_with_object(self, entities, sensors, env_origins, cfg):
    _scene_init(self, entities, sensors, env_origins, cfg)
    feed = entities["robot"].data._feed
    self._e["object"] = types.SimpleNamespace(data=_ObjectData(feed))
    self._e["ee_frame"] = types.SimpleNamespace(data=_FrameData(feed, cfg.ee_frame))


gg.FakeScene.__init__ = _scene_with_object

# ---- the gripper edge actions: run_task draws every action itself; the real manager gets them with the gripper column overwritten, and
#      the recorded step{t}/action is replaced by what it got
_process_action = ActionManager.process_action
_seen_actions: list[torch.Tensor] = []


def _process_with_edges(self, action):
    lc.gripper_edges(action)
    _seen_actions.append(action.clone())
    return _process_action(self, action)


ActionManager.process_action = _process_with_edges


def feed_tweak(feed):
    def ee_fn(bp, bq):
        N = bp.shape[0]
        return ref_math.combine_frame_transforms(bp, bq, torch.tensor(lc.EE_OFFSET).expand(N, 3), torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(N, 4))[0]

    lc.lift_tweak(feed, HAND, torch.Generator().manual_seed(6161), ee_fn=ee_fn,
                  des_fn=lambda rp, rq, c: ref_math.combine_frame_transforms(rp, rq, c)[0])


def dump_managers(env_cfg):
    """Side file: reset events, the curriculum (host-side), the robot init state, and the scene entities beyond the robot the terms read
    (settings only: class, prim paths, init state, target frames and their offsets)."""
    base = env_cfg.to_dict()
    ev = {k: v for k, v in base["events"].items() if v is not None and v.get("mode") in ("reset", "interval")}
    sc = base["scene"]
    frame = sc["ee_frame"]
    side = {"events": ev, "curriculum": base.get("curriculum"),
            "scene": {"robot": {"init_state": {k: list(v) for k, v in sc["robot"]["init_state"].items() if k in ("pos", "rot", "lin_vel", "ang_vel")}},
                      "object": {"class_type": sc["object"]["class_type"], "prim_path": sc["object"]["prim_path"],
                                 "init_state": {k: list(v) for k, v in sc["object"]["init_state"].items()}},
                      "ee_frame": {"class_type": frame["class_type"], "prim_path": frame["prim_path"],
                                   "source_frame_offset": frame["source_frame_offset"],
                                   "target_frames": [{k: t[k] for k in ("prim_path", "name", "offset")} for t in frame["target_frames"]]}}}
    with open(os.path.join(gg.GOLDEN, TASK + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, indent=1, sort_keys=False)


def main():
    steps = 5
    gg.CONFIGS = gg.GOLDEN  # dump_cfg writes the cfg fixture next to the golden
    gg.run_task(TASK, FrankaCubeLiftEnvCfg(), LiftCubePPORunnerCfg(), FRANKA_PANDA, N=64, steps=steps, seed=577, kitchen=dict(feed_tweak=feed_tweak))
    dump_managers(FrankaCubeLiftEnvCfg())
    path = os.path.join(gg.GOLDEN, TASK + ".npz")
    z = np.load(path)
    # the per-step tensors no lift term reads are left out (run_task records every EXTRA tensor of a kitchen run)
    unread = ("body_lin_acc_w", "command_time_left", "command_counter", "link_incoming_joint_force")
    rec = {k: z[k] for k in z.files if k.rpartition("/")[2] not in unread or "/in/" not in k}
    assert len(_seen_actions) == steps
    for t, a in enumerate(_seen_actions):
        rec[f"step{t}/action"] = a.numpy().copy()
    meta = json.loads(str(rec["meta_json"]))
    names = ("root_pos_w", "root_quat_w", "command", "body_pos_w", "body_quat_w", "object_root_pos_w")
    snaps = [{n: torch.from_numpy(rec[f"step{t}/in/{n}"]) for n in names} for t in range(steps)]
    meta.update(ee_body=lc.EE_BODY, ee_body_id=HAND, ee_offset=list(lc.EE_OFFSET), processed_action_dim=int(rec["step0/processed_actions"].shape[1]),
                branches=lc.branch_counts(snaps, HAND, _seen_actions))
    rec["meta_json"] = np.array(json.dumps(meta))
    # the plan blob of the LIVE cfg object: tests/test_lift_plan.py compiles the committed JSON dump and requires the very same blob
    rec["live_cfg/blob"] = np.ascontiguousarray(compile_plan(FrankaCubeLiftEnvCfg(), FRANKA_PANDA).blob, np.int32)
    np.savez_compressed(path, **rec)
    print(f"[golden] {TASK}: {meta['branches']}")


if __name__ == "__main__":
    main()
