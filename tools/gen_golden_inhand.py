"""TEST INFRASTRUCTURE (build container only): the Isaac-Repose-Cube-Allegro-v0 fixtures, from the REAL reference.

    python tools/gen_golden_inhand.py

Writes, all under ``tests/golden/`` (data derived from the reference lives there only),
  * ``Isaac-Repose-Cube-Allegro-v0.json`` (``AllegroCubeEnvCfg()`` and ``AllegroCubePPORunnerCfg()`` through
    ``oracle.gen_golden.dump_cfg``) and ``Isaac-Repose-Cube-Allegro-NoVelObs-v0.json`` (``AllegroCubeNoVelObsEnvCfg()``: the same task
    without three observation terms), each with its ``.managers.json`` side file: reset events, robot init state and the ``object``
    RigidObject the terms read;
  * ``Isaac-Repose-Cube-Allegro-v0.npz``: ``oracle.gen_golden.run_task`` -- the real ActionManager with the real
    ``EMAJointPositionToLimitsAction``, the real termination, reward and observation managers with the manipulation/inhand/mdp terms --
    N = 64, 5 steps, on a feed tweaked so that every branch of those terms is taken (``tests/_inhand_cases.inhand_tweak``; the counts go
    to ``meta_json``), plus the plan blob the live cfg object compiles to (``live_cfg/blob``);
  * ``inhand_command.npz`` / ``inhand_command_in.npz``: the real ``InHandReOrientationCommand`` (``CommandTerm.reset`` / ``compute``) on
    a minimal stand-in env over a reset and six computes at N = 64, every random draw served from a recorded table, with a step at which
    goals are reached, orientation errors a margin away from the threshold on either side and ``make_quat_unique`` on.

Gaps of the fake scene of ``oracle/gen_golden.py`` are filled here, without editing it: an ``object`` entity whose ``data`` serves the
feed's four object tensors, and a command term object exposing ``.command``, ``.cfg`` (the real ``InHandReOrientationCommandCfg``) and
``.metrics["consecutive_success"]`` from the feed.  Deterministic: a second run reproduces the files bit for bit.
"""

from __future__ import annotations

import json
import math
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
from isaaclab_tasks.manager_based.manipulation.inhand.config.allegro_hand.agents.rsl_rl_ppo_cfg import (  # noqa: E402
    AllegroCubeNoVelObsPPORunnerCfg,
    AllegroCubePPORunnerCfg,
)
from isaaclab_tasks.manager_based.manipulation.inhand.config.allegro_hand.allegro_env_cfg import AllegroCubeEnvCfg, AllegroCubeNoVelObsEnvCfg  # noqa: E402
from isaaclab_tasks.manager_based.manipulation.inhand.mdp.commands.orientation_command import InHandReOrientationCommand  # noqa: E402

import _inhand_cases as ic  # noqa: E402
from isaaclab_amd.plan import compile_plan  # noqa: E402
from isaaclab_amd.robots import ALLEGRO_HAND  # noqa: E402
from isaaclab_amd.state_feed import OBJECT_STATE  # noqa: E402

TASK = ic.TASK


# ---- the fake scene's missing pieces
class _ObjectData:
    """RigidObjectData: the root state is the feed's."""

    def __init__(self, feed):
        self._feed = feed

    root_pos_w = property(lambda self: self._feed["object_root_pos_w"])
    root_quat_w = property(lambda self: self._feed["object_root_quat_w"])
    root_lin_vel_w = property(lambda self: self._feed["object_root_lin_vel_w"])
    root_ang_vel_w = property(lambda self: self._feed["object_root_ang_vel_w"])


_scene_init = gg.FakeScene.__init__


def _scene_with_object(self, entities, sensors, env_origins, cfg):
    _scene_init(self, entities, sensors, env_origins, cfg)
    self._e["object"] = types.SimpleNamespace(data=_ObjectData(entities["robot"].data._feed))


_COMMAND_CFG = None  # the live cfg's commands.object_pose (the real InHandReOrientationCommandCfg)


def _get_term(self, name):
    """What the in-hand terms read of the command term: .command, .cfg, .metrics (and what command_resample reads)."""
    f = self._feed
    return types.SimpleNamespace(command=f["command"], cfg=_COMMAND_CFG, metrics={"consecutive_success": f["command_consecutive_success"]},
                                 time_left=f["command_time_left"], command_counter=f["command_counter"])


_feeds = []


def feed_tweak(feed):
    ic.inhand_tweak(feed, torch.Generator().manual_seed(8181))
    _feeds.append(feed)


def dump_managers(task, env_cfg):
    """Side file: reset events, the robot init state, and the scene entity beyond the robot the terms read (settings only)."""
    base = env_cfg.to_dict()
    ev = {k: v for k, v in base["events"].items() if v is not None and v.get("mode") in ("reset", "interval")}
    sc = base["scene"]
    side = {"events": ev, "curriculum": base.get("curriculum"),
            "scene": {"robot": {"init_state": {k: list(v) for k, v in sc["robot"]["init_state"].items() if k in ("pos", "rot", "lin_vel", "ang_vel")}},
                      "object": {"class_type": sc["object"]["class_type"], "prim_path": sc["object"]["prim_path"],
                                 "init_state": {k: list(v) for k, v in sc["object"]["init_state"].items()}}}}
    with open(os.path.join(gg.GOLDEN, task + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, indent=1, sort_keys=False)


def margin_check():
    """The 1e-4 rad margin of the tweak against the reference's own fp32 ``quat_error_magnitude``: 4096 pairs placed 1e-4 .. 0.2 rad on
    either side of the threshold; returns (largest |fp32 - fp64|, comparisons that flip between the two)."""
    g = torch.Generator().manual_seed(4096)
    n = 4096
    q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g, dtype=torch.float64), dim=-1).float()
    side = torch.where(torch.arange(n) % 2 == 0, -1.0, 1.0).double()
    angle = ic.f32(ic.SUCCESS_THRESHOLD) + side * (torch.rand(n, generator=g, dtype=torch.float64) * (0.2 - 1.0e-4) + 1.0e-4)
    angle = angle.clamp(min=1.0e-4)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    goal = ic.quat_mul(ic.quat_conj(ic.quat_about(angle, axis)), q.double()).float()
    e32 = ref_math.quat_error_magnitude(q, goal)
    e64 = ref_math.quat_error_magnitude(q.double(), goal.double())
    th = ic.f32(ic.SUCCESS_THRESHOLD)
    flips = int(((e32 <= th) != (e64 <= th)).sum()) + int(((e32 < th) != (e64 < th)).sum())
    return float((e32.double() - e64).abs().max()), flips


def step_fixture():
    global _COMMAND_CFG
    steps = 5
    gg.CONFIGS = gg.GOLDEN  # dump_cfg writes the cfg fixture next to the golden
    gg.FakeScene.__init__ = _scene_with_object
    gg.FakeCommandManager.get_term = _get_term
    cfg = AllegroCubeEnvCfg()
    _COMMAND_CFG = cfg.commands.object_pose
    gg.run_task(TASK, cfg, AllegroCubePPORunnerCfg(), ALLEGRO_HAND, N=64, steps=steps, seed=909, kitchen=dict(feed_tweak=feed_tweak))
    dump_managers(TASK, AllegroCubeEnvCfg())
    gg.dump_cfg(ic.TASK_NOVEL, AllegroCubeNoVelObsEnvCfg(), AllegroCubeNoVelObsPPORunnerCfg(), ALLEGRO_HAND)
    dump_managers(ic.TASK_NOVEL, AllegroCubeNoVelObsEnvCfg())
    path = os.path.join(gg.GOLDEN, TASK + ".npz")
    z = np.load(path)
    # the per-step tensors no in-hand term reads are left out (run_task records every EXTRA tensor of a kitchen run)
    unread = ("body_lin_acc_w", "command_time_left", "command_counter", "link_incoming_joint_force", "body_pos_w", "body_quat_w")
    rec = {k: z[k] for k in z.files if k.rpartition("/")[2] not in unread or "/in/" not in k}
    feed = _feeds[0]
    for k, tag in enumerate(["reset"] + [f"step{t}" for t in range(steps)]):  # snapshot k: what run_task's feed held at that point
        for n in OBJECT_STATE:
            rec[f"{tag}/in/{n}"] = feed._stack[n][k].numpy().copy()
    meta = json.loads(str(rec["meta_json"]))
    snaps = [{n: torch.from_numpy(rec[f"step{t}/in/{n}"] if n != "env_origins" else rec["static/env_origins"]) for n in ic.NAMES} for t in range(steps)]
    e_max, flips = margin_check()
    meta.update(branches=ic.branch_counts(snaps), margin_check=dict(pairs=4096, max_fp32_fp64_difference_rad=e_max, flipped_comparisons=flips))
    assert flips == 0 and meta["branches"]["min_angle_margin"] >= ic.ANGLE_MARGIN * 0.99 and meta["branches"]["min_distance_margin"] >= ic.DIST_MARGIN
    rec["meta_json"] = np.array(json.dumps(meta))
    # the plan blob of the LIVE cfg object: tests/test_inhand_plan.py compiles the committed JSON dump and requires the very same blob
    rec["live_cfg/blob"] = np.ascontiguousarray(compile_plan(AllegroCubeEnvCfg(), ALLEGRO_HAND).blob, np.int32)
    np.savez_compressed(path, **rec)
    print(f"[golden] {TASK}: {meta['branches']}  margin check {meta['margin_check']}")


# ---------------------------------------------------------------------------------------------------- the command term's fixtures
class DrawTable:
    """``Tensor.uniform_`` of ``CommandTerm._resample`` and ``torch.rand`` of ``_resample_command`` served from U[draw, env, column]: draw =
    which resampling of the env within the running call (reset, timer, goal reached), column = {time_left, rand_floats[:, 0],
    rand_floats[:, 1]}."""

    def __init__(self, N):
        self.N, self.U, self.ids, self.active = N, None, None, False
        self.draw = torch.zeros(N, dtype=torch.long)

    def install(self):
        tab = self
        self._real = (torch.Tensor.uniform_, torch.rand, InHandReOrientationCommand._resample)
        real_resample = self._real[2]

        def fake_uniform(self, lo=0.0, hi=1.0):
            self.copy_(tab.U[tab.draw[tab.ids], tab.ids, 0] * (hi - lo) + lo)
            return self

        real_rand = self._real[1]

        def fake_rand(*size, **kw):
            if not tab.active:  # (not inside _resample: somebody else's draw)
                return real_rand(*size, **kw)
            size = size[0] if len(size) == 1 else size
            assert tuple(size) == (len(tab.ids), 2)
            return tab.U[tab.draw[tab.ids], tab.ids, 1:3].clone()

        def wrapped_resample(self, env_ids):
            env_ids = torch.arange(tab.N)[env_ids] if isinstance(env_ids, slice) else torch.as_tensor(env_ids)
            if len(env_ids) == 0:
                return
            tab.ids, tab.active = env_ids, True
            try:
                real_resample(self, env_ids)
            finally:
                tab.active = False
            tab.draw[env_ids] += 1

        torch.Tensor.uniform_ = fake_uniform
        torch.rand = fake_rand
        InHandReOrientationCommand._resample = wrapped_resample

    def remove(self):
        torch.Tensor.uniform_, torch.rand, InHandReOrientationCommand._resample = self._real


def command_fixture():
    N, computes, step_dt = 64, 6, 1.0 / 30.0
    g = torch.Generator().manual_seed(2024)
    cfg = AllegroCubeEnvCfg().commands.object_pose
    cfg.debug_vis = False
    cfg.make_quat_unique = True
    cfg.resampling_time_range = (2 * step_dt, 5 * step_dt)  # (the task's 1e6 s never runs out: the timer's resampling is exercised too)
    th = cfg.orientation_success_threshold
    env_origins = (torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([40.0, 40.0, 0.0])
    default_root_state = torch.zeros(N, 13)
    default_root_state[:, :3] = torch.tensor(AllegroCubeEnvCfg().scene.object.init_state.pos)
    default_root_state[:, 3] = 1.0
    term = InHandReOrientationCommand.__new__(InHandReOrientationCommand)
    term.cfg = cfg
    term._debug_vis_handle = None
    term._env = types.SimpleNamespace(num_envs=N, device="cpu", step_dt=step_dt, scene=types.SimpleNamespace(env_origins=env_origins))
    data = types.SimpleNamespace(default_root_state=default_root_state)
    term.object = types.SimpleNamespace(data=data)
    # InHandReOrientationCommand.__init__ (orientation_command.py:41-62) after CommandTerm.__init__ (command_manager.py:55-66)
    term.metrics = {}
    term.time_left = torch.zeros(N)
    term.command_counter = torch.zeros(N, dtype=torch.long)
    term.pos_command_e = default_root_state[:, :3] + torch.tensor(cfg.init_pos_offset, dtype=torch.float)
    term.pos_command_w = term.pos_command_e + env_origins
    term.quat_command_w = torch.zeros(N, 4)
    term.quat_command_w[:, 0] = 1.0
    term._X_UNIT_VEC = torch.tensor([1.0, 0, 0]).repeat((N, 1))
    term._Y_UNIT_VEC = torch.tensor([0, 1.0, 0]).repeat((N, 1))
    term._Z_UNIT_VEC = torch.tensor([0, 0, 1.0]).repeat((N, 1))
    for k in ("orientation_error", "position_error", "consecutive_success"):
        term.metrics[k] = torch.zeros(N)
    U_all = torch.rand(computes + 1, 3, N, 3, generator=g)
    # timers: a start value a multiple of step_dt away from zero lands on `<= 0` by rounding alone; keep every start 2 % of a step away
    lo, hi = cfg.resampling_time_range
    while True:
        f = torch.remainder((U_all[..., 0].double() * (hi - lo) + lo) / step_dt, 1.0)
        bad = (f < 0.02) | (f > 0.98)
        if not bool(bad.any()):
            break
        U_all[..., 0][bad] = torch.rand(int(bad.sum()), generator=g)
    masks = torch.stack([torch.rand(N, generator=g) < (1.0 if t == 0 else 0.15) for t in range(computes + 1)])
    out, inp = {}, {"env_origins": env_origins, "default_object_pos": default_root_state[:, :3].clone(), "pos_command_e": term.pos_command_e.clone(),
                    "pos_command_w": term.pos_command_w.clone()}
    tab = DrawTable(N)
    tab.install()
    min_margin, reached_total, timer_total = math.inf, 0, 0
    try:
        for t in range(computes + 1):
            # the object: call 0 is the env reset (no compute); later an object a chosen angle away from the goal of the moment -- a
            # third of the envs inside the threshold by a margin in [1e-4, 0.05] rad (the goal is reached), a third outside by one, the
            # rest anywhere; at the last call consecutive successes accumulate on the envs that stay inside
            tab.U, tab.draw[:] = U_all[t], 0
            ids = masks[t].nonzero().flatten()
            pos = term.pos_command_w + torch.randn(N, 3, generator=g) * 0.02
            if t == 0:
                quat = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1)
                data.root_pos_w, data.root_quat_w = pos, quat
                term.reset(ids)
            else:
                # (the reset of this call replaces the goal of the reset envs first: their object is placed against the NEW goal, which
                # the reference computes from the same recorded draws -- run the reset, then place the object, then compute)
                if len(ids):
                    term.reset(ids)
                goal = term.quat_command_w.double()
                kind = torch.arange(N) % 3
                margin = torch.rand(N, generator=g, dtype=torch.float64) * (0.05 - 1.0e-4) + 1.0e-4
                angle = torch.where(kind == 0, th - margin, torch.where(kind == 1, th + margin, torch.rand(N, generator=g, dtype=torch.float64) * math.pi))
                axis = torch.nn.functional.normalize(torch.randn(N, 3, generator=g, dtype=torch.float64), dim=-1)
                quat = ic.quat_mul(ic.quat_about(angle, axis), goal).float()
                quat[::7] = -quat[::7]  # either sign of the object's quaternion
                data.root_pos_w, data.root_quat_w = pos, quat
                err = ref_math.quat_error_magnitude(quat, term.quat_command_w)
                min_margin = min(min_margin, float((err.double() - th).abs().min()))
                reached_total += int((err < th).sum())
                before = term.command_counter.clone()
                term.compute(step_dt)
                timer_total += int(((term.command_counter - before) > (err < th).long()).sum())
            inp[f"call{t}/object_root_pos_w"], inp[f"call{t}/object_root_quat_w"] = pos, quat
            inp[f"call{t}/uniforms"], inp[f"call{t}/reset_mask"] = U_all[t], masks[t]
            out[f"call{t}/command"] = term.command.clone()
            for k in ("pos_command_w", "quat_command_w", "time_left", "command_counter"):
                out[f"call{t}/{k}"] = getattr(term, k).clone()
            for k, v in term.metrics.items():
                out[f"call{t}/{k}"] = v.clone()
    finally:
        tab.remove()
    assert list(term.metrics) == ["orientation_error", "position_error", "consecutive_success"]
    assert min_margin >= 0.9e-4 and reached_total > 50 and timer_total > 10, (min_margin, reached_total, timer_total)
    assert float(out[f"call{computes}/consecutive_success"].max()) >= 3.0
    d = cfg.to_dict()
    keep = {k: d[k] for k in ("asset_name", "init_pos_offset", "make_quat_unique", "orientation_success_threshold", "update_goal_on_success",
                              "resampling_time_range")}
    keep["class_type"] = f"{InHandReOrientationCommand.__module__}:{InHandReOrientationCommand.__name__}"
    rec = {k: v.numpy().copy() for k, v in out.items()}
    rec["meta"] = np.array(json.dumps(dict(N=N, calls=computes + 1, step_dt=step_dt, cfg=gg._jsonable(keep), metrics=list(term.metrics),
                                           min_threshold_margin_rad=min_margin, goals_reached=reached_total, timer_resamplings=timer_total)))
    np.savez_compressed(os.path.join(gg.GOLDEN, "inhand_command.npz"), **rec)
    np.savez_compressed(os.path.join(gg.GOLDEN, "inhand_command_in.npz"), **{k: v.numpy().copy() for k, v in inp.items()})
    print(f"[golden] inhand_command: {len(rec)} + {len(inp)} arrays, goals reached {reached_total}, timer resamplings {timer_total}, "
          f"min margin {min_margin:.2e} rad")


if __name__ == "__main__":
    step_fixture()
    command_fixture()
