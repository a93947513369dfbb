"""TEST INFRASTRUCTURE (build container only): the fixtures of the Open-Drawer task's ``_reset_idx``, from the REAL reference.

    python tools/gen_golden_cabinet_orchestration.py

Writes, under ``tests/golden/``, ``<name>.npz`` (recorded results), ``<name>_in.npz`` (inputs, actions, draws) and ``<name>.json`` (the cfg
in the fixture-wrapper form) for
  * ``cabinet_orchestration``: the real ``FrankaCabinetEnvCfg`` with its shipped events -- ``reset_scene_to_default`` (``reset_all``), which
    walks BOTH articulations of the scene, and ``reset_joints_by_offset`` on the robot;
  * ``cabinet_events_orchestration``: the same cfg plus two reset events on the cabinet, ``reset_joints_by_offset``
    (``reset_cabinet_joints``) and ``reset_root_state_uniform`` (``reset_cabinet_root``).  The cabinet's limit tables, which PhysX provides
    in a live binding, are this tool's own (LIMITS below) and sit in the scene entry of the JSON; both changes are recorded in the meta.

Each run drives the real ``ManagerBasedRLEnv._reset_idx`` and ``EventManager`` over the recording asset of
``oracle/gen_golden_orchestration.py`` for the robot and a recording articulation for the cabinet, following the recipe of
``tools/gen_golden_manip_orchestration.py``: N = 64, ``reset()`` + 40 steps, observation corruption off.  The two startup
``randomize_rigid_body_material`` terms stay in the JSON; the run itself leaves them out (class terms that read PhysX views when built).
The resets are time-outs, scheduled through ``episode_length_buf`` before the first step; nothing the events write depends on the
per-step state, so the inputs hold the static tensors, the draws, the actions and that buffer only.

Ranges are chosen so that the kernel's fp32 ``hi - lo`` equals the reference's (symmetric ranges), and the cabinet's root event moves and
pushes but does not rotate: every recorded quantity is then reproducible bit for bit.  Deterministic: a second run reproduces the files.
"""

from __future__ import annotations

import functools
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
from oracle.gen_golden_orchestration import RecordingAsset  # noqa: E402
from tools import gen_golden_cabinet as gc  # noqa: E402  (the fake scene's cabinet and frame entities)

import isaaclab.envs.mdp as mdp  # noqa: E402
import isaaclab.envs.mdp.events as ref_events  # noqa: E402
import isaaclab.utils.string as ref_string  # noqa: E402
from isaaclab.envs import ManagerBasedRLEnv  # noqa: E402
from isaaclab.managers import CommandManager, CurriculumManager, EventManager, SceneEntityCfg  # noqa: E402
from isaaclab.managers import EventTermCfg as EventTerm  # noqa: E402

import _cabinet_cases as cc  # noqa: E402
from isaaclab_amd.plan import compile_plan  # noqa: E402
from isaaclab_amd.robots import FRANKA_PANDA_CABINET as ROBOT  # noqa: E402
from isaaclab_amd.robots import SceneEntityResolver  # noqa: E402
from isaaclab_amd.state_feed import STATIC, StateFeed  # noqa: E402

N, STEPS = 64, 40
STARTUP = ("robot_physics_material", "cabinet_physics_material")
# the cabinet's joint limits (joint order of tests/_cabinet_cases.CABINET_JOINTS): this tool's own, the USD is not available offline
LIMITS = {"joint_pos_limits": [[-1.57, 0.0], [0.0, 1.57], [-0.1, 0.4], [-0.15, 0.25]], "joint_vel_limits": [1.0, 1.0, 0.3, 0.2],
          "soft_joint_pos_limit_factor": 0.9}
CABINET_EVENTS = {
    "reset_cabinet_joints": dict(func="reset_joints_by_offset", params={"position_range": (-0.2, 0.2), "velocity_range": (-0.5, 0.5)}),
    "reset_cabinet_root": dict(func="reset_root_state_uniform", params={
        "pose_range": {"x": (-0.1, 0.1), "y": (-0.05, 0.05), "z": (0.0, 0.02)},
        "velocity_range": {"x": (-0.1, 0.1), "z": (-0.05, 0.05), "yaw": (-0.2, 0.2)}}),
}


def _root_state(init, n):
    s = torch.zeros(n, 13)
    s[:, 0:3] = torch.tensor(init.pos, dtype=torch.float32)
    s[:, 3:7] = torch.tensor(init.rot, dtype=torch.float32)
    s[:, 7:10] = torch.tensor(init.lin_vel, dtype=torch.float32)
    s[:, 10:13] = torch.tensor(init.ang_vel, dtype=torch.float32)
    return s


class RecordingArticulation:
    """The scene's second articulation: name tables, defaults and limits in ``data``; ``write_*_to_sim`` land in persistent buffers."""

    def __init__(self, name, n, default_root_state, limits):
        J = len(cc.CABINET_JOINTS)
        self.device, self.num_instances = "cpu", n
        self.joint_names, self.body_names = list(cc.CABINET_JOINTS), list(cc.CABINET_BODIES)
        self.num_joints, self.num_bodies = J, len(self.body_names)
        self.sim_writes = {f"{name}_root_pose": torch.zeros(n, 7), f"{name}_root_vel": torch.zeros(n, 6), f"{name}_joint_pos": torch.zeros(n, J),
                           f"{name}_joint_vel": torch.zeros(n, J)}
        self._name, self.calls = name, []
        self.data = types.SimpleNamespace(default_root_state=default_root_state, default_joint_pos=torch.zeros(n, J), default_joint_vel=torch.zeros(n, J))
        if limits is not None:  # Articulation._process_cfg: the soft limits (articulation.py), fp32
            lim = torch.tensor(limits["joint_pos_limits"], dtype=torch.float32)
            mean, rng = (lim[..., 0] + lim[..., 1]) / 2, lim[..., 1] - lim[..., 0]
            f = limits["soft_joint_pos_limit_factor"]
            self.data.soft_joint_pos_limits = torch.stack([mean - 0.5 * rng * f, mean + 0.5 * rng * f], dim=-1).repeat(n, 1, 1)
            self.data.soft_joint_vel_limits = torch.tensor(limits["joint_vel_limits"], dtype=torch.float32).repeat(n, 1)

    def find_joints(self, name_keys, joint_subset=None, preserve_order=False):
        return ref_string.resolve_matching_names(name_keys, self.joint_names, preserve_order)

    def find_bodies(self, name_keys, preserve_order=False):
        return ref_string.resolve_matching_names(name_keys, self.body_names, preserve_order)

    def _put(self, key, value, env_ids):
        self.sim_writes[f"{self._name}_{key}"][slice(None) if env_ids is None else env_ids] = value

    def write_root_pose_to_sim(self, pose, env_ids=None):
        self._put("root_pose", pose, env_ids)
        self.calls.append(f"{self._name}_root_pose")

    def write_root_velocity_to_sim(self, vel, env_ids=None):
        self._put("root_vel", vel, env_ids)
        self.calls.append(f"{self._name}_root_vel")

    def write_joint_state_to_sim(self, pos, vel, env_ids=None):
        self._put("joint_pos", pos, env_ids)
        self._put("joint_vel", vel, env_ids)
        self.calls.append(f"{self._name}_joints")


def _schedule(gen, max_len):
    """The step index at which each env times out (>= STEPS: never); env 0 never, env 1 at the first and env 2 at the last step."""
    pick = torch.randint(0, STEPS + 12, (N,), generator=gen)  # (the 12 extra values: no reset inside the run)
    at = torch.where(pick < STEPS, pick, torch.full_like(pick, STEPS + 5))
    at[0], at[1], at[2] = STEPS + 5, 0, STEPS - 1
    return at, (max_len - 1 - at)


def run(task, cfg, agent_cfg, seed, cabinet_events: bool):
    torch.manual_seed(seed)
    J, J2 = ROBOT.num_joints, len(cc.CABINET_JOINTS)
    gen = torch.Generator().manual_seed(seed + 1)
    feed = StateFeed(ROBOT, N, "cpu", seed=seed, num_snapshots=STEPS + 1)
    full = cfg.to_dict()  # the JSON keeps the shipped events, the two startup terms included
    for k in STARTUP:
        assert getattr(cfg.events, k).mode == "startup"
        setattr(cfg.events, k, None)
    if cabinet_events:
        for k, t in CABINET_EVENTS.items():
            setattr(cfg.events, k, EventTerm(func=getattr(mdp, t["func"]), mode="reset", params=dict(t["params"], asset_cfg=SceneEntityCfg("cabinet"))))
    scene_d = full["scene"]
    second = SceneEntityResolver(ROBOT, {"cabinet": dict(scene_d["cabinet"], joint_names=cc.CABINET_JOINTS, body_names=cc.CABINET_BODIES)}).second
    feed.ensure_articulation_state(second, compile_plan(gc.live_cfg_dict(cfg), ROBOT).frame_tables)
    drs = _root_state(cfg.scene.robot.init_state, N)
    events = {k: v for k, v in cfg.events.to_dict().items() if v is not None and v.get("mode") == "reset"}
    widths = {"reset_scene_to_default": 0, "reset_root_state_uniform": 12}
    T1 = STEPS + 1

    def width(name, term):
        fn = term["func"].rsplit(":", 1)[-1]
        if fn.startswith("reset_joints"):
            return 2 * (J2 if (term["params"].get("asset_cfg") or {}).get("name") == "cabinet" else J)
        return widths[fn]

    U = {k: torch.rand(T1, N, max(width(k, v), 1), generator=gen) for k, v in events.items()}
    ctx = {"name": None, "ids": None, "col": 0, "slot": 0}

    def wrap(name, fn):
        @functools.wraps(fn)
        def term(env, env_ids, *a, **k):
            ctx.update(name=name, ids=torch.arange(N) if env_ids is None else torch.as_tensor(env_ids), col=0)
            try:
                return fn(env, env_ids, *a, **k)
            finally:
                ctx["name"] = None
        return term

    for k in events:
        getattr(cfg.events, k).func = wrap(k, getattr(cfg.events, k).func)

    def fake_sample_uniform(lower, upper, size, device):
        size = (size,) if isinstance(size, int) else tuple(size)
        w = int(np.prod(size[1:])) if len(size) > 1 else 1
        u = U[ctx["name"]][ctx["slot"]][ctx["ids"], ctx["col"]:ctx["col"] + w].reshape(size)
        ctx["col"] += w
        return u * (upper - lower) + lower

    real_sample_uniform = ref_events.math_utils.sample_uniform
    ref_events.math_utils.sample_uniform = fake_sample_uniform
    scene_init = gg.FakeScene.__init__
    gg.FakeScene.__init__ = gc._scene_with_cabinet
    rec, rec_in = {}, {}

    def put(name, t):
        is_in = name.endswith("/action") or name.startswith(("static/", "draws/")) or name == "reset/episode_length_buf"
        (rec_in if is_in else rec)[name] = t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.asarray(t)

    try:
        env = gg.build_ref_env(cfg, ROBOT, feed)
        asset = RecordingAsset(ROBOT, feed, drs)
        cab = RecordingArticulation("cabinet", N, _root_state(cfg.scene.cabinet.init_state, N), LIMITS if cabinet_events else None)
        cab.data.__dict__.update({k: v for k, v in vars(env.scene["cabinet"].data).items() if not k.startswith("default_")})  # (the feed's tensors)
        env.scene._e["robot"], env.scene._e["cabinet"] = asset, cab
        env.scene.articulations = {"robot": asset, "cabinet": cab}  # the cfg's order: reset_scene_to_default walks it
        env.scene.rigid_objects, env.scene.deformable_objects = {}, {}
        env.scene.reset = lambda env_ids=None: None
        env.extras = {}
        env._sim_step_counter = 0
        env.recorder_manager = types.SimpleNamespace(reset=lambda env_ids=None: {}, active_terms=[])
        env.command_manager = CommandManager(cfg.commands, env)
        env.event_manager = EventManager(cfg.events, env)
        env.curriculum_manager = CurriculumManager(cfg.curriculum, env)
        env.action_manager = gg.ActionManager(cfg.actions, env)  # (built on the recording asset)
        A = env.action_manager.total_action_dim
        em = env.event_manager
        meta = dict(task=task, robot=ROBOT.name, num_envs=N, steps=STEPS, seed=seed, action_dim=int(A), step_dt=env.step_dt,
                    max_episode_length=env.max_episode_length, gravity_dir=feed.gravity_dir, event_terms=em.active_terms,
                    skipped_startup_terms=list(STARTUP), second_articulation="cabinet",
                    cabinet=dict(joint_names=cc.CABINET_JOINTS, body_names=cc.CABINET_BODIES),
                    changes=dict(num_envs=N, enable_corruption=False,
                                 added_events={k: dict(func=t["func"], params=t["params"], asset="cabinet") for k, t in CABINET_EVENTS.items()} if cabinet_events else {},
                                 cabinet_limit_tables=LIMITS if cabinet_events else None))
        for n_ in STATIC:
            put("static/" + n_, feed[n_])
        put("static/default_root_state", drs)
        put("static/cabinet_default_root_state", cab.data.default_root_state)
        put("static/cabinet_default_joint_pos", cab.data.default_joint_pos)
        put("static/cabinet_default_joint_vel", cab.data.default_joint_vel)
        if cabinet_events:
            put("static/cabinet_soft_joint_pos_limits", cab.data.soft_joint_pos_limits)
            put("static/cabinet_soft_joint_vel_limits", cab.data.soft_joint_vel_limits)
        for k in events:
            put("draws/" + k, U[k])

        def snapshot(tag):
            for k_, v in list(asset.sim_writes.items())[:4] + list(cab.sim_writes.items()):
                put(f"{tag}/sim_writes/{k_}", v)
            put(f"{tag}/reset_last_triggered_step", torch.stack(em._reset_term_last_triggered_step_id))
            put(f"{tag}/reset_triggered_once", torch.stack(em._reset_term_last_triggered_once))
            put(f"{tag}/common_step_counter", torch.tensor(env.common_step_counter))
            rec[f"{tag}/calls_json"] = np.array(json.dumps(asset.calls + cab.calls))
            asset.calls.clear()
            cab.calls.clear()

        # ---- ManagerBasedEnv.reset (manager_based_env.py:264-315): _reset_idx on every env
        ctx["slot"] = 0
        ManagerBasedRLEnv._reset_idx(env, torch.arange(N))
        snapshot("reset")
        at, ep = _schedule(gen, env.max_episode_length)
        env.episode_length_buf[:] = ep
        put("reset/episode_length_buf", env.episode_length_buf)
        n_resets, reset_count, subset = 0, torch.zeros(N, dtype=torch.long), False
        for t in range(STEPS):
            tag = f"step{t}"
            ctx["slot"] = 1 + t
            action = torch.randn(N, A, generator=gen).clamp(-3, 3)
            put(f"{tag}/action", action)
            # ManagerBasedRLEnv.step (manager_based_rl_env.py:153-242)
            env.action_manager.process_action(action)
            feed.advance()
            env._sim_step_counter += cfg.decimation
            env.episode_length_buf += 1
            env.common_step_counter += 1
            reset_buf = env.termination_manager.compute()
            put(f"{tag}/terminated", env.termination_manager.terminated)
            put(f"{tag}/time_outs", env.termination_manager.time_outs)
            reset_env_ids = reset_buf.nonzero(as_tuple=False).squeeze(-1)
            put(f"{tag}/reset_env_ids", reset_env_ids)
            if len(reset_env_ids) > 0:
                n_resets += len(reset_env_ids)
                reset_count[reset_env_ids] += 1
                subset |= len(reset_env_ids) < N
                ManagerBasedRLEnv._reset_idx(env, reset_env_ids)
            put(f"{tag}/episode_length_buf", env.episode_length_buf)
            snapshot(tag)
        assert subset and n_resets > 20 and int(reset_count[0]) == 0 and int(reset_count[1]) == 1
        assert cab.sim_writes["cabinet_root_pose"][:, :3].abs().sum() > 0
        meta.update(n_resets=n_resets, max_resets_per_env=int(reset_count.max()))
        print(f"[golden] {task}: {n_resets} resets over {STEPS} steps; terms {em.active_terms}")
    finally:
        ref_events.math_utils.sample_uniform = real_sample_uniform
        gg.FakeScene.__init__ = scene_init
    rec["meta_json"] = np.array(json.dumps(gg._jsonable(meta)))

    d = full
    if cabinet_events:
        for k, t in CABINET_EVENTS.items():
            fn = getattr(mdp, t["func"])
            d["events"][k] = dict(d["events"]["reset_robot_joints"], func=f"{fn.__module__}:{fn.__name__}",
                                  params=dict(t["params"], asset_cfg=dict(d["events"]["robot_physics_material"]["params"]["asset_cfg"], name="cabinet",
                                                                          body_names=None, body_ids="slice(None,None,None)")))
    keep = {k: d[k] for k in ("decimation", "episode_length_s", "is_finite_horizon", "observations", "actions", "rewards", "terminations",
                              "commands", "events", "curriculum", "seed") if k in d}
    keep["observations"]["policy"]["enable_corruption"] = False
    keep["sim"] = {"dt": d["sim"]["dt"], "gravity": d["sim"].get("gravity", (0.0, 0.0, -9.81))}
    init = lambda e: {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, (list, tuple)) else v) for k, v in e["init_state"].items()  # noqa: E731
                      if k in ("pos", "rot", "lin_vel", "ang_vel", "joint_pos", "joint_vel")}
    cabinet = {"class_type": scene_d["cabinet"]["class_type"], "prim_path": scene_d["cabinet"]["prim_path"], "init_state": init(scene_d["cabinet"]),
               "joint_names": list(cc.CABINET_JOINTS), "body_names": list(cc.CABINET_BODIES)}
    if cabinet_events:
        cabinet.update(LIMITS)
    rinit = {k: v for k, v in init(scene_d["robot"]).items() if k in ("pos", "rot", "lin_vel", "ang_vel")}
    keep["scene"] = {"num_envs": N, "env_spacing": scene_d["env_spacing"], "robot": {"init_state": rinit}, "cabinet": cabinet,
                     "ee_frame": gc._frame_entry(scene_d["ee_frame"]), "cabinet_frame": gc._frame_entry(scene_d["cabinet_frame"])}
    out = {"task": task, "robot": ROBOT.name, "env": keep, "agent": agent_cfg.to_dict()}
    with open(os.path.join(gg.GOLDEN, task + ".json"), "w") as f:
        json.dump(gg._jsonable(out), f, indent=1, sort_keys=False)
    np.savez_compressed(os.path.join(gg.GOLDEN, task + ".npz"), **rec)
    np.savez_compressed(os.path.join(gg.GOLDEN, task + "_in.npz"), **rec_in)
    print(f"[golden] {task}:", len(rec), "+", len(rec_in), "arrays")


def main():
    from isaaclab_tasks.manager_based.manipulation.cabinet.config.franka.agents.rsl_rl_ppo_cfg import CabinetPPORunnerCfg
    from isaaclab_tasks.manager_based.manipulation.cabinet.config.franka.joint_pos_env_cfg import FrankaCabinetEnvCfg

    for task, seed, more in (("cabinet_orchestration", 911, False), ("cabinet_events_orchestration", 923, True)):
        cfg = FrankaCabinetEnvCfg()
        cfg.scene.num_envs = N
        cfg.observations.policy.enable_corruption = False
        run(task, cfg, CabinetPPORunnerCfg(), seed, more)


if __name__ == "__main__":
    main()
