"""TEST INFRASTRUCTURE (build container only): the fixtures of the env's own pose-2d command terms, from the REAL reference.

    python tools/gen_golden_pose2d_command.py [classes | orchestration]

Writes
  * ``tests/golden/pose2d_command.npz`` (recorded results) + ``tests/golden/pose2d_command_in.npz`` (inputs and draws): the real
    ``UniformPose2dCommand`` / ``TerrainBasedPose2dCommand`` alone (``CommandTerm.reset`` / ``compute``), objects created with ``__new__``
    and their buffers set by hand: N = 300, 12 steps, random root poses (every other env tilted at random, the rest within 0.3 rad of
    upright), non-zero ``env_origins``, the robot within a few metres of its origin (of a patch of its terrain cell for ``T1``), random reset masks, recorded (2, N, 4) draws, ``resampling_time_range`` = (2, 5) x step_dt.
    Variants: ``U0`` the Navigation task's own cfg (``simple_heading=False``), ``U1`` ``simple_heading=True``, ``T1``
    ``TerrainBasedPose2dCommand`` with ``simple_heading=True``, a made-up ``valid_targets`` (3, 4, 5, 3), random levels / types and
    recorded (2, N) patch ids.
  * ``tests/golden/navigation_orchestration.npz`` (recorded results), ``navigation_orchestration_in.npz`` (inputs, actions, draws) +
    ``navigation_orchestration.json``: the real ``ManagerBasedRLEnv._reset_idx``, ``CommandManager`` + ``UniformPose2dCommand`` and
    ``EventManager`` (``reset_base`` = ``reset_root_state_uniform``) of ``NavigationEnvCfg`` over the recording asset of
    ``oracle/gen_golden_orchestration.py``, following the recipe of ``tools/gen_golden_pose_command.py``: ``debug_vis`` off,
    observation corruption off, ``resampling_time_range`` = (0.4, 1.2) (2-6 steps at step_dt = 0.2), N = 64, 40 steps,
    ``episode_length_buf`` seeded near the limit.  The pre-trained low-level policy is not part of it (the action term is
    replaced by one that stores the raw action: no reward, observation or termination of the task reads the joint targets).

Discrete decisions must not hang on an ulp of ``atan2f``: on the reference's own values every ``simple_heading`` choice is at least
ANGLE_MARGIN away from its tie, every ``wrap_to_pi`` argument at least ANGLE_MARGIN away from an odd multiple of pi, and every
``time_left`` at a compute at least step_dt / 100 away from 0.  The seed is incremented until the angle margins hold for EVERY element;
the timer's margin is built into its column of the draw table (``timer_draws``) and asserted like the others; the margins met are
printed and stored in the meta.  Deterministic: a second run reproduces the files bit for bit.
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

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)

import isaaclab.utils.math as ref_math  # noqa: E402
from isaaclab.envs.mdp.commands.commands_cfg import TerrainBasedPose2dCommandCfg  # noqa: E402
from isaaclab.envs.mdp.commands.pose_2d_command import TerrainBasedPose2dCommand, UniformPose2dCommand  # noqa: E402

ANGLE_MARGIN = 1.0e-4  # rad
VARIANTS = ("U0", "U1", "T1")


class Margins:
    """The smallest distances met from the points where one ulp of an angle would flip a decision."""

    def __init__(self):
        self.tie = self.wrap = self.timer = math.inf

    def wrap_arg(self, a: torch.Tensor):
        if a.numel():  # distance of the argument from the nearest odd multiple of pi
            a = a.double()
            self.wrap = min(self.wrap, float(((a - math.pi) - 2 * math.pi * torch.round((a - math.pi) / (2 * math.pi))).abs().min()))

    def ok(self, step_dt: float) -> bool:
        return self.tie >= ANGLE_MARGIN and self.wrap >= ANGLE_MARGIN and self.timer >= step_dt / 100.0

    def meta(self) -> dict:
        return {k: (None if math.isinf(v) else v) for k, v in (("min_tie_margin", self.tie), ("min_wrap_margin", self.wrap),
                                                               ("min_time_left_margin", self.timer))}


class DrawTable:
    """``Tensor.uniform_`` of ``CommandTerm._resample`` / ``_resample_command`` served from U[draw, env, column] and ``torch.randint`` of
    ``TerrainBasedPose2dCommand._resample_command`` from ids[draw, env]: draw = which resampling of the env within the running call
    (reset, timer), column = {time_left, pos_x, pos_y, heading} (the order of the uniform_ calls of ``UniformPose2dCommand``; with
    ``simple_heading`` the heading column is not drawn)."""

    def __init__(self, N: int, margins: Margins | None = None):
        self.N, self.U, self.patch_ids, self.ids, self.col = N, None, None, None, 0
        self.draw = torch.zeros(N, dtype=torch.long)
        self.margins = margins

    def install(self):
        tab = self
        self._real = (torch.Tensor.uniform_, UniformPose2dCommand._resample, torch.randint, UniformPose2dCommand._resample_command,
                      TerrainBasedPose2dCommand._resample_command)
        _, real_resample, _, real_u, real_t = self._real

        def fake_uniform(self, lo=0.0, hi=1.0):
            ids, col = tab.ids, tab.col
            tab.col += 1
            self.copy_(tab.U[tab.draw[ids], ids, col] * (hi - lo) + lo)
            return self

        real_randint = self._real[2]

        def fake_randint(low, high, size, *a, **kw):
            if tab.patch_ids is None:  # (not the terrain-based class: somebody else's randint)
                return real_randint(low, high, size, *a, **kw)
            assert low == 0 and tuple(size) == (len(tab.ids),)
            ids = tab.patch_ids[tab.draw[tab.ids], tab.ids]
            assert int(ids.max()) < high
            return ids.clone()

        def wrapped_resample(self, env_ids):
            env_ids = torch.arange(tab.N)[env_ids] if isinstance(env_ids, slice) else torch.as_tensor(env_ids)
            if len(env_ids) == 0:
                return
            tab.ids, tab.col = env_ids, 0
            real_resample(self, env_ids)
            tab.draw[env_ids] += 1

        def checked(real):
            def resample_command(self, env_ids):
                real(self, env_ids)
                if self.cfg.simple_heading and tab.margins is not None:  # the decisions of pose_2d_command.py:96-112 on the reference's own values
                    ids = torch.as_tensor(env_ids)
                    tv = self.pos_command_w[ids] - self.robot.data.root_pos_w[ids]
                    td = torch.atan2(tv[:, 1], tv[:, 0])
                    h = self.robot.data.heading_w[ids]
                    flipped = ref_math.wrap_to_pi(td + torch.pi)
                    tab.margins.tie = min(tab.margins.tie, float((ref_math.wrap_to_pi(td - h).abs().double() - math.pi / 2).abs().min()))
                    for a in (td + torch.pi, td - h, flipped - h):
                        tab.margins.wrap_arg(a)
            return resample_command

        torch.Tensor.uniform_ = fake_uniform
        torch.randint = fake_randint
        UniformPose2dCommand._resample = wrapped_resample
        UniformPose2dCommand._resample_command = checked(real_u)
        TerrainBasedPose2dCommand._resample_command = checked(real_t)

    def remove(self):
        (torch.Tensor.uniform_, UniformPose2dCommand._resample, torch.randint, UniformPose2dCommand._resample_command,
         TerrainBasedPose2dCommand._resample_command) = self._real


def heading_w(quat: torch.Tensor) -> torch.Tensor:
    """ArticulationData.heading_w (articulation_data.py:518-526)"""
    fwd = ref_math.quat_apply(quat, torch.tensor([1.0, 0.0, 0.0]).repeat(quat.shape[0], 1))
    return torch.atan2(fwd[:, 1], fwd[:, 0])


def random_root_quat(N: int, g: torch.Generator) -> torch.Tensor:
    """Every other env fully random (tilted: yaw_quat matters), the rest a random yaw with roll / pitch within 0.3 rad."""
    q = torch.randn(N, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    rp = (torch.rand(N, 2, generator=g) - 0.5) * 0.6
    yaw = (torch.rand(N, generator=g) - 0.5) * 2 * math.pi
    q[1::2] = ref_math.quat_from_euler_xyz(rp[:, 0], rp[:, 1], yaw)[1::2]
    return q.contiguous()


def _term_cfg(variant: str, step_dt: float):
    from isaaclab_tasks.manager_based.navigation.config.anymal_c.navigation_env_cfg import NavigationEnvCfg

    cfg = NavigationEnvCfg().commands.pose_command
    assert cfg.class_type is UniformPose2dCommand and cfg.simple_heading is False
    if variant == "T1":
        cfg = TerrainBasedPose2dCommandCfg(asset_name=cfg.asset_name, resampling_time_range=cfg.resampling_time_range,
                                           ranges=TerrainBasedPose2dCommandCfg.Ranges(heading=cfg.ranges.heading))
    cfg.simple_heading = variant != "U0"
    cfg.debug_vis = False
    cfg.resampling_time_range = (2 * step_dt, 5 * step_dt)
    return cfg


def timer_draws(U0: torch.Tensor, lo: float, hi: float, dt: float, g: torch.Generator) -> torch.Tensor:
    """Column 0 of the draw table (the timer's).  A timer started at u (hi - lo) + lo passes 0 at distance dt * frac((u (hi - lo) + lo) /
    dt) from it, whichever step that happens at, so a seed search alone cannot keep some 3600 timer values all dt / 100 away from 0 (about
    one in 200 lands inside).  The elements whose start value is within dt / 50 of a multiple of dt are drawn again, one by one, until
    none is; every (env, step) stays in the fixture, and the margin is then asserted on the reference's own time_left."""
    U0 = U0.clone()
    while True:
        f = torch.remainder((U0.double() * (hi - lo) + lo) / dt, 1.0)
        bad = (f < 0.02) | (f > 0.98)
        if not bool(bad.any()):
            return U0
        U0[bad] = torch.rand(int(bad.sum()), generator=g)


def class_golden(rec, rec_in, variant: str, seed: int) -> bool:
    """One try with ``seed``; False when a margin is missed (nothing is recorded then)."""
    N, steps, step_dt = 300, 12, 0.2
    L, T, P = 3, 4, 5
    cfg = _term_cfg(variant, step_dt)
    g = torch.Generator().manual_seed(seed)
    U_all = torch.rand(steps, 2, N, 4, generator=g)
    masks = torch.stack([torch.rand(N, generator=g) < (1.0 if t == 0 else 0.1) for t in range(steps)])
    U_all[..., 0] = timer_draws(U_all[..., 0], *cfg.resampling_time_range, step_dt, g)
    cls = TerrainBasedPose2dCommand if variant == "T1" else UniformPose2dCommand
    term = cls.__new__(cls)
    term.cfg = cfg
    term._debug_vis_handle = None
    env_origins = (torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([40.0, 40.0, 2.0])
    default_root_state = torch.zeros(N, 13)
    default_root_state[:, 2] = 0.6
    default_root_state[:, 3] = 1.0
    term._env = types.SimpleNamespace(num_envs=N, device="cpu", step_dt=step_dt, scene=types.SimpleNamespace(env_origins=env_origins))
    data = types.SimpleNamespace(default_root_state=default_root_state)
    term.robot = types.SimpleNamespace(data=data)
    term.pos_command_w = torch.zeros(N, 3)
    term.heading_command_w = torch.zeros(N)
    term.pos_command_b = torch.zeros(N, 3)
    term.heading_command_b = torch.zeros(N)
    term.metrics = {"error_pos": torch.zeros(N), "error_heading": torch.zeros(N)}
    term.time_left = torch.zeros(N)
    term.command_counter = torch.zeros(N, dtype=torch.long)
    out, inp = {}, {}
    if variant == "T1":
        # the patches of a cell lie within 3 m of its centre, the cells 8 m apart (the robot stands near a patch of its own cell, below)
        centre = torch.stack(torch.meshgrid(torch.arange(L) * 8.0 - 8.0, torch.arange(T) * 8.0 - 12.0, indexing="ij"), dim=-1)
        term.valid_targets = (torch.rand(L, T, P, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 1.0])
        term.valid_targets[..., :2] += centre[:, :, None, :]
        term.terrain = types.SimpleNamespace(terrain_levels=torch.randint(0, L, (N,), generator=g), terrain_types=torch.randint(0, T, (N,), generator=g))
        patch_ids = torch.randint(0, P, (steps, 2, N), generator=g)
        near_patch = torch.randint(0, P, (steps, N), generator=g)  # the patch each env stands near at step t
        inp.update(valid_targets=term.valid_targets, terrain_levels=term.terrain.terrain_levels, terrain_types=term.terrain.terrain_types)
    inp.update(env_origins=env_origins, default_root_z=default_root_state[:, 2])
    m = Margins()
    tab = DrawTable(N, m)
    tab.install()
    keys_seen = []
    try:
        for t in range(steps):
            q = random_root_quat(N, g)
            base = env_origins
            if variant == "T1":
                base = term.valid_targets[term.terrain.terrain_levels, term.terrain.terrain_types, near_patch[t]]
            root_pos = base + torch.randn(N, 3, generator=g) * torch.tensor([2.0, 2.0, 0.2]) + torch.tensor([0.0, 0.0, 0.6])
            data.root_pos_w, data.root_quat_w, data.heading_w = root_pos, q, heading_w(q)
            tab.U = U_all[t]
            tab.patch_ids = patch_ids[t] if variant == "T1" else None
            tab.draw[:] = 0
            ids = masks[t].nonzero().flatten()
            if len(ids):
                term.reset(ids)
            keys_seen.append(list(term.metrics))
            m.wrap_arg(term.heading_command_w - data.heading_w)  # _update_metrics
            m.timer = min(m.timer, float((term.time_left - step_dt).abs().min()))
            term.compute(step_dt)
            m.wrap_arg(term.heading_command_w - data.heading_w)  # _update_command (after a timer resampling)
            inp[f"step{t}/root_pos_w"], inp[f"step{t}/root_quat_w"] = root_pos, q
            inp[f"step{t}/uniforms"], inp[f"step{t}/reset_mask"] = U_all[t], masks[t]
            if variant == "T1":
                inp[f"step{t}/patch_ids"] = patch_ids[t]
            for k in ("pos_command_w", "heading_command_w", "time_left", "command_counter"):
                out[f"step{t}/{k}"] = getattr(term, k).clone()
            out[f"step{t}/command"] = term.command
            for k, v in term.metrics.items():
                out[f"step{t}/{k}"] = v.clone()
            if not m.ok(step_dt):
                return False
    finally:
        tab.remove()
    assert keys_seen[0] == ["error_pos", "error_heading"] and list(term.metrics) == ["error_pos", "error_heading", "error_pos_2d"]
    assert float(term.metrics["error_pos"].abs().max()) == 0.0  # the reference's quirk: never written
    for k, v in out.items():
        rec[f"{variant}/{k}"] = v.numpy().copy()
    for k, v in inp.items():
        rec_in[f"{variant}/{k}"] = v.numpy().copy()
    d = cfg.to_dict()
    keep = {k: d[k] for k in ("asset_name", "simple_heading", "resampling_time_range", "ranges")}
    keep["class_type"] = f"{cls.__module__}:{cls.__name__}"
    rec[f"{variant}/meta"] = np.array(json.dumps(dict(N=N, steps=steps, step_dt=step_dt, seed=seed, kind=int(variant == "T1"), cfg=gg._jsonable(keep),
                                                      metrics_before_first_compute=keys_seen[0], metrics=list(term.metrics), **m.meta())))
    resampled = sum(int((out[f"step{t}/command_counter"] > 1).sum()) for t in range(steps))
    print(f"[golden] pose2d_command {variant}: seed {seed}, {resampled} (env, step) pairs past their first timer resampling, margins {m.meta()}")
    assert resampled > 100
    return True


def classes():
    rec, rec_in = {}, {}
    for variant, seed in zip(VARIANTS, (3001, 5001, 7001)):
        while not class_golden(rec, rec_in, variant, seed):
            seed += 1
    np.savez_compressed(os.path.join(gg.GOLDEN, "pose2d_command.npz"), **rec)
    np.savez_compressed(os.path.join(gg.GOLDEN, "pose2d_command_in.npz"), **rec_in)
    print("[golden] pose2d_command:", len(rec), "+", len(rec_in), "arrays")


# ---------------------------------------------------------------------------------------------------- the orchestration fixture
TASK = "navigation_orchestration"
ON, OSTEPS = 64, 40
ARCHIVE = "navigation_low_level_policy.pt"  # (written by tools/gen_golden_navigation.py; only read here)


def make_navigation_cfg():
    import copy

    from isaaclab_tasks.manager_based.navigation.config.anymal_c.navigation_env_cfg import NavigationEnvCfg

    cfg = NavigationEnvCfg()
    cfg.scene.num_envs = ON
    a = cfg.actions.pre_trained_policy_action
    a.policy_path = os.path.join(gg.GOLDEN, ARCHIVE)
    a.debug_vis = False
    a.low_level_observations = copy.deepcopy(a.low_level_observations)
    a.low_level_observations.enable_corruption = False
    cfg.observations.policy.enable_corruption = False
    cfg.commands.pose_command.debug_vis = False
    cfg.commands.pose_command.resampling_time_range = (0.4, 1.2)
    assert cfg.curriculum is None and cfg.commands.pose_command.simple_heading is False
    assert cfg.events.reset_base.func.__name__ == "reset_root_state_uniform"
    return cfg


def navigation_orchestration_golden(seed: int) -> bool:
    """One try with ``seed``; False when an angle margin is missed (nothing is written then)."""
    import functools

    import isaaclab.envs.mdp.events as ref_events
    from isaaclab.envs import ManagerBasedRLEnv
    from isaaclab.managers import CommandManager, CurriculumManager, EventManager
    from isaaclab_tasks.manager_based.navigation.config.anymal_c.agents.rsl_rl_ppo_cfg import NavigationEnvPPORunnerCfg
    from oracle.gen_golden_orchestration import RecordingAsset

    from isaaclab_amd.robots import ANYMAL_C_NAV
    from isaaclab_amd.state_feed import STATIC, StateFeed

    torch.manual_seed(seed)
    cfg = make_navigation_cfg()
    robot = ANYMAL_C_NAV
    N = ON
    gen = torch.Generator().manual_seed(seed + 1)
    feed = StateFeed(robot, N, "cpu", seed=seed, num_snapshots=OSTEPS + 1)
    init = cfg.scene.robot.init_state
    drs = torch.zeros(N, 13)
    drs[:, 0:3] = torch.tensor(init.pos)
    drs[:, 3:7] = torch.tensor(init.rot)
    drs[:, 7:10] = torch.tensor(init.lin_vel)
    drs[:, 10:13] = torch.tensor(init.ang_vel)
    T1 = OSTEPS + 1
    U = {"reset_base": torch.rand(T1, N, 12, generator=gen)}
    U_cmd = torch.rand(T1, 2, N, 4, generator=gen)
    step_dt = cfg.sim.dt * cfg.decimation
    U_cmd[..., 0] = timer_draws(U_cmd[..., 0], *cfg.commands.pose_command.resampling_time_range, step_dt, gen)
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

    cfg.events.reset_base.func = wrap("reset_base", cfg.events.reset_base.func)

    def fake_sample_uniform(lower, upper, size, device):
        size = (size,) if isinstance(size, int) else tuple(size)
        width = int(np.prod(size[1:])) if len(size) > 1 else 1
        u = U[ctx["name"]][ctx["slot"]][ctx["ids"], ctx["col"]:ctx["col"] + width].reshape(size)
        ctx["col"] += width
        return u * (upper - lower) + lower

    real_sample_uniform = ref_events.math_utils.sample_uniform
    ref_events.math_utils.sample_uniform = fake_sample_uniform
    m = Margins()
    tab = DrawTable(N, m)
    tab.install()
    rec: dict[str, np.ndarray] = {}
    rec_in: dict[str, np.ndarray] = {}

    def put(name, t):  # inputs, actions and draws go to the _in file, recorded results to the other
        is_in = "/in/" in name or name.endswith("/action") or name.startswith(("static/", "draws/"))
        (rec_in if is_in else rec)[name] = t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.asarray(t)

    try:
        env = gg.build_ref_env(cfg, robot, feed)
        asset = RecordingAsset(robot, feed, drs)
        env.scene._e["robot"] = asset
        env.scene.articulations = {"robot": asset}
        env.scene.reset = lambda env_ids=None: None
        env.extras = {}
        env._sim_step_counter = 0
        env.recorder_manager = types.SimpleNamespace(reset=lambda env_ids=None: {}, active_terms=[])
        tab.U = U_cmd[0]
        env.command_manager = CommandManager(cfg.commands, env)
        env.event_manager = EventManager(cfg.events, env)
        env.curriculum_manager = CurriculumManager(cfg.curriculum, env)
        # the managers built by build_ref_env hold the fake command manager of the other fixtures: rebuild those that read commands
        env.reward_manager = gg.RewardManager(cfg.rewards, env)
        env.observation_manager = gg.ObservationManager(cfg.observations, env)
        term = env.command_manager.get_term("pose_command")
        assert type(term) is UniformPose2dCommand and term.robot is asset
        A = env.action_manager.total_action_dim
        meta = dict(task=TASK, robot=robot.name, num_envs=N, steps=OSTEPS, seed=seed, action_dim=int(A),
                    obs_dim=int(env.observation_manager.group_obs_dim["policy"][0]), step_dt=env.step_dt,
                    max_episode_length=env.max_episode_length, max_episode_length_s=env.max_episode_length_s, gravity_dir=feed.gravity_dir,
                    reward_terms=env.reward_manager.active_terms, termination_terms=env.termination_manager.active_terms,
                    event_terms=env.event_manager.active_terms, command_term="pose_command")
        assert abs(env.step_dt - step_dt) < 1e-12
        used = ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w", "joint_pos", "joint_vel", "net_forces_w_history")
        for n_ in STATIC:
            put("static/" + n_, feed[n_])
        put("static/default_root_state", drs)
        put("draws/reset_base", U["reset_base"])
        put("draws/command", U_cmd)
        max_target = 0.0

        def snapshot(tag):
            for n_ in used:
                put(f"{tag}/in/{n_}", feed[n_])
            for k_, v in asset.sim_writes.items():
                if k_ in ("root_pose", "root_vel"):
                    put(f"{tag}/sim_writes/{k_}", v)
            put(f"{tag}/command", term.command)
            put(f"{tag}/pos_command_w", term.pos_command_w)
            put(f"{tag}/heading_command_w", term.heading_command_w)
            put(f"{tag}/command_time_left", term.time_left)
            put(f"{tag}/command_counter", term.command_counter)
            for k_, v in term.metrics.items():
                put(f"{tag}/metric_{k_}", v)
            em = env.event_manager
            put(f"{tag}/reset_last_triggered_step", torch.stack(em._reset_term_last_triggered_step_id))
            put(f"{tag}/reset_triggered_once", torch.stack(em._reset_term_last_triggered_once))
            rec[f"{tag}/log_json"] = np.array(json.dumps({k: float(v) for k, v in env.extras.get("log", {}).items()}))
            rec[f"{tag}/calls_json"] = np.array(json.dumps(asset.calls))
            asset.calls.clear()

        # ---- ManagerBasedEnv.reset (manager_based_env.py:264-315): _reset_idx on every env, then the observations
        ctx["slot"] = 0
        tab.U = U_cmd[0]
        tab.draw[:] = 0
        ManagerBasedRLEnv._reset_idx(env, torch.arange(N))
        put("reset/obs", env.observation_manager.compute()["policy"])
        snapshot("reset")
        assert sorted(env.extras["log"]) == sorted(["Metrics/pose_command/error_pos", "Metrics/pose_command/error_heading"]
                                                   + [k for k in env.extras["log"] if not k.startswith("Metrics/")])
        # every env starts within OSTEPS steps of the time-out, so each one resets once inside the run; every seventh at the first step and
        # the next ones at the second, so that both the log without error_pos_2d (step 0) and the first one with it (step 1) are recorded
        ep = env.max_episode_length - 1 - torch.randint(0, OSTEPS, (N,), generator=gen)
        ep[::7] = env.max_episode_length - 1
        ep[1::7] = env.max_episode_length - 2
        env.episode_length_buf[:] = ep
        put("reset/episode_length_buf", env.episode_length_buf)

        n_resets = n_timer = 0
        for t in range(OSTEPS):
            tag = f"step{t}"
            ctx["slot"] = 1 + t
            tab.U = U_cmd[1 + t]
            tab.draw[:] = 0
            action = torch.randn(N, A, generator=gen).clamp(-3, 3)
            put(f"{tag}/action", action)
            # ManagerBasedRLEnv.step (manager_based_rl_env.py:153-242)
            env.action_manager.process_action(action)
            for _ in range(cfg.decimation):
                env.action_manager.apply_action()
            feed.advance()
            env._sim_step_counter += cfg.decimation
            env.episode_length_buf += 1
            env.common_step_counter += 1
            reset_buf = env.termination_manager.compute()
            reward = env.reward_manager.compute(dt=env.step_dt)
            put(f"{tag}/reward", reward)
            put(f"{tag}/terminated", env.termination_manager.terminated)
            put(f"{tag}/time_outs", env.termination_manager.time_outs)
            reset_env_ids = reset_buf.nonzero(as_tuple=False).squeeze(-1)
            put(f"{tag}/reset_env_ids", reset_env_ids)
            if len(reset_env_ids) > 0:
                n_resets += len(reset_env_ids)
                ManagerBasedRLEnv._reset_idx(env, reset_env_ids)
            if t < 2:
                assert len(reset_env_ids) > 0 and ("Metrics/pose_command/error_pos_2d" in env.extras["log"]) == (t == 1)
            n_timer += int(((term.time_left - env.step_dt) <= 0.0).sum())
            heading = asset.data.heading_w
            m.wrap_arg(term.heading_command_w - heading)  # _update_metrics
            m.timer = min(m.timer, float((term.time_left - env.step_dt).abs().min()))
            env.command_manager.compute(dt=env.step_dt)
            m.wrap_arg(term.heading_command_w - heading)  # _update_command
            max_target = max(max_target, float(term.pos_command_b.norm(dim=-1).max()))
            if not m.ok(env.step_dt):
                return False
            put(f"{tag}/obs", env.observation_manager.compute()["policy"])
            put(f"{tag}/episode_length_buf", env.episode_length_buf)
            snapshot(tag)
        meta.update(n_resets=n_resets, n_timer_resamplings=n_timer, max_target_distance=max_target, metrics=list(term.metrics), **m.meta())
        print(f"[golden] navigation orchestration: seed {seed}, {n_resets} resets, {n_timer} timer resamplings over {OSTEPS} steps, "
              f"targets within {max_target:.1f} m, margins {m.meta()}; log keys {sorted(env.extras['log'])}")
        assert 60 <= n_resets <= 200 and n_timer > 100 and list(term.metrics) == ["error_pos", "error_heading", "error_pos_2d"]
    finally:
        tab.remove()
        ref_events.math_utils.sample_uniform = real_sample_uniform
    rec["meta_json"] = np.array(json.dumps(gg._jsonable(meta)))

    d = cfg.to_dict()
    keep = {k: d[k] for k in ("decimation", "episode_length_s", "is_finite_horizon", "observations", "actions", "rewards", "terminations",
                              "commands", "events", "curriculum", "seed") if k in d}
    keep["sim"] = {"dt": d["sim"]["dt"], "gravity": d["sim"].get("gravity", (0.0, 0.0, -9.81))}
    scene = d["scene"]
    keep["scene"] = {"num_envs": scene["num_envs"], "env_spacing": scene["env_spacing"],
                     "robot": {"init_state": {k: list(v) if isinstance(v, (list, tuple)) else v for k, v in scene["robot"]["init_state"].items()
                                              if k in ("pos", "rot", "lin_vel", "ang_vel")}}}
    if "contact_forces" in scene:
        keep["scene"]["contact_forces"] = scene["contact_forces"]
    out = gg._jsonable({"task": TASK, "robot": robot.name, "env": keep, "agent": NavigationEnvPPORunnerCfg().to_dict()})
    out["env"]["actions"]["pre_trained_policy_action"]["policy_path"] = ARCHIVE  # relative to this file (load_task_cfg)
    with open(os.path.join(gg.GOLDEN, TASK + ".json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=False)
    np.savez_compressed(os.path.join(gg.GOLDEN, TASK + ".npz"), **rec)
    np.savez_compressed(os.path.join(gg.GOLDEN, TASK + "_in.npz"), **rec_in)
    print("[golden] navigation orchestration:", len(rec), "+", len(rec_in), "arrays")
    return True


def orchestration():
    seed = 811
    while not navigation_orchestration_golden(seed):
        seed += 1


def main(argv):
    what = argv[1] if len(argv) > 1 else "all"
    if what in ("all", "classes"):
        classes()
    if what in ("all", "orchestration"):
        orchestration()


if __name__ == "__main__":
    main(sys.argv)
