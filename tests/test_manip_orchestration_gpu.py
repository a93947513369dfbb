"""GPU: the manipulation tasks' ``_reset_idx`` inside the one orchestration launch (``imx_reset_orchestrate_manip``) --
``reset_scene_to_default``, ``reset_root_state_uniform`` on the rigid object and the device-side ``modify_reward_weight`` switch -- against
the fixtures of the REAL reference (tools/gen_golden_manip_orchestration.py) and the numpy restatement (tests/_manip_orch_oracle.py)."""

import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _manip_orch_oracle as mo
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

NAN_BITS = 0x7FC0BEEF


def _env(g, fixture=None, **kw):
    from isaaclab_amd.env import ManagerBasedRLEnv

    return ManagerBasedRLEnv(fixture or g.fixture, state_feed=g.feed("cuda:0"), own_managers=True, reward_curriculum=True, **kw)


def _feed_draws(env, g, slot):
    d = g.draws(slot)
    for t in env.event_manager.terms:
        if t.width:
            t.uniforms = d[t.name][:, :t.width].cuda().contiguous()
    env._orch_draws["command"] = d["command"].cuda().contiguous()


def _weights(env, g):
    return {n: float(env.reward_manager.get_term_cfg(n).weight) for n in g.meta["reward_terms"]}


# ------------------------------------------------------------------------------------------------ parity with the real managers
@pytest.mark.parametrize("which", ["lift", "reach"])
def test_orchestration_matches_the_real_managers(which):
    """``own_managers=True, reward_curriculum=True`` on the fixture's cfg, fed the recorded draws, ``reset()`` + every recorded step:
    masks, ids and trigger state exact; both weights the reference's after every step, changing on exactly the recorded steps; all
    ``sim_writes`` (the object's two among them on Lift), reward, ``_step_reward``, episode sums, observations, the command term's state
    and every log entry within 1e-5."""
    g = mo.ManipOrchGolden(which)
    env = _env(g)
    assert env.event_manager.active_terms == g.meta["event_terms"] and env.curriculum_manager.active_terms == g.meta["curriculum_terms"]
    assert env.command_manager.active_terms == [g.meta["command_term"]] and env.command_term.body_idx == g.body_idx
    assert env._orch_manip is None  # (built with the first launch)
    assert set(g.write_keys) <= set(env.sim_writes) and ("object_root_pose" in env.sim_writes) == (which == "lift")
    ev, ct = env.event_manager, env.command_term

    def check(tag, extras):
        torch.cuda.synchronize()
        for k in g.write_keys:
            assert_close(env.sim_writes[k], g.t(f"{tag}/sim_writes/{k}"), FLOAT_TOL, f"{tag} sim_writes[{k}]")
        for k, a in (("command", ct.command), ("pose_command_w", ct.pose_command_w), ("command_time_left", ct.time_left),
                     ("metric_position_error", ct.metrics["position_error"]), ("metric_orientation_error", ct.metrics["orientation_error"])):
            assert_close(a, g.t(f"{tag}/{k}"), FLOAT_TOL, f"{tag} {k}")
        assert torch.equal(ct.command_counter.cpu(), g.t(f"{tag}/command_counter")), f"{tag} command counter"
        assert torch.equal(torch.stack([t.last_triggered_step.cpu() for t in ev.terms]).long(), g.t(f"{tag}/reset_last_triggered_step").long()), tag
        assert torch.equal(torch.stack([t.triggered_once.cpu() for t in ev.terms]), g.t(f"{tag}/reset_triggered_once")), tag
        assert_close(env._episode_sums, g.t(f"{tag}/episode_sums"), FLOAT_TOL, f"{tag} episode sums")
        for key, v in g.log(tag).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (tag, key, got, v)
        w, ref = _weights(env, g), g.weights(tag)
        for n in ref:
            assert np.float32(w[n]) == np.float32(ref[n]), (tag, n, w[n], ref[n])
        return w

    _feed_draws(env, g, 0)
    obs, extras = env.reset()
    assert env._orch_manip is not None
    assert_close(obs["policy"], g.t("reset/obs"), FLOAT_TOL, "reset obs")
    prev = check("reset", extras)
    env.episode_length_buf = g.t("reset/episode_length_buf")
    changes, resets = {}, 0
    for k in range(g.steps):
        tag = f"step{k}"
        _feed_draws(env, g, k + 1)
        obs, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").cuda())
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")) and torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs"))
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids"))
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf"))
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(env._step_reward, g.t(f"{tag}/step_reward"), FLOAT_TOL, f"{tag} step reward")
        assert_close(obs["policy"], g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        w = check(tag, extras)
        changes.update({n: k for n in w if w[n] != prev[n]})
        prev = w
        resets += len(g.t(f"{tag}/reset_env_ids"))
    assert changes == g.meta["weight_change_steps"] and resets == g.meta["n_resets"]
    env.close()


# ------------------------------------------------------------------------------------------------ the launch alone
def _lift_env(N, curriculum=None, rewards=None, snapshots=2, seed=3, **kw):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    fx = copy.deepcopy(mo.ManipOrchGolden("lift").fixture)
    for name, p in (curriculum or {}).items():
        fx["env"]["curriculum"][name]["params"].update(p)
    for name, w in (rewards or {}).items():
        fx["env"]["rewards"][name]["weight"] = w
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=seed, num_snapshots=snapshots)
    feed._stack["object_root_pos_w"][..., 2].abs_().add_(0.02)  # (no cube drops: the resets are the test's own)
    return ManagerBasedRLEnv(fx, state_feed=feed, own_managers=True, reward_curriculum=True, num_envs=N, **kw), fx


@pytest.mark.parametrize("N", [100, 1])
def test_masking_and_tails(N):
    """N no multiple of 64 and N = 1; ``sim_writes`` pre-filled with a NaN bit pattern; a mask with a few rows set, the last env among
    them: rows not reset keep their bits, reset rows equal the restatement."""
    env, fx = _lift_env(N)
    g = mo.ManipOrchGolden("lift")
    keys = g.write_keys
    nan = torch.tensor(NAN_BITS, dtype=torch.int32).view(torch.float32).item()
    for k in keys:
        env.sim_writes[k].fill_(nan)
    before = {k: env.sim_writes[k].clone() for k in keys}
    mask = np.zeros(N, bool)
    mask[[i for i in (0, 3, 63, 64, 70, N - 1) if i < N]] = True
    rng = np.random.default_rng(N)
    u = rng.random((N, 12), np.float32)
    env.feed["env_origins"].copy_(torch.from_numpy(rng.normal(size=(N, 3)).astype(np.float32) * 4))  # (a single env sits at the world origin)
    env.event_manager.get_term("reset_object_position").uniforms = torch.from_numpy(u).cuda()
    env._counters[2] = 5
    env._orchestrate(torch.from_numpy(mask).cuda(), do_step=False)
    torch.cuda.synchronize()
    f = env.feed
    st = {k: f[k].cpu().numpy() for k in ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits", "env_origins")}
    st["default_root_state"], st["default_object_root_state"] = env.default_root_state.cpu().numpy(), env.default_object_root_state.cpu().numpy()
    assert np.abs(st["env_origins"]).max() > 0 and tuple(st["default_object_root_state"][0, :3]) == (0.5, 0.0, np.float32(0.055))
    sw = {k: np.zeros(tuple(v.shape), np.float32) for k, v in before.items()}
    trig = {"last": np.zeros((2, N), np.int64), "once": np.zeros((2, N), bool)}
    ids = np.nonzero(mask)[0]
    mo.apply_reset_events(g.events, ids, 5, sw, trig, st, {"reset_object_position": u}, "object")
    for k in keys:
        got = env.sim_writes[k].cpu()
        assert torch.equal(got[~mask].view(torch.int32), before[k].cpu()[~mask].view(torch.int32)), f"sim_writes[{k}]: a row that did not reset changed"
        assert_close(got[mask], sw[k][mask], FLOAT_TOL, f"sim_writes[{k}]")
    for i, t in enumerate(env.event_manager.terms):
        assert np.array_equal(t.last_triggered_step.cpu().numpy(), trig["last"][i]) and np.array_equal(t.triggered_once.cpu().numpy(), trig["once"][i])
    env.close()


def test_no_reset_no_switch():
    """The step counter far beyond ``num_steps`` and an all-false reset mask: the weight word is unchanged.  One reset switches it."""
    env, fx = _lift_env(100)
    old = {n: fx["env"]["rewards"][n]["weight"] for n in ("action_rate", "joint_vel")}
    env._counters[2] = 100000
    none = torch.zeros(100, dtype=torch.bool, device="cuda:0")
    for _ in range(2):
        env._orchestrate(none, do_step=False)
    for n in old:
        assert np.float32(env.reward_manager.get_term_cfg(n).weight) == np.float32(old[n])
    one = none.clone()
    one[99] = True
    env._counters[2] = 12  # the first threshold is not crossed at 12 (the condition is a strict >), the second not either
    env._orchestrate(one, do_step=False)
    assert np.float32(env.reward_manager.get_term_cfg("action_rate").weight) == np.float32(old["action_rate"])
    env._counters[2] = 13
    env._orchestrate(one, do_step=False)
    assert np.float32(env.reward_manager.get_term_cfg("action_rate").weight) == np.float32(-0.1)
    assert np.float32(env.reward_manager.get_term_cfg("joint_vel").weight) == np.float32(old["joint_vel"])
    env._counters[2] = 100000
    env._orchestrate(one, do_step=False)
    assert np.float32(env.reward_manager.get_term_cfg("joint_vel").weight) == np.float32(-0.1)
    env.close()


def _wake_sleep_env():
    """Lift with ``joint_vel`` asleep (weight 0) and a curriculum that wakes it (-0.5) and puts ``action_rate`` to sleep (0) once
    ``common_step_counter > 1`` in a step that resets an env: two steps without a reset, then env 7 times out in the third.  Two
    workgroups (N = 100), of which the second has no reset env: the switch and what goes with it reach its envs too."""
    N = 100
    env, fx = _lift_env(N, curriculum={"action_rate": dict(weight=0.0, num_steps=1), "joint_vel": dict(weight=-0.5, num_steps=1)},
                        rewards={"joint_vel": 0.0}, snapshots=4)
    names = list(env.reward_manager.active_terms)
    ia, ij = names.index("action_rate"), names.index("joint_vel")
    gen = torch.Generator().manual_seed(1)
    act = lambda: torch.randn(N, env.plan.action_dim, generator=gen).cuda()  # noqa: E731
    env.reset()
    env.step(act())
    env.step(act())  # common_step_counter 2 > 1, but no env resets
    sr = env._step_reward.clone()
    assert float(sr[:, ia].abs().min()) > 0.0 and not bool(sr[:, ij].any())
    ep = torch.zeros(N, dtype=torch.long)
    ep[7] = env.max_episode_length - 1
    env.episode_length_buf = ep
    env.step(act())  # env 7 times out: the switch happens after this step's reward
    before = env._step_reward.clone()
    assert env.reset_env_ids.cpu().tolist() == [7]
    assert float(before[:, ia].abs().min()) > 0.0 and not bool(before[:, ij].any())
    sums = env._episode_sums.clone()
    _, rew, _, _, _ = env.step(act())
    return env, ia, ij, before, sums, rew


def test_wake():
    """A curriculum term taking a weight from 0 to non-zero: the next step's ``_step_reward`` column becomes non-zero, the term enters
    the reward and its episode sum starts to move."""
    env, ia, ij, before, sums, rew = _wake_sleep_env()
    sr = env._step_reward
    assert float(sr[:, ij].abs().min()) > 0.0 and float((env._episode_sums[ij] - sums[ij]).abs().min()) > 0.0
    assert_close(rew, (sr.sum(dim=1) - sr[:, ia]) * env.step_dt, FLOAT_TOL, "reward = every awake term")
    env.close()


def test_sleep():
    """A curriculum term taking a weight to 0: the sleeping term leaves the reward, its episode sum stops, and the next step's
    ``_step_reward`` column is zero for EVERY env, not only the one that reset.  The zero-weight skip (reward_manager.py:145-146) never
    writes the column of a sleeping term, in ``k_term_rew`` as in the reference, so it is the orchestration launch of the step after the switch
    that zeroes it (left to the skip alone it would keep the values of the last step the term was awake); the step of the switch itself
    still shows that step's values (``_wake_sleep_env`` asserts it)."""
    env, ia, ij, before, sums, rew = _wake_sleep_env()
    sr = env._step_reward
    assert_close(rew, (sr.sum(dim=1) - sr[:, ia]) * env.step_dt, FLOAT_TOL, "reward = every awake term")
    keep = torch.ones(sr.shape[0], dtype=torch.bool, device=sr.device)
    keep[7] = False  # (env 7 was reset: its sums restarted)
    assert torch.equal(env._episode_sums[ia][keep], sums[ia][keep])
    assert not bool(sr[:, ia].any())
    env.close()


def test_set_term_cfg_keeps_a_switched_weight():
    """After a device-side switch ``get_term_cfg`` reports the new weight, and ``set_term_cfg`` on a DIFFERENT term (a recompile of the
    tables from the host's cfg) leaves the switched weight in place on the device."""
    N = 64
    env, fx = _lift_env(N, curriculum={"action_rate": dict(num_steps=0), "joint_vel": dict(num_steps=10 ** 6)}, snapshots=4)
    names = list(env.reward_manager.active_terms)
    ia = names.index("action_rate")
    env.reset()
    assert env.reward_manager.get_term_cfg("action_rate").weight == fx["env"]["rewards"]["action_rate"]["weight"] == -1e-4  # 0 > 0 is false
    a = torch.randn(N, env.plan.action_dim, generator=torch.Generator().manual_seed(2)).cuda()
    env.step(a)
    env.reset(env_ids=torch.tensor([5], device="cuda:0"))  # _reset_idx at common_step_counter 1
    assert env.reward_manager.get_term_cfg("action_rate").weight == -0.1 and env.plan.reward_terms[ia].weight == -0.1
    c = env.reward_manager.get_term_cfg("lifting_object")
    c.weight = 3.0
    env.reward_manager.set_term_cfg("lifting_object", c)
    from isaaclab_amd import _lib

    host = ctypes.c_float()
    _lib.check(_lib.lib().imx_plan_reward_weight_get(env._plan_h, ia, _lib.current_stream(env.device), ctypes.byref(host)))
    assert np.float32(host.value) == np.float32(-0.1)
    env.step(a * 0.5)
    env.step(a)
    d = a - a * 0.5
    assert_close(env._step_reward[:, ia], -0.1 * torch.sum(torch.square(d), dim=1), FLOAT_TOL, "action_rate at the switched weight")
    assert np.float32(env.reward_manager.get_term_cfg("joint_vel").weight) == np.float32(fx["env"]["rewards"]["joint_vel"]["weight"])
    env.close()


def test_refusals_on_the_device_path():
    """Without the keyword ``own_managers=True`` on Lift stops at the curriculum manager, naming the keyword; the C entry points name
    what they lack."""
    from isaaclab_amd import _abi, _lib
    from isaaclab_amd._lib import ImxOrch, ImxOrchManip
    from isaaclab_amd.env import ManagerBasedRLEnv

    ops = _abi.ENUMS["imx_event_op"]
    root_uniform, scene_default = ops["IMX_E_RESET_ROOT_STATE_UNIFORM"], ops["IMX_E_RESET_SCENE_TO_DEFAULT"]

    g = mo.ManipOrchGolden("lift")
    with pytest.raises(NotImplementedError, match="modify_reward_weight.*reward_curriculum=True"):
        ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"), own_managers=True)
    N = 8
    z = lambda *s: torch.zeros(*s, device="cuda:0")  # noqa: E731
    t = dict(org=z(N, 3), d=z(N, 13), pose=z(N, 7), vel=z(N, 6), last=torch.zeros(N, dtype=torch.int32, device="cuda:0"),
             once=torch.zeros(N, dtype=torch.uint8, device="cuda:0"), w=z(1), cnt=torch.zeros(1, dtype=torch.int32, device="cuda:0"))
    o = ImxOrch(num_envs=N, num_joints=1, num_bodies=1, dt=0.02, env_origins_d=t["org"].data_ptr(), num_terms=1, step_counter_d=t["cnt"].data_ptr())
    T = o.terms[0]
    T.op, T.asset, T.last_triggered_step_d, T.triggered_once_d = root_uniform, 1, t["last"].data_ptr(), t["once"].data_ptr()
    L, s = _lib.lib(), _lib.current_stream(torch.device("cuda:0"))
    err = lambda: L.imx_last_error().decode()  # noqa: E731
    assert L.imx_reset_orchestrate(ctypes.byref(o), s) != 0 and "imx_reset_orchestrate_manip" in err()
    m = ImxOrchManip()
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "rigid object" in err()
    m.object_default_root_state_d, m.object_root_pose_out_d, m.object_root_vel_out_d = t["d"].data_ptr(), t["pose"].data_ptr(), t["vel"].data_ptr()
    m.num_weight_terms = _lib.ORCH_MAX_WEIGHT_TERMS + 1
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "weight terms" in err()
    m.num_weight_terms = 1
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "weight address" in err()
    T.asset = 2
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "asset 2" in err()
    T.asset, T.op = 0, scene_default
    assert L.imx_reset_orchestrate(ctypes.byref(o), s) != 0 and "reset_scene_to_default" in err()
    T.op, T.asset = root_uniform, 1
    m.weight_terms[0].weight_d, m.weight_terms[0].weight, m.weight_terms[0].num_steps = t["w"].data_ptr(), 2.5, -1
    m.weight_terms[0].step_reward_d = t["vel"].data_ptr()
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "step_reward_stride" in err()
    m.weight_terms[0].step_reward_d = None
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) == 0, err()  # complete: every env resets (no mask)
    torch.cuda.synchronize()
    assert float(t["w"]) == 2.5 and bool((t["pose"][:, 3:].abs().sum(dim=1) == 0).all()) and bool(t["once"].all())
    out = ctypes.c_void_p()
    assert L.imx_plan_reward_weight_ptr(None, 0, ctypes.byref(out)) != 0 and "null" in err()


def test_weight_curriculum_beside_what_its_launch_lacks_is_refused_at_construction():
    """The launch that switches reward weights has no terrain curriculum and no velocity command: a cfg that asks for either beside a
    ``modify_reward_weight`` term is refused when the env is built, with the term's name, not at the first launch."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.events import TerrainImporterState
    from isaaclab_amd.robots import ANYMAL_C
    from isaaclab_amd.state_feed import StateFeed

    N = 64
    fx = load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")
    target = next(n for n, t in fx["env"]["rewards"].items() if t is not None)
    switch = {"func": "isaaclab.envs.mdp.curriculums:modify_reward_weight", "params": {"term_name": target, "weight": -0.5, "num_steps": 10}}
    levels = {"func": "isaaclab_tasks.manager_based.locomotion.velocity.mdp.curriculums:terrain_levels_vel", "params": {}}
    ti = TerrainImporterState(torch.zeros(2, 2, 3, device="cuda:0"), torch.zeros(N, dtype=torch.long, device="cuda:0"),
                              torch.zeros(N, dtype=torch.long, device="cuda:0"), 8.0)
    kw = dict(use_command_term=True, use_curriculum=True, reward_curriculum=True, terrain_importer=ti)
    fx["env"]["curriculum"] = {"terrain_levels": levels, "slow_down": switch}
    with pytest.raises(NotImplementedError, match="'slow_down'.*terrain_levels_vel \\('terrain_levels'\\)"):
        ManagerBasedRLEnv(fx, state_feed=StateFeed(ANYMAL_C, N, "cuda:0", seed=3, num_snapshots=2), **kw)
    fx["env"]["curriculum"] = {"slow_down": switch}
    with pytest.raises(NotImplementedError, match="'slow_down'.*velocity command term 'base_velocity'"):
        ManagerBasedRLEnv(fx, state_feed=StateFeed(ANYMAL_C, N, "cuda:0", seed=3, num_snapshots=2), **kw)


def test_reach_ur10_switches_its_weights():
    """Isaac-Reach-UR10-v0 with ``own_managers=True, reward_curriculum=True``: its two curriculum terms, with thresholds 1 and 3, switch
    on the first step with a reset whose ``common_step_counter`` exceeds them, and ``action_rate`` is then paid at the new weight."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg("Isaac-Reach-UR10-v0")
    cur = {n: t["params"] for n, t in fx["env"]["curriculum"].items()}
    assert sorted(p["term_name"] for p in cur.values()) == ["action_rate", "joint_vel"]
    for p in cur.values():
        p["num_steps"] = 1 if p["term_name"] == "action_rate" else 3
    old = {p["term_name"]: fx["env"]["rewards"][p["term_name"]]["weight"] for p in cur.values()}
    N = 100
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(ROBOTS[fx["robot"]], N, "cuda:0", seed=3, num_snapshots=4), own_managers=True,
                            reward_curriculum=True, seed=11)
    assert env.curriculum_manager.active_terms == list(cur) and env.command_term is not None
    ia = list(env.reward_manager.active_terms).index("action_rate")
    gen = torch.Generator().manual_seed(4)
    env.reset()
    prev = None
    for k in range(1, 6):
        paid = np.float32(env.reward_manager.get_term_cfg("action_rate").weight)  # the weight this step's reward is computed with
        ep = torch.zeros(N, dtype=torch.long)
        ep[99] = env.max_episode_length - 1  # env 99 times out in every step, so every step runs _reset_idx
        env.episode_length_buf = ep
        a = torch.randn(N, env.plan.action_dim, generator=gen).cuda()
        env.step(a)
        assert env.reset_env_ids.cpu().tolist() == [99]
        for p in cur.values():
            want = p["weight"] if k > p["num_steps"] else old[p["term_name"]]
            assert np.float32(env.reward_manager.get_term_cfg(p["term_name"]).weight) == np.float32(want), (k, p["term_name"])
        if prev is not None:
            assert_close(env._step_reward[:98, ia], float(paid) * torch.sum(torch.square(a - prev), dim=1)[:98], FLOAT_TOL, f"step {k} action_rate")
        prev = a
    assert env._orch_manip is not None
    env.close()


# ------------------------------------------------------------------------------------------------ captured rollout
def test_weights_switch_inside_a_captured_rollout(tmp_path):
    """Lift, N = 256, ``OnPolicyRunner(use_graph=True)``, 8 steps per iteration, thresholds inside the second iteration; three
    iterations.  The weights switch without a re-capture, and the storage of a ``use_graph=False`` run with the same seeds is
    bit-identical."""
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    N, T = 256, 8
    runs = []
    os.environ["IMX_RUNNER_QUIET"] = "1"
    try:
        for graph in (True, False):
            # the graph run warms up with one eager rollout before it captures: thresholds count from there (device step counter)
            env, fx = _lift_env(N, curriculum={"action_rate": dict(num_steps=2 * T + 2), "joint_vel": dict(num_steps=2 * T + 5)}, snapshots=T, seed=9,
                                noise_seed=5)
            env.seed(21)
            venv = RslRlVecEnvWrapper(env)
            runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=T), log_dir=str(tmp_path / f"g{int(graph)}"), device="cuda:0", use_graph=graph)
            assert runner._fusable()
            venv.episode_length_buf = env.max_episode_length - 1 - (torch.arange(N) % 40)  # a few envs time out on every step
            if not graph:  # the same warm-up rollout, discarded
                runner.collect()
                runner.alg.storage.clear()
            seen = []
            for it in range(3):
                runner.learn(1)
                torch.cuda.synchronize()
                seen.append((np.float32(env.reward_manager.get_term_cfg("action_rate").weight), np.float32(env.reward_manager.get_term_cfg("joint_vel").weight),
                             runner._graph))
            st = runner.alg.storage
            runs.append((seen, {k: getattr(st, k).clone() for k in ("observations", "actions", "rewards", "dones", "values")}))
            env.close()
    finally:
        os.environ.pop("IMX_RUNNER_QUIET", None)
    (seen, store), (seen_e, store_e) = runs
    old = (np.float32(-1e-4), np.float32(-1e-4))
    assert seen[0][:2] == old and seen[1][:2] == (np.float32(-0.1), np.float32(-0.1)) and seen[2][:2] == seen[1][:2]
    assert seen[0][2] is not None and seen[0][2] is seen[1][2] is seen[2][2]  # one capture
    assert [s[:2] for s in seen_e] == [s[:2] for s in seen]
    for k in store:
        assert torch.equal(store[k], store_e[k]), f"storage.{k} differs between the captured and the eager rollout"


# ------------------------------------------------------------------------------------------------ fixed-seed cases of the sweep
@pytest.mark.parametrize("seed", range(700, 706))
def test_manip_orchestration_sweep(seed):
    import fuzz_orchestration

    fuzz_orchestration.one_case_manip(seed)
