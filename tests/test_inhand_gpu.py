"""GPU: Isaac-Repose-Cube-Allegro-v0 on the fused HIP path -- the golden of the REAL reference managers (EMA action, the
manipulation/inhand/mdp terms, the root observations on the object), a per-op sweep against the fp64 statements of tests/_inhand_cases.py
with every branch taken and every comparison checked on every env, make_quat_unique with negative and zero real parts, the NoVelObs
layout, a captured against an eager rollout, the refusal of each missing state tensor and what the env refuses on this cfg."""

import copy

import pytest
import torch

import _inhand_cases as ic
import _inhand_oracle as io
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu

OBJECT = {"name": "object"}


def _orientation_error_bound(snaps) -> float:
    """E: the largest |fp32 - fp64| of quat_error_magnitude (the reference's formula, restated step by step in tests/_inhand_oracle.py)
    on these inputs, on the CPU."""
    e = 0.0
    for s in snaps:
        q, g = s["object_root_quat_w"].cpu(), s["command"].cpu()[:, 3:7]
        e = max(e, float((io.quat_error_magnitude(q, g).double() - io.quat_error_magnitude(q.double(), g.double())).abs().max()))
    return e


# ------------------------------------------------------------------------------------------------ the reference golden
@pytest.mark.parametrize("tail", ["deferred", "in_kernel"])
def test_inhand_env_step_matches_reference_golden(tail):
    """Masks, reset ids and episode lengths bit for bit, floats at 1e-5.  track_orientation_inv_l2 = 1 / (dtheta + rot_eps): its relative
    error is |d dtheta| / (dtheta + rot_eps) <= |d dtheta| / rot_eps, and dtheta of the kernel and of the reference each lie within E of
    the exact value, so it -- and the sums that hold it -- gets 1e-5 + 2 E / rot_eps, relative, E measured here on the fixture's inputs."""
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = ic.golden()
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"))
    p = env.plan
    assert p.n_ext_rew == 0 and p.n_ext_term == 0 and p.n_ext_obs == 0 and (p.action_dim, p.obs_dim) == (ic.A, ic.D)
    assert env._lib.imx_observations_kernel_name(env._plan_h) == b"k_obs_inhand<false>"
    E = _orientation_error_bound(g.snapshots())
    tol_track = FLOAT_TOL + 2.0 * E / ic.ROT_EPS
    print(f"E = {E:.3e} rad, track_orientation_inv_l2 tolerance {tol_track:.3e}")
    assert E < 2.0e-6
    env.defer_step_tail = tail == "deferred"
    env._noise_u = torch.zeros(g.N, g.meta["obs_dim"], device="cuda:0")
    env._noise_u.copy_(g.t("reset/noise_u"))
    obs_dict, _ = env.reset()
    torch.cuda.synchronize()
    assert_close(obs_dict["policy"].cpu(), g.t("reset/obs"), FLOAT_TOL, "reset obs")
    env.episode_length_buf = g.t("reset/episode_length_buf")
    names_r = g.meta["reward_terms"]
    for k in range(g.steps):
        tag = f"step{k}"
        env._noise_u.copy_(g.t(f"{tag}/noise_u"))
        obs_dict, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").cuda())
        torch.cuda.synchronize()
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")), "terminated"
        assert torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs")), "time_outs"
        assert torch.equal(env.reset_buf.cpu(), g.t(f"{tag}/reset_buf")), "reset_buf"
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids")), "reset_env_ids"
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf")), "episode_length_buf"
        for name in g.meta["termination_terms"]:
            assert torch.equal(env.termination_manager.get_term(name).cpu(), g.t(f"{tag}/term_dones/{name}")), name
        sr, sr_ref = env.reward_manager._step_reward.cpu(), g.t(f"{tag}/step_reward")
        assert torch.equal(sr[:, 1], sr_ref[:, 1]), "success_bonus"
        err = ((sr[:, 0] - sr_ref[:, 0]).abs() / sr_ref[:, 0].abs()).max()
        print(f"{tag}: track_orientation_inv_l2 max relative error {float(err):.3e}")
        assert_close(sr[:, 0], sr_ref[:, 0], tol_track, f"{tag} track_orientation_inv_l2")
        assert_close(sr[:, 2:], sr_ref[:, 2:], FLOAT_TOL, f"{tag} step_reward")
        assert_close(env._processed_action, g.t(f"{tag}/processed_actions"), FLOAT_TOL, f"{tag} processed_actions")
        assert_close(env.action_manager.action, g.t(f"{tag}/action_after_reset"), FLOAT_TOL, f"{tag} action")
        assert_close(env.action_manager.prev_action, g.t(f"{tag}/prev_action_after_reset"), FLOAT_TOL, f"{tag} prev_action")
        assert_close(rew, g.t(f"{tag}/reward"), tol_track, f"{tag} reward")
        for name in names_r:
            assert_close(env.reward_manager._episode_sums[name], g.t(f"{tag}/episode_sums/{name}"),
                         tol_track if name == "track_orientation_inv_l2" else FLOAT_TOL, f"{tag} {name}")
        assert_close(obs_dict["policy"].cpu(), g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        for key, v in g.log(k).items():
            got = float(extras["log"][key])
            tol = tol_track if key.endswith("track_orientation_inv_l2") else FLOAT_TOL
            assert abs(got - v) <= tol * max(1.0, abs(v)), (key, got, v)
    for name in g.meta["termination_terms"]:
        assert sum(int(g.t(f"step{k}/term_dones/{name}").sum()) for k in range(g.steps)) > 0, name
    env.close()


# ------------------------------------------------------------------------------------------------ per-op sweep against fp64
def _sweep_cfg():
    fx = ic.load_fixture()
    env = fx["env"]
    env["observations"]["policy"]["enable_corruption"] = False
    env["rewards"]["track_pos"] = {"func": f"{ic.INHAND}.rewards:track_pos_l2", "weight": -2.0, "params": {"object_cfg": OBJECT, "command_name": "object_pose"}}
    env["terminations"]["away"] = {"func": f"{ic.INHAND}.terminations:object_away_from_goal", "time_out": False,
                                   "params": {"threshold": ic.GOAL_REACH, "command_name": "object_pose"}}
    return fx


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 257])
def test_inhand_ops_against_fp64_formulas(N):
    """The five in-hand ops of the task, track_pos_l2 and object_away_from_goal, the object's root observations and goal_quat_diff after
    one step against the fp64 statements on the same fp32 inputs, at the 16-env item groups and 64-lane waves of the step kernel, one
    past each, and a ragged multi-workgroup grid.  Every comparison op on every env (the tweak keeps each env a margin from each
    threshold).  Tolerances: FLOAT_TOL, plus 2 E / rot_eps for 1 / (dtheta + rot_eps) as in the golden test (here against fp64: E once
    would do; the same bound is kept), plus the world-coordinate rounding for what subtracts positions far from the origin."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    fx = _sweep_cfg()
    feed = StateFeed(ALLEGRO_HAND, N, "cuda:0", seed=900 + N, num_snapshots=2)
    ic.inhand_tweak(feed, torch.Generator().manual_seed(N))
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    env.reset()
    action = (torch.randn(N, ic.A, generator=torch.Generator().manual_seed(7)) * 0.8).cuda()
    obs, _, _, _, _ = env.step(action)
    torch.cuda.synchronize()
    s = {n: feed[n] for n in ic.NAMES}
    ref = ic.inhand_terms(s)
    ulp = ic.position_rounding(s)
    E = _orientation_error_bound([s])
    sr = env.reward_manager._step_reward.double()
    names = [t.name for t in env.plan.reward_terms]
    for key, name, w, rel, extra in (("track_orientation_inv_l2", "track_orientation_inv_l2", 1.0, FLOAT_TOL + 2.0 * E / ic.ROT_EPS, 0.0),
                                     ("success_bonus", "success_bonus", 250.0, FLOAT_TOL, 0.0), ("track_pos_l2", "track_pos", -2.0, FLOAT_TOL, ulp)):
        got, val = sr[:, names.index(name)] / w, ref[key]
        err = (got - val).abs()
        print(f"N={N} {key}: max err {float(err.max()):.3e}")
        assert bool((err <= rel * val.abs().clamp_min(1.0) + extra).all()), (N, key, float(err.max()))
    assert torch.equal((sr[:, names.index("success_bonus")] > 125.0).double(), ref["success_bonus"]), "success_bonus (dtheta <= threshold) on every env"
    tm = env.termination_manager
    assert torch.equal(tm.get_term("max_consecutive_success"), ref["max_consecutive_success"]), "max_consecutive_success"
    assert torch.equal(tm.get_term("object_out_of_reach"), ref["object_away_from_robot"]), "object_away_from_robot"
    assert torch.equal(tm.get_term("away"), ref["object_away_from_goal"]), "object_away_from_goal"
    margin = min(float((ref["dtheta"][ref["dtheta"] > 0] - ic.f32(ic.SUCCESS_THRESHOLD)).abs().min()) if bool((ref["dtheta"] > 0).any()) else 1.0, 1.0)
    dist_margin = min(float((ref["robot_distance"] - ic.f32(ic.REACH)).abs().min()), float((ref["goal_distance"] - ic.f32(ic.GOAL_REACH)).abs().min()))
    print(f"N={N}: E {E:.3e}, threshold margins {margin:.3e} rad, {dist_margin:.3e} m")
    assert margin >= 0.99 * ic.ANGLE_MARGIN and dist_margin >= ic.DIST_MARGIN
    o = obs["policy"].double()
    for name, scale, extra in (("object_pos", 1.0, ulp[:, None]), ("object_quat", 1.0, 0.0), ("object_lin_vel", 1.0, 0.0), ("object_ang_vel", 0.2, 0.0),
                               ("goal_quat_diff", 1.0, 0.0)):
        lo, hi = ic.COLS[name]
        val = ref[name] * ic.f32(scale) if scale != 1.0 else ref[name]
        err = (o[:, lo:hi] - val).abs()
        assert bool((err <= FLOAT_TOL * val.abs().clamp_min(1.0) + extra).all()), (N, name, float(err.max()))
    assert torch.equal(obs["policy"][:, ic.COLS["object_quat"][0]:ic.COLS["object_quat"][1]], s["object_root_quat_w"])
    assert torch.equal(obs["policy"][:, ic.COLS["goal_pose"][0]:ic.COLS["goal_pose"][1]], s["command"])
    if N >= 64:  # every branch was taken
        c = ic.branch_counts([s])
        c.pop("min_angle_margin"), c.pop("min_distance_margin")
        assert all(v > 0 for v in c.values()), c
    env.close()


# ------------------------------------------------------------------------------------------------ make_quat_unique
def test_make_quat_unique_on_the_object_quaternion_and_the_goal_difference():
    """quat_unique negates where w < 0 and nowhere else: w = +0.0 and w = -0.0 stay as they are."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    N = 65
    fx = ic.load_fixture()
    pol = fx["env"]["observations"]["policy"]
    pol["enable_corruption"] = False
    pol["object_quat"]["params"]["make_quat_unique"] = True
    pol["goal_quat_diff"]["params"]["make_quat_unique"] = True
    feed = StateFeed(ALLEGRO_HAND, N, "cuda:0", seed=31, num_snapshots=1)
    ic.inhand_tweak(feed, torch.Generator().manual_seed(31))
    oq, cmd = feed._stack["object_root_quat_w"][0], feed._stack["command"][0]
    # exact cases: the object's real part +0.0 / -0.0 against the identity goal (the difference is the object's quaternion itself)
    oq[6] = torch.tensor([0.0, 1.0, 0.0, 0.0])
    oq[22] = torch.tensor([-0.0, 0.0, 1.0, 0.0])
    oq[38] = torch.tensor([-0.6, 0.0, 0.8, 0.0])
    for e in (6, 22, 38):
        cmd[e, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    obs, _ = env.reset()
    torch.cuda.synchronize()
    o = obs["policy"].cpu()
    q = feed["object_root_quat_w"].cpu()
    lo, hi = ic.COLS["object_quat"]
    assert torch.equal(o[:, lo:hi], ic.quat_unique(q))  # a copy or its negation: exact
    assert bool((q[:, 0] < 0).any()) and bool((q[:, 0] > 0).any())
    assert torch.equal(o[6, lo:hi], q[6]) and torch.equal(o[22, lo:hi], q[22]) and torch.equal(o[38, lo:hi], -q[38])
    assert torch.signbit(o[22, lo]) and not torch.signbit(o[6, lo])  # -0.0 is not < 0: it is not negated
    d64 = ic.quat_mul(q.double(), ic.quat_conj(feed["command"].cpu()[:, 3:7].double()))
    want = ic.quat_unique(d64)
    lo, hi = ic.COLS["goal_quat_diff"]
    got = o[:, lo:hi].double()
    assert bool((got[:, 0] >= 0).all())
    # (a real part within rounding of zero may come out on either side: the sign of the whole quaternion is then open)
    open_sign = d64[:, 0].abs() < 1.0e-6
    err = torch.minimum((got - want).abs().amax(-1), torch.where(open_sign, (got + want).abs().amax(-1), torch.full((N,), 1.0e9, dtype=torch.float64)))
    assert float(err.max()) <= FLOAT_TOL, float(err.max())
    for e in (6, 22):
        assert torch.equal(got[e].abs(), q[e].double().abs()) and float(got[e, 0]) == 0.0
    assert float((got[38] + q[38].double()).abs().max()) <= FLOAT_TOL  # negated (the product with the identity is no copy: it rounds)
    assert bool((d64[:, 0] < -1.0e-3).any()) and bool((d64[:, 0] > 1.0e-3).any())
    env.close()


# ------------------------------------------------------------------------------------------------ the NoVelObs variant
def test_no_velocity_observation_group_against_the_oracle():
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    N = 67
    fx = ic.load_fixture(ic.TASK_NOVEL)
    fx["env"]["observations"]["policy"]["enable_corruption"] = False
    feed = StateFeed(ALLEGRO_HAND, N, "cuda:0", seed=12, num_snapshots=2)
    ic.inhand_tweak(feed, torch.Generator().manual_seed(12))
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    assert env.plan.obs_dim == ic.D_NOVEL and "object_root_lin_vel_w" not in env.plan.state_reads
    env.reset()
    action = (torch.randn(N, ic.A, generator=torch.Generator().manual_seed(3)) * 0.5).cuda()
    obs, _, _, _, _ = env.step(action)
    torch.cuda.synchronize()
    o = obs["policy"].cpu()
    assert o.shape == (N, ic.D_NOVEL)
    s = {n: feed[n].cpu() for n in ic.NAMES}
    r = io.terms(s, ic.SUCCESS_THRESHOLD, ic.ROT_EPS, float(ic.NUM_SUCCESS), ic.REACH)
    for name in ("object_pos", "object_quat", "goal_pose", "goal_quat_diff"):
        lo, hi = ic.COLS_NOVEL[name]
        extra = ic.position_rounding(s)[:, None].float() if name == "object_pos" else 0.0
        err = (o[:, lo:hi] - r[name]).abs()
        assert bool((err <= FLOAT_TOL * r[name].abs().clamp_min(1.0) + extra).all()), (name, float(err.max()))
    lim = feed["soft_joint_pos_limits"].cpu()
    jp = 2.0 * (feed["joint_pos"].cpu() - (lim[..., 0] + lim[..., 1]) * 0.5) / (lim[..., 1] - lim[..., 0])
    assert_close(o[:, 0:16], jp, FLOAT_TOL, "joint_pos_limit_normalized")
    reset = env.reset_buf.cpu()
    lo, hi = ic.COLS_NOVEL["last_action"]
    assert_close(o[:, lo:hi][~reset], action.cpu()[~reset], FLOAT_TOL, "last_action")
    assert bool((o[:, lo:hi][reset] == 0).all()) and bool(reset.any()) and not bool(reset.all())
    env.close()


# ------------------------------------------------------------------------------------------------ captured = eager
def _rollouts(use_graph, task):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    fx = ic.load_fixture(task)
    torch.manual_seed(23)
    feed = StateFeed(ALLEGRO_HAND, 64, "cuda:0", seed=23, num_snapshots=3)  # (a captured rollout walks the snapshots once per graph)
    ic.inhand_tweak(feed, torch.Generator().manual_seed(23))
    u = ManagerBasedRLEnv(fx, state_feed=feed, seed=23, noise_seed=23)
    env = RslRlVecEnvWrapper(u)
    # (the task's agent cfg has empirical_normalization=True, which the runner rolls out un-fused; off, this is the fused rollout)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=3, empirical_normalization=False), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    assert runner._fusable()
    u.episode_length_buf[::5] = int(u.max_episode_length) - 2  # time-outs inside the recorded rollout
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    out = {k: getattr(st, k).cpu() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    out["processed"] = u._processed_action.cpu()
    env.close()
    return out


@pytest.mark.parametrize("task", [ic.TASK, ic.TASK_NOVEL])
def test_inhand_captured_rollout_equals_eager(task):
    a, c = _rollouts(True, task), _rollouts(False, task)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert float(a["dones"].sum()) > 0 and float(a["rewards"].abs().sum()) > 0
    assert a["observations"].shape == (3, 64, ic.D if task == ic.TASK else ic.D_NOVEL) and a["actions"].shape == (3, 64, ic.A)


# ------------------------------------------------------------------------------------------------ refusals at the launch checks
@pytest.mark.parametrize("missing", ["object_root_quat_w", "object_root_lin_vel_w", "object_root_ang_vel_w", "command_consecutive_success"])
def test_missing_state_tensor_is_refused_with_a_message_not_a_fault(missing):
    """Host-side validation only: the launch checks name the tensor and no kernel goes out with a NULL pointer."""
    from isaaclab_amd._lib import ImxError
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    full = StateFeed(ALLEGRO_HAND, 33, "cuda:0", seed=2, num_snapshots=2)
    full.ensure_object_state()
    bare = StateFeed.from_tensors(ALLEGRO_HAND, [{n: v for n, v in full.snapshot(k).items() if n != missing} for k in range(2)], device="cuda:0")
    assert missing not in bare.names()
    fx = ic.load_fixture()
    pol = fx["env"]["observations"]["policy"]
    if missing == "command_consecutive_success":  # read by a termination only
        env = ManagerBasedRLEnv(fx, state_feed=bare)
        env.reset()
        before = env._counters.clone()
        with pytest.raises(ImxError, match=f"'{missing}' is required by a term"):
            env.step(torch.zeros(33, ic.A, device="cuda:0"))  # the step launch check
        torch.cuda.synchronize()
        assert torch.equal(env._counters, before)  # no launch went out: the step counter did not move
        env.close()
        return
    env = ManagerBasedRLEnv(fx, state_feed=bare)
    with pytest.raises(ImxError, match=f"'{missing}' is required by an observation term"):
        env.reset()  # the observation launch check
    env.close()
    if missing == "object_root_quat_w":  # also read by the two rewards: without the observation terms the step check names it
        del pol["object_quat"], pol["goal_quat_diff"]
        env = ManagerBasedRLEnv(fx, state_feed=bare)
        env.reset()
        before = env._counters.clone()
        with pytest.raises(ImxError, match=f"'{missing}' is required by a term"):
            env.step(torch.zeros(33, ic.A, device="cuda:0"))
        torch.cuda.synchronize()
        assert torch.equal(env._counters, before)
        env.close()


def test_mixed_plans_are_refused_by_the_step_launch():
    """An in-hand op beside a lift op: refused with a message by imx_terminations_rewards, before any launch."""
    from isaaclab_amd._lib import ImxError
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    fx = ic.load_fixture()
    fx["env"]["rewards"]["lifted"] = {"func": "isaaclab_tasks.manager_based.manipulation.lift.mdp.rewards:object_is_lifted", "weight": 1.0,
                                      "params": {"minimal_height": 0.04, "object_cfg": OBJECT}}
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(ALLEGRO_HAND, 16, "cuda:0", seed=1, num_snapshots=2))
    env.reset()
    with pytest.raises(ImxError, match="in-hand .* ops beside classic/humanoid, reach, lift or navigation ops is not supported"):
        env.step(torch.zeros(16, ic.A, device="cuda:0"))
    env.close()


# ------------------------------------------------------------------------------------------------ what the env refuses on this cfg
def test_env_refusals():
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.producers import InHandReOrientationCommand
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.state_feed import StateFeed

    fx = ic.load_fixture()
    feed = StateFeed(ALLEGRO_HAND, 16, "cuda:0", seed=1, num_snapshots=2)
    stand_alone = "is stand-alone: the orchestration launch does not run it yet"
    with pytest.raises(NotImplementedError, match=f"command_term='object_pose'.*{stand_alone}"):
        ManagerBasedRLEnv(copy.deepcopy(fx), state_feed=feed, command_term="object_pose")
    term = InHandReOrientationCommand(fx["env"]["commands"]["object_pose"], 16, 1.0 / 30.0, "cuda:0", seed=0, env_origins=feed["env_origins"],
                                      default_object_pos=(0.0, -0.19, 0.56))
    with pytest.raises(NotImplementedError, match=f"command_term=<producers.InHandReOrientationCommand>.*{stand_alone}"):
        ManagerBasedRLEnv(copy.deepcopy(fx), state_feed=feed, command_term=term)
    no_kernel = "event term 'reset_robot_joints': 'reset_joints_within_limits_range' has no kernel"
    with pytest.raises(NotImplementedError, match=no_kernel):
        ManagerBasedRLEnv(copy.deepcopy(fx), state_feed=feed, events_cfg=True)
    with pytest.raises(NotImplementedError, match=no_kernel):
        ManagerBasedRLEnv(copy.deepcopy(fx), state_feed=feed, own_managers=True)
    env = ManagerBasedRLEnv(copy.deepcopy(fx), state_feed=feed)  # the plain env runs: command, metric and object state from the feed
    assert env.command_term is None and env.event_manager is None
    assert torch.equal(env.command_manager.get_command("object_pose"), feed["command"])
    env.close()
