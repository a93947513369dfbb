"""GPU: Isaac-Open-Drawer-Franka-v0 on the fused HIP path -- the golden of the REAL reference managers (arm and binary gripper action,
the manipulation/cabinet/mdp rewards, the joint observations on the cabinet, rel_ee_drawer_distance; a short step of each IK variant), a sweep of all ten ops against the
fp64 statements of tests/_cabinet_oracle.py with every branch taken and every comparison checked on every env, k_frame_transformer
against its fixture and against fp64, env.scene[...] against what the fused ops used, a captured against an eager rollout, one learning
iteration, and the refusal of each missing tensor of the new struct."""

import pytest
import torch

import _cabinet_cases as cc
import _cabinet_oracle as co
from _task_space_cases import SENTINEL
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu


def _feed(N, seed, snapshots=2):
    from isaaclab_amd.robots import FRANKA_PANDA_CABINET
    from isaaclab_amd.state_feed import StateFeed

    feed = StateFeed(FRANKA_PANDA_CABINET, N, "cuda:0", seed=seed, num_snapshots=snapshots)
    cc.cabinet_tweak(feed, torch.Generator().manual_seed(seed))
    return feed


# ------------------------------------------------------------------------------------------------ the reference golden
@pytest.mark.parametrize("task,tail", [(cc.TASK, "deferred"), (cc.TASK, "in_kernel"), (cc.TASK_IK_ABS, "deferred"), (cc.TASK_IK_REL, "deferred")])
def test_cabinet_env_step_matches_reference_golden(task, tail):
    """Masks, reset ids and episode lengths bit for bit, floats at FLOAT_TOL.  The two IK variants (the real
    DifferentialInverseKinematicsAction in the fixture; the env's differential-IK term on the recorded Jacobians): a short fixture each."""
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = cc.golden(task)
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"))
    p = env.plan
    assert p.n_ext_rew == 0 and p.n_ext_term == 0 and p.n_ext_obs == 0
    assert (p.action_dim, p.processed_action_dim, p.obs_dim) == cc.DIMS[task] == (g.meta["action_dim"], g.meta["processed_action_dim"], g.meta["obs_dim"])
    assert len(p.ik_terms) == (0 if task == cc.TASK else 1)
    assert env._lib.imx_observations_kernel_name(env._plan_h) == b"k_obs_cabinet<true>"
    env.defer_step_tail = tail == "deferred"
    env._noise_u = torch.zeros(g.N, g.meta["obs_dim"], device="cuda:0")
    env._noise_u.copy_(g.t("reset/noise_u"))
    obs_dict, _ = env.reset()
    torch.cuda.synchronize()
    assert_close(obs_dict["policy"].cpu(), g.t("reset/obs"), FLOAT_TOL, "reset obs")
    env.episode_length_buf = g.t("reset/episode_length_buf")
    names_r = g.meta["reward_terms"]
    bool_terms = [names_r.index(n) for n in ("align_grasp_around_handle", "multi_stage_open_drawer")]
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
        for i in bool_terms:  # sums of exact constants selected by the comparisons: bit for bit
            assert torch.equal(sr[:, i], sr_ref[:, i]), names_r[i]
        assert_close(sr, sr_ref, FLOAT_TOL, f"{tag} step_reward")
        assert_close(env._processed_action, g.t(f"{tag}/processed_actions"), FLOAT_TOL, f"{tag} processed_actions")
        assert_close(env.action_manager.action, g.t(f"{tag}/action_after_reset"), FLOAT_TOL, f"{tag} action")
        assert_close(env.action_manager.prev_action, g.t(f"{tag}/prev_action_after_reset"), FLOAT_TOL, f"{tag} prev_action")
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        for name in names_r:
            assert_close(env.reward_manager._episode_sums[name], g.t(f"{tag}/episode_sums/{name}"), FLOAT_TOL, f"{tag} {name}")
        assert_close(obs_dict["policy"].cpu(), g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        for key, v in g.log(k).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (key, got, v)
    assert sum(int(g.t(f"step{k}/time_outs").sum()) for k in range(g.steps)) > 0
    env.close()


# ------------------------------------------------------------------------------------------------ per-op sweep against fp64
def _sweep_cfg():
    fx = cc.load_fixture()
    pol = fx["env"]["observations"]["policy"]
    pol["enable_corruption"] = False
    for f in ("ee_pos", "ee_quat", "fingertips_pos"):  # the three observation terms the task cfg leaves out, behind its own
        pol[f] = {"func": f"{cc.CABINET}.observations:{f}", "params": {}}
    return fx


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 257])
def test_cabinet_ops_against_fp64_formulas(N):
    """The seven rewards, the joint observations on the cabinet and the four frame observations after one step against the fp64
    statements on the same fp32 inputs, at the 16-env item groups and 64-lane waves of the step kernel, one past each, and a ragged
    multi-workgroup grid.  Every comparison on every env: the tweak keeps each env a margin from each threshold, and the test requires
    it.  Tolerance: FLOAT_TOL relative to max(1, |value|), on every term."""
    from isaaclab_amd.env import ManagerBasedRLEnv

    fx = _sweep_cfg()
    feed = _feed(N, 700 + N)
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    assert env._lib.imx_observations_kernel_name(env._plan_h) == b"k_obs_cabinet<true>"
    env.reset()
    action = (torch.randn(N, cc.A, generator=torch.Generator().manual_seed(7)) * 0.8).cuda()
    obs, _, _, _, _ = env.step(action)
    torch.cuda.synchronize()
    s = {n: feed[n] for n in cc.NAMES}
    scene = cc.scene_of()
    ref = cc.cabinet_terms(s, scene)
    c = cc.branch_counts([s], scene)
    print(f"N={N}: margins {c['min_distance_margin']:.3e} m, {c['min_gap_margin']:.3e} m, {c['min_joint_margin']:.3e} m")
    assert cc.margins_hold(c), c
    sr = env.reward_manager._step_reward.double().cpu()
    names = [t.name for t in env.plan.reward_terms]
    for name in cc.REWARDS[:7]:
        got, val = sr[:, names.index(name)] / cc.WEIGHTS[name], ref[name]
        err = (got - val).abs()
        print(f"N={N} {name}: max err {float(err.max()):.3e}")
        assert bool((err <= FLOAT_TOL * val.abs().clamp_min(1.0)).all()), (N, name, float(err.max()))
    # the step functions, on every env: their values lie 0.5 apart (the manager's value * dt / dt may cost an ulp)
    g = ref["is_graspable"].double()
    assert float((sr[:, names.index("align_grasp_around_handle")] / cc.WEIGHTS["align_grasp_around_handle"] - g).abs().max()) < 1.0e-6
    assert float((sr[:, names.index("multi_stage_open_drawer")] - ref["multi_stage_open_drawer"]).abs().max()) < 1.0e-6
    close = ref["distance"] <= cc.f32(cc.GRASP_THRESHOLD)
    assert torch.equal(sr[:, names.index("grasp_handle")] != 0, close & (ref["grasp_handle"] != 0))
    twice = sr[:, names.index("approach_ee_handle")] / cc.WEIGHTS["approach_ee_handle"] > (1.0 / (1.0 + ref["distance"] ** 2)) ** 2 * 1.5
    assert torch.equal(twice, ref["distance"] <= cc.f32(cc.APPROACH_THRESHOLD))
    o = obs["policy"].double().cpu()
    cols = dict(cc.COLS, ee_pos=(31, 34), ee_quat=(34, 38), fingertips_pos=(38, 44))
    want = dict(ref, ee_quat=co.quat_unique(ref["ee_quat"]))
    for name in ("cabinet_joint_pos", "cabinet_joint_vel", "rel_ee_drawer_distance", "ee_pos", "fingertips_pos"):
        lo, hi = cols[name]
        err = (o[:, lo:hi] - want[name]).abs()
        print(f"N={N} {name}: max err {float(err.max()):.3e}")
        assert bool((err <= FLOAT_TOL * want[name].abs().clamp_min(1.0)).all()), (N, name, float(err.max()))
    lo, hi = cols["ee_quat"]  # (a real part within rounding of zero may come out on either side: the sign of the whole quaternion is then open)
    q = o[:, lo:hi]
    open_sign = ref["ee_quat"][:, 0].abs() < 1.0e-6
    err = torch.minimum((q - want["ee_quat"]).abs().amax(-1), torch.where(open_sign, (q + want["ee_quat"]).abs().amax(-1), torch.full((N,), 1.0e9, dtype=torch.float64)))
    assert float(err.max()) <= FLOAT_TOL and bool((q[:, 0] >= 0).all())
    reset = env.reset_buf.cpu()
    lo, hi = cols["actions"]
    assert_close(o[:, lo:hi][~reset].float(), action.cpu()[~reset], FLOAT_TOL, "last_action")
    if N >= 64:  # every branch was taken
        assert all(v > 0 for k, v in c.items() if not k.startswith("min_")), c
    # env.scene[...] serves what the fused ops used
    ee, cab = env.scene["ee_frame"].data, env.scene["cabinet_frame"].data
    torch.cuda.synchronize()
    assert ee.target_frame_names == ["ee_tcp", "tool_leftfinger", "tool_rightfinger"] and cab.target_frame_names == ["drawer_handle_top"]
    lo, hi = cols["rel_ee_drawer_distance"]
    assert torch.equal((cab.target_pos_w[:, 0] - ee.target_pos_w[:, 0]), obs["policy"][:, lo:hi])
    lo, hi = cols["fingertips_pos"]
    assert torch.equal((ee.target_pos_w[:, 1:] - feed["env_origins"].unsqueeze(1)).reshape(N, -1), obs["policy"][:, lo:hi])
    lo, hi = cols["ee_quat"]
    assert torch.equal(co.quat_unique(ee.target_quat_w[:, 0]), obs["policy"][:, lo:hi])
    cabinet = env.scene["cabinet"]
    assert cabinet.joint_names == cc.CABINET_JOINTS and cabinet.body_names == cc.CABINET_BODIES
    d = cabinet.data
    assert torch.equal(d.joint_pos, feed["articulation_joint_pos"]) and torch.equal(d.body_quat_w, feed["articulation_body_quat_w"])
    lo, hi = cols["cabinet_joint_pos"]
    assert torch.equal((d.joint_pos - d.default_joint_pos)[:, 3:4], obs["policy"][:, lo:hi])
    lo, hi = cols["cabinet_joint_vel"]
    assert torch.equal((d.joint_vel - d.default_joint_vel)[:, 3:4], obs["policy"][:, lo:hi])
    # the sensor is refreshed lazily, at most once per env step: no further launch within this step, one after the next step
    sensor = env.scene["ee_frame"]._sensor
    launches, update = [], sensor.update
    sensor.update = lambda *a: (launches.append(1), update(*a))[1]
    before = ee.target_pos_w.clone()
    assert env.scene["ee_frame"].data is ee and env.scene["ee_frame"].data is ee and launches == []
    env.step(action)
    assert launches == []  # (nobody asked: a step alone launches nothing)
    after = env.scene["ee_frame"].data.target_pos_w
    assert env.scene["ee_frame"].data.target_pos_w is after and launches == [1]
    torch.cuda.synchronize()
    want_tcp = co.frame_transformer(scene[2], feed["body_pos_w"].double().cpu(), feed["body_quat_w"].double().cpu())["target_pos_w"]
    assert float((after.double().cpu() - want_tcp).abs().max()) <= FLOAT_TOL * float(want_tcp.abs().max().clamp_min(1.0))
    assert not torch.equal(after, before)  # the feed moved to its next snapshot: other body poses
    env.close()


# ------------------------------------------------------------------------------------------------ k_frame_transformer
@pytest.mark.parametrize("case", cc.FT_CASES)
def test_frame_transformer_kernel_matches_the_fixture(case):
    from isaaclab_amd.producers import FrameTransformer
    from isaaclab_amd.robots import Frame, FrameTable

    fg = cc.FrameGolden()
    src, tg = fg.sensor(case)
    mk = lambda i, f: Frame(f"f{i}", 0, f"b{f[0]}", f[0], f[1], f[2])  # noqa: E731
    table = FrameTable(case, 0, mk(0, src), [mk(1 + i, f) for i, f in enumerate(tg)])
    bp, bq = (x.cuda() for x in fg.bodies(case))
    ft = FrameTransformer(table, None, bp.shape[0], "cuda:0")
    d = ft.update(bp, bq)
    torch.cuda.synchronize()
    ref = fg.expected(case)
    for k in cc.FT_OUTPUTS:
        assert_close(getattr(d, k).cpu(), ref[k], FLOAT_TOL, f"{case} {k}")


@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("source_offset", [False, True])
def test_frame_transformer_kernel_against_fp64(N, T, source_offset):
    """Random body poses around the origin (|x| < 4: fp32 rounds at 2.4e-7), random offsets with rotated ones; a sentinel row behind
    every output stays untouched."""
    from isaaclab_amd.producers import FrameTransformer
    from isaaclab_amd.robots import Frame, FrameTable

    g = torch.Generator().manual_seed(100 * N + 10 * T + int(source_offset))
    B = 7
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, 4, generator=g), dim=-1)  # noqa: E731
    frames = []
    for i in range(1 + T):
        ident = i == 0 and not source_offset
        pos = (0.0, 0.0, 0.0) if ident else tuple(float(x) for x in torch.randn(3, generator=g) * 0.2)
        rot = (1.0, 0.0, 0.0, 0.0) if ident or i == 1 else tuple(float(x) for x in unit())
        frames.append(Frame(f"f{i}", 0, "b", int(torch.randint(0, B, (1,), generator=g)), pos, rot))
    table = FrameTable("sensor", 0, frames[0], frames[1:])
    bp, bq = torch.randn(N, B, 3, generator=g).cuda(), unit(N, B).cuda()
    ft = FrameTransformer(table, None, N, "cuda:0")
    pads = {}
    for k in cc.FT_OUTPUTS:  # every output becomes the first N rows of a buffer one row longer: the row behind holds a sentinel
        pads[k] = torch.full((N + 1, *getattr(ft.data, k).shape[1:]), SENTINEL, device="cuda:0")
        setattr(ft.data, k, pads[k][:N])
    d = ft.update(bp, bq)
    torch.cuda.synchronize()
    for k in cc.FT_OUTPUTS:
        assert bool((pads[k][N] == SENTINEL).all()), f"{k}: the row behind the output was written"
        assert bool((pads[k][:N] != SENTINEL).all()), f"{k}: an element was not written"
    ref = co.frame_transformer(co.frames_of(table), bp.double().cpu(), bq.double().cpu())
    for k in cc.FT_OUTPUTS:
        err = (getattr(d, k).double().cpu() - ref[k]).abs().max()
        assert float(err) <= FLOAT_TOL, (k, float(err))
    assert d.target_pos_w.shape == (N, T, 3) and d.target_quat_source.shape == (N, T, 4) and d.source_quat_w.shape == (N, 4)
    with pytest.raises(ValueError, match="body_pos_w / body_quat_w must be"):
        ft.update(bp[:, :, :2], bq)


# ------------------------------------------------------------------------------------------------ captured = eager, learning
def _rollouts(use_graph):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    fx = cc.load_fixture()
    torch.manual_seed(29)
    feed = _feed(64, 29, snapshots=4)  # (a captured rollout walks the snapshots once per graph)
    u = ManagerBasedRLEnv(fx, state_feed=feed, seed=29, noise_seed=29)
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    assert runner._fusable()  # (the task's agent cfg has empirical_normalization=False: the fused three-launch rollout)
    # time-outs (the task's only termination) inside the recorded rollout: it is the third of four steps each, and these envs' tenth step
    u.episode_length_buf[::5] = int(u.max_episode_length) - 10
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    out = {k: getattr(st, k).cpu() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    out["processed"] = u._processed_action.cpu()
    env.close()
    return out


def test_cabinet_captured_rollout_equals_eager():
    a, c = _rollouts(True), _rollouts(False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert float(a["dones"].sum()) > 0 and float(a["rewards"].abs().sum()) > 0
    assert a["observations"].shape == (4, 64, cc.D) and a["actions"].shape == (4, 64, cc.A) and a["processed"].shape == (64, cc.PA)


def test_cabinet_runner_learns_one_iteration():
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    fx = cc.load_fixture()
    torch.manual_seed(3)
    u = ManagerBasedRLEnv(fx, state_feed=_feed(64, 3, snapshots=4), seed=3, noise_seed=3)
    runner = OnPolicyRunner(RslRlVecEnvWrapper(u), dict(fx["agent"], num_steps_per_env=8), log_dir=None, device="cuda:0")
    before = [p.detach().clone() for p in runner.alg.policy.parameters()]
    runner.learn(1)
    torch.cuda.synchronize()
    after = list(runner.alg.policy.parameters())
    assert all(torch.isfinite(p).all() for p in after) and any(not torch.equal(a, b) for a, b in zip(after, before))
    u.close()


# ------------------------------------------------------------------------------------------------ refusals at the launch checks
@pytest.mark.parametrize("missing", ["joint_pos", "joint_vel", "body_pos_w", "body_quat_w"])
def test_missing_tensor_of_the_second_articulation_is_refused_with_its_name_not_a_fault(missing):
    """Host-side validation only: the launch checks name the tensor and no kernel goes out with a NULL pointer."""
    from isaaclab_amd._lib import ImxError
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA_CABINET
    from isaaclab_amd.state_feed import StateFeed

    full = _feed(33, 2)
    name = "articulation_" + missing
    bare = StateFeed.from_tensors(FRANKA_PANDA_CABINET, [{n: v for n, v in full.snapshot(k).items() if n != name} for k in range(2)], device="cuda:0")
    assert name not in bare.names()
    fx = cc.load_fixture()
    env = ManagerBasedRLEnv(fx, state_feed=bare)
    with pytest.raises(ImxError, match=f"'articulation_state.{missing}' is required by an observation term"):
        env.reset()  # the observation launch check
    env.close()
    if missing == "joint_vel":  # read by an observation only
        return
    pol = fx["env"]["observations"]["policy"]  # without the observation terms that read it the step check names it
    del pol["cabinet_joint_pos"], pol["cabinet_joint_vel"], pol["rel_ee_drawer_distance"]
    env = ManagerBasedRLEnv(fx, state_feed=bare)
    env.reset()
    before = env._counters.clone()
    with pytest.raises(ImxError, match=f"'articulation_state.{missing}' is required by a term"):
        env.step(torch.zeros(33, cc.A, device="cuda:0"))
    torch.cuda.synchronize()
    assert torch.equal(env._counters, before)  # no launch went out: the step counter did not move
    env.close()


def test_mixed_plans_are_refused_by_the_step_launch():
    """A cabinet op beside a reach op: refused with a message by imx_terminations_rewards, before any launch."""
    from isaaclab_amd._lib import ImxError
    from isaaclab_amd.env import ManagerBasedRLEnv

    fx = cc.load_fixture()
    fx["env"]["commands"] = {"ee_pose": {"class_type": "isaaclab.envs.mdp.commands.pose_command:UniformPoseCommand", "body_name": "panda_hand"}}
    fx["env"]["rewards"]["tracking"] = {"func": "isaaclab_tasks.manager_based.manipulation.reach.mdp.rewards:position_command_error", "weight": -0.2,
                                        "params": {"asset_cfg": {"name": "robot", "body_names": ["panda_hand"]}, "command_name": "ee_pose"}}
    fx["robot"] = "franka_panda"  # (the feed then serves the 7-wide pose command)
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(FRANKA_PANDA, 16, "cuda:0", seed=1, num_snapshots=2))
    env.reset()
    with pytest.raises(ImxError, match="cabinet .* ops beside classic/humanoid, reach, lift, navigation or in-hand ops is not supported"):
        env.step(torch.zeros(16, cc.A, device="cuda:0"))
    env.close()
