"""GPU: Isaac-Lift-Cube-Franka-v0 on the fused HIP path -- the golden of the REAL reference managers (binary gripper action, the
manipulation/lift/mdp terms, root_height_below_minimum on the object), a per-op sweep against the fp64 statements of
tests/_lift_cases.py with every branch taken, the gripper's edge actions through both action paths (k_action and the actor head of the
fused rollout), a captured against an eager rollout with the env's own pose command, and the refusal of a missing object tensor."""

import numpy as np
import pytest
import torch

import _lift_cases as lc
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu

NAMES = ("root_pos_w", "root_quat_w", "command", "body_pos_w", "body_quat_w", "object_root_pos_w")


def _hand():
    from isaaclab_amd.robots import FRANKA_PANDA

    return FRANKA_PANDA.body_names.index(lc.EE_BODY)


def _gripper_targets(a):
    """where(a < 0, close 0.0, open 0.04) (binary_joint_actions.py:118-133)"""
    return torch.where(a < 0, torch.zeros_like(a), torch.full_like(a, float(np.float32(0.04))))


# ------------------------------------------------------------------------------------------------ the reference golden
@pytest.mark.parametrize("tail", ["deferred", "in_kernel"])
def test_lift_env_step_matches_reference_golden(tail):
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = lc.golden()
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"))
    p = env.plan
    assert p.n_ext_rew == 0 and p.n_ext_term == 0 and p.n_ext_obs == 0 and (p.action_dim, p.processed_action_dim, p.obs_dim) == (lc.A, lc.PA, lc.D)
    env.defer_step_tail = tail == "deferred"
    env._noise_u = torch.zeros(g.N, g.meta["obs_dim"], device="cuda:0")
    env._noise_u.copy_(g.t("reset/noise_u"))
    obs_dict, _ = env.reset()
    torch.cuda.synchronize()
    assert_close(obs_dict["policy"].cpu(), g.t("reset/obs"), FLOAT_TOL, "reset obs")
    env.episode_length_buf = g.t("reset/episode_length_buf")
    names_r = g.meta["reward_terms"]
    grip, arm = env.action_manager.get_term("gripper_action"), env.action_manager.get_term("arm_action")
    assert grip.raw_actions.shape == (g.N, 1) and grip.processed_actions.shape == (g.N, 2)
    assert arm.raw_actions.shape == (g.N, 7) and arm.processed_actions.shape == (g.N, 7)
    assert env.action_manager.action_term_dim == [7, 1] and env.action_manager.total_action_dim == 8
    for k in range(g.steps):
        tag = f"step{k}"
        env._noise_u.copy_(g.t(f"{tag}/noise_u"))
        obs_dict, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").cuda())
        torch.cuda.synchronize()
        # exact: masks, reset ids, episode lengths, the lifted values, the raw gripper column, the two processed gripper columns
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")), "terminated"
        assert torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs")), "time_outs"
        assert torch.equal(env.reset_buf.cpu(), g.t(f"{tag}/reset_buf")), "reset_buf"
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids")), "reset_env_ids"
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf")), "episode_length_buf"
        for name in g.meta["termination_terms"]:
            assert torch.equal(env.termination_manager.get_term(name).cpu(), g.t(f"{tag}/term_dones/{name}")), name
        sr = env.reward_manager._step_reward.cpu()
        assert torch.equal(sr[:, 1], g.t(f"{tag}/step_reward")[:, 1]), "object_is_lifted"
        assert torch.equal(grip.raw_actions.cpu(), g.t(f"{tag}/action_after_reset")[:, 7:8]), "raw gripper action (zeroed where the env was reset)"
        assert torch.equal(grip.processed_actions.cpu(), g.t(f"{tag}/processed_actions")[:, 7:9]), "processed gripper actions"
        assert torch.equal(grip.processed_actions.cpu(), _gripper_targets(g.t(f"{tag}/action")[:, 7:8]).expand(g.N, 2))
        # within FLOAT_TOL: everything that goes through fp32 arithmetic
        assert_close(env._processed_action, g.t(f"{tag}/processed_actions"), FLOAT_TOL, f"{tag} processed_actions")
        assert_close(env.action_manager.action, g.t(f"{tag}/action_after_reset"), FLOAT_TOL, f"{tag} action")
        assert_close(env.action_manager.prev_action, g.t(f"{tag}/prev_action_after_reset"), FLOAT_TOL, f"{tag} prev_action")
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(sr, g.t(f"{tag}/step_reward"), FLOAT_TOL, f"{tag} step_reward")
        for name in names_r:
            assert_close(env.reward_manager._episode_sums[name], g.t(f"{tag}/episode_sums/{name}"), FLOAT_TOL, f"{tag} {name}")
        assert_close(obs_dict["policy"].cpu(), g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        for key, v in g.log(k).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (key, got, v)
    assert sum(int(g.t(f"step{k}/term_dones/object_dropping").sum()) for k in range(g.steps)) > 0
    assert sum(int(g.t(f"step{k}/time_outs").sum()) for k in range(g.steps)) > 0
    env.close()


# ------------------------------------------------------------------------------------------------ per-op sweep against fp64
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 257])
def test_lift_ops_against_fp64_formulas(N):
    """The lift terms after one step against the fp64 statements on the same fp32 inputs, at the 16-env item groups and 64-lane waves of
    the step kernel, one past each, and a ragged multi-workgroup grid.  Tolerances as in tests/test_lift_plan.py: FLOAT_TOL plus the
    world-coordinate rounding (over std for the tanh kernels); thresholds and the gripper targets exact."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    b = _hand()
    fx = lc.load_fixture()
    fx["env"]["observations"]["policy"]["enable_corruption"] = False
    fx["env"]["terminations"]["reached"] = {"func": f"{lc.LIFT}.terminations:object_reached_goal", "params": {"threshold": 0.06}, "time_out": False}
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=700 + N, num_snapshots=2)
    lc.lift_tweak(feed, b, torch.Generator().manual_seed(N))
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    env.reset()
    action = lc.gripper_edges(torch.randn(N, lc.A, generator=torch.Generator().manual_seed(7)) * 0.8).cuda()
    obs, _, _, _, _ = env.step(action)
    torch.cuda.synchronize()
    s = {n: feed[n] for n in NAMES}
    ref = lc.lift_terms(s, b)
    ulp = lc.position_rounding(s, b)
    sr = env.reward_manager._step_reward.double()
    for col, (key, w, extra) in enumerate((("object_ee_distance", 1.0, ulp / lc.STD_EE), ("object_is_lifted", 15.0, 0.0),
                                           ("object_goal_distance", 16.0, ulp / lc.STD_GOAL), ("object_goal_distance_fine", 5.0, ulp / lc.STD_GOAL_FINE))):
        got, val = sr[:, col] / w, ref[key]
        err = (got - val).abs()
        print(f"N={N} {key}: max err {float(err.max()):.3e}, max allowance {float((FLOAT_TOL * val.abs().clamp_min(1.0) + extra).max()):.3e}")
        assert bool((err <= FLOAT_TOL * val.abs().clamp_min(1.0) + extra).all()), (N, key, float(err.max()))
    assert torch.equal((sr[:, 1] > 7.5).double(), ref["object_is_lifted"]), "object_is_lifted"
    assert torch.equal(env.termination_manager.get_term("object_dropping"), ref["object_dropping"]), "object_dropping"
    # object_reached_goal: distance < f32(threshold); envs whose fp64 distance is within the rounding allowance of it may fall either side
    th = lc.f32(0.06)
    got_reached, d_goal = env.termination_manager.get_term("reached"), ref["goal_distance"]
    clear = (d_goal - th).abs() > FLOAT_TOL + ulp
    assert torch.equal(got_reached[clear], (d_goal < th)[clear]), "object_reached_goal"
    err = (obs["policy"][:, 18:21].double() - ref["object_position"]).abs()
    print(f"N={N} object_position: max err {float(err.max()):.3e}")
    assert bool((err <= FLOAT_TOL * ref["object_position"].abs().clamp_min(1.0) + ulp[:, None]).all()), (N, float(err.max()))
    assert torch.equal(obs["policy"][:, 21:28], s["command"])
    # the gripper: both finger targets from the one action column, exactly; the arm's seven columns stay where they were
    grip = env.action_manager.get_term("gripper_action")
    assert torch.equal(grip.processed_actions, _gripper_targets(action[:, 7:8]).expand(N, 2))
    arm = action[:, :7] * 0.5 + feed["default_joint_pos"][:, :7]
    assert_close(env.action_manager.get_term("arm_action").processed_actions, arm, FLOAT_TOL, "arm targets")
    if N >= 64:  # every branch was taken
        c = lc.branch_counts([s], b, [action])
        assert c.pop("gripper_nan") == 0 and all(v > 0 for v in c.values()), c
        assert bool(got_reached.any()) and not bool(got_reached.all())
    env.close()


# ------------------------------------------------------------------------------------------------ both action paths
@pytest.mark.parametrize("clip", [None, 1.0e-30, float(np.float32(1.0e-45)), 0.0])
def test_gripper_edge_actions_agree_between_k_action_and_the_actor_head(clip):
    """A 4-step rollout at N = 257, split (imx_policy_act, then env.step -> k_action) against fused (the actor head of k_mlp_infer calls
    the same action element).  The wrapper's action clamp forces the sampled action onto the edge values in both: +-1e-30, the smallest
    subnormals of either sign, +-0.0; without a clamp the ordinary +- values.  action, prev_action, processed_action and the storage must
    be identical, and the gripper targets what where(a < 0, close, open) says."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    fx = lc.load_fixture()
    out = {}
    for fuse in (False, True):
        torch.manual_seed(3)
        feed = StateFeed(FRANKA_PANDA, 257, "cuda:0", seed=5, num_snapshots=4)
        lc.lift_tweak(feed, _hand(), torch.Generator().manual_seed(5))
        env = ManagerBasedRLEnv(fx, state_feed=feed, noise_seed=11)
        venv = RslRlVecEnvWrapper(env, clip_actions=clip)
        runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=True)
        runner.fuse_launches = fuse
        runner.train_mode()
        assert runner._fusable()
        for _ in range(2):
            runner.collect()
        torch.cuda.synchronize()
        st = runner.alg.storage
        out[fuse] = {k: getattr(st, k).cpu() for k in ("observations", "actions", "actions_log_prob", "mu", "sigma", "values", "rewards", "dones")}
        out[fuse].update(action=env._action.cpu(), prev_action=env._prev_action.cpu(), processed=env._processed_action.cpu(),
                         reset=env.reset_buf.cpu())  # (compared on the host: its arithmetic keeps subnormals)
        env.close()
    a, b = out[False], out[True]
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: fused and split rollouts differ"
    assert a["processed"].shape == (257, lc.PA) and a["action"].shape == (257, lc.A)
    keep = ~a["reset"]  # (a reset env's raw action is zeroed, its targets stay)
    raw = a["action"][keep][:, 7:8]
    assert torch.equal(a["processed"][keep][:, 7:9], _gripper_targets(raw).expand(int(keep.sum()), 2))
    sampled = a["actions"][-1][keep][:, 7]  # what the policy drew at the last step, before the clamp
    assert bool((sampled < 0).any()) and bool((sampled > 0).any())
    if clip is None:
        assert torch.equal(raw[:, 0], sampled)
    else:
        assert bool((raw.abs() <= clip).all())
        if clip > 0.0:  # the clamp leaves the edge value of the drawn sign: negative closes, positive opens
            assert torch.equal(raw[:, 0], torch.where(sampled < 0, -torch.ones_like(sampled), torch.ones_like(sampled)) * clip)
            assert bool((a["processed"][keep][:, 7] == 0).any()) and bool((a["processed"][keep][:, 7] > 0).any())
        else:  # +-0.0 never closes
            assert bool((a["processed"][keep][:, 7:9] == float(np.float32(0.04))).all())


# ------------------------------------------------------------------------------------------------ captured = eager, own pose command
def _rollouts(use_graph):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.producers import UniformPoseCommand
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    fx = lc.load_fixture()
    torch.manual_seed(17)
    feed = StateFeed(FRANKA_PANDA, 512, "cuda:0", seed=17, num_snapshots=4)
    lc.lift_tweak(feed, _hand(), torch.Generator().manual_seed(17))
    u = ManagerBasedRLEnv(fx, state_feed=feed, seed=17, noise_seed=17, command_term="object_pose")
    assert isinstance(u.command_term, UniformPoseCommand) and u.command_term.body_name == "panda_hand"
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=8), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    u.episode_length_buf[::5] = int(u.max_episode_length) - 10  # time-outs inside the recorded rollout
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    res.update(command=u.command_term.command.clone(), processed=u._processed_action.clone())
    runner.learn(1)
    torch.cuda.synchronize()
    res["params"] = runner.alg.bucket.flat.clone()
    out = {k: v.cpu() for k, v in res.items()}
    env.close()
    return out


def test_lift_captured_rollout_equals_eager_with_its_own_pose_command():
    a, c = _rollouts(True), _rollouts(False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert float(a["dones"].sum()) > 0 and float(a["rewards"].abs().sum()) > 0
    assert a["observations"].shape == (8, 512, lc.D) and a["actions"].shape == (8, 512, lc.A)
    cmd = a["command"]  # the env's own object_pose term, in the ranges of the cfg
    assert bool(((cmd[:, 0] >= 0.4) & (cmd[:, 0] <= 0.6) & (cmd[:, 2] >= 0.25) & (cmd[:, 2] <= 0.5)).all())


# ------------------------------------------------------------------------------------------------ refusals at the launch checks
def test_missing_object_tensor_is_refused_with_a_message_not_a_fault():
    from isaaclab_amd._lib import ImxError
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import DYNAMIC, EXTRA, STATIC, StateFeed

    full = StateFeed(FRANKA_PANDA, 33, "cuda:0", seed=2, num_snapshots=2)
    snaps = [{n: v for n, v in full.snapshot(k).items() if n in DYNAMIC + EXTRA + STATIC and n != "object_root_pos_w"} for k in range(2)]
    bare = StateFeed.from_tensors(FRANKA_PANDA, snaps, device="cuda:0")
    assert "object_root_pos_w" not in bare.names()
    fx = lc.load_fixture()
    env = ManagerBasedRLEnv(fx, state_feed=bare)
    with pytest.raises(ImxError, match="'object_root_pos_w' is required by an observation term"):
        env.reset()  # the observation launch check
    env.close()
    del fx["env"]["observations"]["policy"]["object_position"]
    env = ManagerBasedRLEnv(fx, state_feed=bare)
    env.reset()
    before = env._counters.clone()
    with pytest.raises(ImxError, match="'object_root_pos_w' is required by a term"):
        env.step(torch.zeros(33, lc.A, device="cuda:0"))  # the step launch check
    torch.cuda.synchronize()
    assert torch.equal(env._counters, before)  # no launch went out: the step counter did not move
    env.close()


def test_actuator_needs_one_target_per_joint():
    from isaaclab_amd.env import ManagerBasedRLEnv

    env = ManagerBasedRLEnv("Isaac-Cartpole-v0", num_envs=8)  # one effort column, two joints
    with pytest.raises(ValueError, match="1 joint targets, the robot has 2 joints"):
        env.attach_actuator(object())
    env.close()


# ------------------------------------------------------------------------------------------------ the actor head on 32-row tiles
@pytest.mark.parametrize("packed", [True, False])
def test_binary_head_of_the_shared_input_launch_on_32_row_tiles(packed):
    """The rollouts above run 257 envs (16-row tiles): ``k_mlp_infer_binary`` at 2081 rows, packed and row-layout weights, against
    ``imx_mlp_infer`` + ``imx_policy_act`` + the action terms."""
    from test_infer_two_inputs_gpu import binary_head_on_32_row_tiles

    binary_head_on_32_row_tiles("shared", packed)
