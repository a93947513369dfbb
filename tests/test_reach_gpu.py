"""GPU: Isaac-Reach-Franka-v0 and Isaac-Reach-UR10-v0 on the fused HIP path -- the golden of the REAL reference managers with the
manipulation/reach/mdp rewards, a per-op sweep against fp64 statements of the formulas (tests/_reach_cases.py) with every branch taken,
the fused rollout against the split one, a 4096-env training iteration per task, and both policy shapes through the minibatch-gradient
check at the batch size the tasks train with."""

import numpy as np
import pytest
import torch

from _reach_cases import TASKS, position_rounding, reach_terms, reach_tweak
from _util import FLOAT_TOL, Golden, assert_close, check_minibatch_gradients, fill_storage

pytestmark = pytest.mark.gpu


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the reference golden
@pytest.mark.parametrize("tail", ["deferred", "in_kernel"])
@pytest.mark.parametrize("task", list(TASKS))
def test_reach_env_step_matches_reference_golden(task, tail):
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = Golden(task)
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"))
    assert env.plan.n_ext_rew == 0 and env.plan.n_ext_term == 0 and env.plan.n_ext_obs == 0 and env.plan.cmd_dim == 7
    env.defer_step_tail = tail == "deferred"
    # parity mode: the uniforms of the reference's uniform_noise draws (joint_pos_rel, joint_vel_rel: +-0.01) replace the in-kernel RNG
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
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(env.reward_manager._step_reward, g.t(f"{tag}/step_reward"), FLOAT_TOL, f"{tag} step_reward")
        for name in names_r:
            assert_close(env.reward_manager._episode_sums[name], g.t(f"{tag}/episode_sums/{name}"), FLOAT_TOL, f"{tag} {name}")
        assert_close(obs_dict["policy"].cpu(), g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        for key, v in g.log(k).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (key, got, v)
    assert sum(int(g.t(f"step{k}/reset_buf").sum()) for k in range(g.steps)) > 0  # time-outs reset envs inside the replay
    env.close()


# ------------------------------------------------------------------------------------------------ per-op sweep against fp64
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4096, 100_003])
@pytest.mark.parametrize("task", list(TASKS))
def test_reach_ops_against_fp64_formulas(task, N):
    """The three reach rewards and the 7-wide command observation after one step, against fp64 statements of the formulas on the same
    fp32 inputs.  The position terms get the fp32 rounding allowance of world coordinates far from the origin (tests/_reach_cases.py:
    position_rounding), times 1 / std for the tanh kernel."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    robot_name, ee, D, A, pitch = TASKS[task]
    robot = ROBOTS[robot_name]
    b = robot.body_names.index(ee)
    fx = load_task_cfg(task)
    fx["env"]["observations"]["policy"]["enable_corruption"] = False  # the columns without their uniform noise
    feed = StateFeed(robot, N, "cuda:0", seed=900 + N, num_snapshots=2)
    reach_tweak(feed, b, pitch, torch.Generator().manual_seed(N))
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    assert env.plan.obs_dim == D
    env.reset()
    gen = torch.Generator().manual_seed(7)
    action = (torch.randn(N, A, generator=gen) * 0.8).cuda()
    obs, _, _, _, _ = env.step(action)
    torch.cuda.synchronize()
    s = {n: feed[n] for n in feed.names()}
    ref = reach_terms(s, b, 0.1)
    ulp_pos = position_rounding(s, b)
    extra = {"position_command_error": ulp_pos, "position_command_error_tanh": ulp_pos / 0.1}
    names = [t.func.rpartition(":")[2] for t in env.plan.reward_terms]
    for k, name in enumerate(names[:3]):
        w = env.plan.reward_terms[k].weight
        got = env.reward_manager._step_reward[:, k].double() / _f32(w)
        val = ref[name]
        tol = FLOAT_TOL * val.abs().clamp_min(1.0) + extra.get(name, 0.0)
        err = (got - val).abs()
        assert bool((err <= tol).all()), (task, N, name, float((err - tol).max()))
    # generated_commands: the 7 command columns, exactly (no noise, no scale)
    J = robot.num_joints
    assert torch.equal(obs["policy"][:, 2 * J:2 * J + 7], s["command"])
    if N >= 64:  # every branch was taken
        ori, pos = ref["orientation_command_error"], ref["position_command_error"]
        assert bool((ori < 1e-6).any()) and bool((ori > np.pi - 2e-3).any()) and bool((pos < 1e-6).any())
        assert bool(((pos > 0.099) & (pos < 0.101)).any())
        assert bool((s["body_quat_w"][:, b, 0] < 0).any()) and bool((s["command"][:, 3] < 0).any())
    env.close()


# ------------------------------------------------------------------------------------------------ fused rollout = split rollout
def test_three_launch_rollout_equals_six_launch_split_for_franka():
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    task = "Isaac-Reach-Franka-v0"
    robot_name, ee, _, _, pitch = TASKS[task]
    fx = load_task_cfg(task)
    out = {}
    for fuse in (False, True):
        torch.manual_seed(3)
        feed = StateFeed(ROBOTS[robot_name], 2500, "cuda:0", seed=5, num_snapshots=4)
        reach_tweak(feed, ROBOTS[robot_name].body_names.index(ee), pitch, torch.Generator().manual_seed(5))
        env = ManagerBasedRLEnv(fx, state_feed=feed, noise_seed=11)
        venv = RslRlVecEnvWrapper(env)
        runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=True)
        runner.fuse_launches = fuse
        runner.train_mode()
        ep = torch.randint(0, int(venv.max_episode_length), (env.num_envs,), generator=torch.Generator().manual_seed(9))
        ep[::7] = int(venv.max_episode_length) - 2
        venv.episode_length_buf = ep.cuda()
        assert runner._fusable()
        for _ in range(2):
            runner.collect()
        torch.cuda.synchronize()
        st = runner.alg.storage
        out[fuse] = {k: getattr(st, k).clone() for k in ("observations", "actions", "actions_log_prob", "mu", "sigma", "values", "rewards", "dones")}
        out[fuse].update(action=env._action.clone(), ep_len=env.episode_length_buf.clone(), log_out=env._log_out.clone())
        env.close()
    a, b = out[False], out[True]
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: fused and split rollouts differ"
    assert float(a["dones"].sum()) > 0


# ------------------------------------------------------------------------------------------------ training at 4096 envs
def _train_once(task, seed, use_graph):
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    robot_name, ee, _, _, pitch = TASKS[task]
    fx = load_task_cfg(task)
    torch.manual_seed(seed)
    feed = StateFeed(ROBOTS[robot_name], 4096, "cuda:0", seed=seed, num_snapshots=4)
    reach_tweak(feed, ROBOTS[robot_name].body_names.index(ee), pitch, torch.Generator().manual_seed(seed))
    env = RslRlVecEnvWrapper(ManagerBasedRLEnv(fx, state_feed=feed, seed=seed, noise_seed=seed))
    u = env.unwrapped
    agent = fx["agent"]
    assert (agent["algorithm"]["num_learning_epochs"], agent["algorithm"]["num_mini_batches"]) == (8, 4)
    runner = OnPolicyRunner(env, dict(agent, num_steps_per_env=8), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    u.episode_length_buf[::5] = int(u.max_episode_length) - 20  # time-outs inside the recorded rollout
    for _ in range(2 if use_graph else 3):
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    runner.learn(1)
    torch.cuda.synchronize()
    res["params"] = runner.alg.bucket.flat.clone()
    out = {k: v.cpu() for k, v in res.items()}
    env.close()
    return out


@pytest.mark.parametrize("task", list(TASKS))
def test_reach_4096_training_graph_equals_eager_and_reproduces(task):
    a = _train_once(task, 17, True)
    b = _train_once(task, 17, True)
    c = _train_once(task, 17, False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), f"{k}: not reproducible"
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert float(a["dones"].sum()) > 0 and float(a["rewards"].abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ policy shapes at the training batch
@pytest.mark.parametrize("task", list(TASKS))
def test_update_gradient_at_reach_shapes(monkeypatch, task):
    """[64, 64] ELU actor and critic at the tasks' D and A, M = 4096 envs x 24 steps / 4 minibatches = 24 576 rows, through the storage's
    own permutation and gather, against fp64 autograd (tests/_util.py tolerance rule)."""
    import isaaclab_amd.rsl_rl.ppo as ppo_mod
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    robot_name, _, D, A, _ = TASKS[task]
    fx = load_task_cfg(task)
    plan = compile_plan(fx["env"], ROBOTS[robot_name])
    assert (plan.obs_dim, plan.action_dim) == (D, A)
    agent = fx["agent"]
    T, nmb = int(agent["num_steps_per_env"]), int(agent["algorithm"]["num_mini_batches"])
    assert (T, nmb) == (24, 4)
    torch.manual_seed(0)
    pol = ActorCritic(D, D, A, actor_hidden_dims=agent["policy"]["actor_hidden_dims"], critic_hidden_dims=agent["policy"]["critic_hidden_dims"],
                      activation=agent["policy"]["activation"], init_noise_std=agent["policy"]["init_noise_std"],
                      noise_std_type=agent["policy"]["noise_std_type"])
    alg = PPO(pol, device="cuda:0", **{k: v for k, v in agent["algorithm"].items() if k != "class_name"})
    alg.init_storage("rl", 4096, T, (D,), (0,), (A,))
    fill_storage(alg, 1)
    torch.manual_seed(1)
    alg.storage.draw_permutation(nmb)
    batch = alg.storage.gather_minibatch(0, nmb)
    assert batch[0].shape[0] == 24_576
    for two_streams in (True, False):
        monkeypatch.setattr(ppo_mod, "FUSED_HEAD", "0")
        alg.two_streams = two_streams
        check_minibatch_gradients(alg, batch, f"{task} two_streams={two_streams}")


# ------------------------------------------------------------------------------------------------ where the command comes from
def test_pose_command_width_is_checked_at_construction():
    """The Reach command comes from the state feed: a feed whose command is not 7 wide is refused before any launch could read past its
    rows, and so is ``use_command_term=True`` (the env's own command term is a UniformVelocityCommand; a pose command has no producer)."""
    import dataclasses

    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg("Isaac-Reach-Franka-v0")
    narrow = StateFeed(dataclasses.replace(FRANKA_PANDA, command_dim=3), 16, "cuda:0", seed=1, num_snapshots=2)
    with pytest.raises(ValueError, match="3 wide, the plan's 7"):
        ManagerBasedRLEnv(fx, state_feed=narrow)
    feed = StateFeed(FRANKA_PANDA, 16, "cuda:0", seed=1, num_snapshots=2)
    with pytest.raises(NotImplementedError, match="UniformPoseCommand"):
        ManagerBasedRLEnv(fx, state_feed=feed, use_command_term=True)
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    assert env.command_manager.get_command("ee_pose").shape == (16, 7)
    env.close()
