"""GPU: Isaac-Ant-v0 and Isaac-Humanoid-v0 on the fused HIP path -- the golden of the REAL reference managers with the classic/humanoid/mdp
terms (progress_reward's potentials bit for bit), a per-op sweep against fp64 statements of the formulas, the potentials across env.reset()
and steps against their fp32 formula, the fused rollout against the split one, a 4096-env training iteration per task, and both policy
shapes through the minibatch-gradient check at the batch size the tasks train with."""

import math

import numpy as np
import pytest
import torch

from _util import FLOAT_TOL, Golden, assert_close, check_minibatch_gradients, fill_storage

pytestmark = pytest.mark.gpu

TASKS = ("Isaac-Ant-v0", "Isaac-Humanoid-v0")
ANGLE_COLS = (7, 8, 9)  # base_yaw_roll (yaw, roll), base_angle_to_target: atan2 of a wrapped angle, compared modulo 2 pi


def _f32(x):
    return float(np.float32(x))


def assert_close_angles(a, b, tol, what):
    """|wrap(a - b)| <= tol: near +-pi one ulp of sin / cos / atan2 flips the sign of the reference's atan2(sin, cos) (a known deviation)."""
    d = (a.double().cpu() - b.double().cpu() + math.pi) % (2 * math.pi) - math.pi
    assert bool((d.abs() <= tol).all()), f"{what}: max wrapped err {float(d.abs().max()):.3e}"


def assert_obs_close(got, ref, what):
    cols = [c for c in range(ref.shape[1]) if c not in ANGLE_COLS]
    assert_close(got[:, cols], ref[:, cols], FLOAT_TOL, what)
    assert_close_angles(got[:, list(ANGLE_COLS)], ref[:, list(ANGLE_COLS)], FLOAT_TOL, what + " angles")


# ------------------------------------------------------------------------------------------------ the reference golden
@pytest.mark.parametrize("tail", ["deferred", "in_kernel"])
@pytest.mark.parametrize("task", TASKS)
def test_classic_env_step_matches_reference_golden(task, tail):
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = Golden(task)
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"))
    assert env.plan.n_ext_rew == 0 and env.plan.n_ext_term == 0 and env.plan.n_ext_obs == 0
    env.defer_step_tail = tail == "deferred"
    obs_dict, _ = env.reset()
    torch.cuda.synchronize()
    assert torch.equal(env._term_state[0].cpu(), g.t("reset/potentials")), "potentials after reset()"
    assert_obs_close(obs_dict["policy"].cpu(), g.t("reset/obs"), "reset obs")
    env.episode_length_buf = g.t("reset/episode_length_buf")
    names_r, names_t = g.meta["reward_terms"], g.meta["termination_terms"]
    for k in range(g.steps):
        tag = f"step{k}"
        obs_dict, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").cuda())
        torch.cuda.synchronize()
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")), "terminated"
        assert torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs")), "time_outs"
        assert torch.equal(env.reset_buf.cpu(), g.t(f"{tag}/reset_buf")), "reset_buf"
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids")), "reset_env_ids"
        for name in names_t:
            assert torch.equal(env.termination_manager.get_term(name).cpu(), g.t(f"{tag}/term_dones/{name}")), name
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf")), "episode_length_buf"
        assert torch.equal(env._term_state[0].cpu(), g.t(f"{tag}/potentials")), f"{tag} potentials"
        # progress = potentials - prev_potentials of identical fp32 numbers: exact
        k_prog = names_r.index("progress")
        assert torch.equal(env.reward_manager._step_reward[:, k_prog].cpu(), g.t(f"{tag}/step_reward")[:, k_prog]), f"{tag} progress"
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(env.reward_manager._step_reward, g.t(f"{tag}/step_reward"), FLOAT_TOL, f"{tag} step_reward")
        for name in names_r:
            assert_close(env.reward_manager._episode_sums[name], g.t(f"{tag}/episode_sums/{name}"), FLOAT_TOL, f"{tag} {name}")
        assert_obs_close(obs_dict["policy"].cpu(), g.t(f"{tag}/obs"), f"{tag} obs")
        for key, v in g.log(k).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (key, got, v)
    env.close()


# ------------------------------------------------------------------------------------------------ per-op sweep against fp64
def _qri(q, v):
    w, xyz = q[:, :1], q[:, 1:]
    return v * (2.0 * w * w - 1.0) - torch.cross(xyz, v, dim=-1) * w * 2.0 + xyz * (xyz * v).sum(-1, keepdim=True) * 2.0


def _tweak(feed, gen):
    """Tilts past the upright threshold, yaw / roll at +-pi, low torsos (terminations) on a random feed."""
    from isaaclab_amd.state_feed import _quat_from_euler

    st, N = feed._stack, feed.num_envs
    idx = torch.arange(N)
    for k in range(feed.num_snapshots):
        roll = torch.randn(N, generator=gen) * 0.3
        pitch = torch.randn(N, generator=gen) * 0.3
        yaw = (torch.rand(N, generator=gen) * 2.0 - 1.0) * math.pi
        yaw[idx % 13 == 3] = math.pi - 1.0e-3
        roll[idx % 13 == 5] = -math.pi + 1.0e-3
        st["root_quat_w"][k].copy_(_quat_from_euler(roll, pitch, yaw))
        low = (idx % 7 == 2).to(st["root_pos_w"].device)
        st["root_pos_w"][k][low, 2] = 0.2


def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def _ref_obs(s, robot, fx, wrench_ids, action):
    """Every observation column in fp64 from the fp32 inputs (classic/humanoid/mdp/observations.py, envs/mdp/observations.py)."""
    d = lambda n: s[n].double()  # noqa: E731
    q = d("root_quat_w")
    w, x, y, z = q.unbind(-1)
    roll = torch.atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y))
    yaw = torch.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    pos = d("root_pos_w")
    t = torch.tensor([1000.0, 0.0, 0.0], dtype=torch.float64, device=q.device)
    to = t - pos
    walk = torch.atan2(to[:, 1], to[:, 0])
    to2 = to.clone()
    to2[:, 2] = 0.0
    u = to2 / to2.norm(dim=-1, keepdim=True).clamp_min(1e-9)
    head = torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z), 2.0 * (x * z - w * y)], dim=-1)  # R(q) (1, 0, 0)
    g = _qri(q, torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=q.device).expand_as(pos))
    lim = d("soft_joint_pos_limits")
    jpn = 2.0 * (d("joint_pos") - 0.5 * (lim[..., 0] + lim[..., 1])) / (lim[..., 1] - lim[..., 0])
    P = fx["env"]["observations"]["policy"]
    N = q.shape[0]
    cols = [pos[:, 2:3], _qri(q, d("root_lin_vel_w")), _qri(q, d("root_ang_vel_w")) * _f32(P["base_ang_vel"].get("scale") or 1.0),
            torch.stack([_wrap(yaw), _wrap(roll)], -1), _wrap(walk - yaw)[:, None], -g[:, 2:3], (head * u).sum(-1, keepdim=True), jpn,
            (d("joint_vel") - d("default_joint_vel")) * _f32(P["joint_vel_rel"]["scale"]),
            d("link_incoming_joint_force")[:, wrench_ids].reshape(N, -1) * _f32(P["feet_body_forces"]["scale"]), action.double()]
    return torch.cat(cols, dim=-1), g


def _potential(pos, dt, z_on):
    """progress_reward's potential in the reference's fp32 sequence (numpy: separately rounded squares, correctly rounded sqrt, IEEE
    division by fp32(step_dt))."""
    p = pos.cpu().numpy().astype(np.float32)
    dx, dy = np.float32(1000.0) - p[:, 0], np.float32(0.0) - p[:, 1]
    dz = (np.float32(0.0) - p[:, 2]) if z_on else np.zeros_like(dx)
    return torch.from_numpy(-np.sqrt((dx * dx + dy * dy) + dz * dz) / np.float32(dt))


@pytest.mark.parametrize("N", [1, 63, 4097, 100_003])
@pytest.mark.parametrize("task", TASKS)
def test_classic_ops_against_fp64_formulas(task, N):
    """Every reward term and every observation column after one step, against fp64 statements of the formulas on the same fp32 inputs.
    The wrench term reads an odd body list (three bodies, not in cfg order).  progress = potentials - prev_potentials cancels two ~6e4
    potentials (one ulp: 4e-3): it must equal the reference's fp32 sequence bit for bit, and its fp64 value may differ by the potentials'
    own fp32 rounding (a few ulp of |potential| each), which the tolerance adds per env."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg(task)
    robot = ROBOTS[fx["robot"]]
    odd = [robot.body_names[i] for i in (len(robot.body_names) - 1, 0, 3)]
    fx["env"]["observations"]["policy"]["feet_body_forces"]["params"]["asset_cfg"]["body_names"] = odd
    wrench_ids = sorted(robot.body_names.index(n) for n in odd)
    feed = StateFeed(robot, N, "cuda:0", seed=700 + N, num_snapshots=2)
    gen = torch.Generator().manual_seed(N)
    _tweak(feed, gen)
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    assert env.plan.obs_dim == 1 + 3 + 3 + 2 + 1 + 1 + 1 + 2 * robot.num_joints + 18 + robot.num_joints
    env.reset()
    pot0 = feed["root_pos_w"].clone()
    A = env.plan.action_dim
    action = (torch.randn(N, A, generator=gen) * 0.8).cuda()
    obs, _, terminated, _, _ = env.step(action)
    torch.cuda.synchronize()
    s = {n: feed[n] for n in feed.names()}
    reset = env.reset_buf.clone()
    ref_obs, g = _ref_obs(s, robot, fx, wrench_ids, torch.where(reset[:, None], torch.zeros_like(action), action))  # ActionManager.reset
    got = obs["policy"].cpu()
    assert_obs_close(got, ref_obs.cpu(), f"{task} N={N} obs")
    R = fx["env"]["rewards"]
    d = lambda n: s[n].double()  # noqa: E731
    pos = d("root_pos_w")
    dt = env.step_dt
    to = torch.tensor([1000.0, 0.0], dtype=torch.float64, device=pos.device) - pos[:, :2]
    cur64 = -to.norm(dim=-1) / _f32(dt)
    p0 = pot0.double()
    prev64 = -(torch.tensor([1000.0, 0.0, 0.0], dtype=torch.float64, device=pos.device) - p0).norm(dim=-1) / _f32(dt)
    up = -g[:, 2]
    head = ref_obs[:, 11]
    lim = d("soft_joint_pos_limits")
    s_abs = (2.0 * (d("joint_pos") - 0.5 * (lim[..., 0] + lim[..., 1])) / (lim[..., 1] - lim[..., 0])).abs()
    from isaaclab_amd import plan as pm

    rew_off = int(env.plan.blob[pm.H["REW_OFF"]])

    def table(k):
        r = env.plan.blob[rew_off + k * pm.REC_WORDS: rew_off + (k + 1) * pm.REC_WORDS]
        o, n = int(r[pm.R["IDS2_OFF"]]), int(r[pm.R["NIDS2"]])
        return torch.from_numpy(np.frombuffer(np.ascontiguousarray(env.plan.blob[o:o + n]).tobytes(), np.float32).astype(np.float64)).to(pos.device)

    names = [t.name for t in env.plan.reward_terms]
    th_l = _f32(R["joint_pos_limits"]["params"]["threshold"])
    ref = {
        "progress": cur64 - prev64,
        "alive": (~terminated).double(),
        "upright": (up > _f32(R["upright"]["params"]["threshold"])).double(),
        "move_to_target": torch.where(head > _f32(R["move_to_target"]["params"]["threshold"]), torch.ones_like(head),
                                      head / _f32(R["move_to_target"]["params"]["threshold"])),
        "action_l2": (action.double() ** 2).sum(1),
        "energy": (action.double() * d("joint_vel") * table(names.index("energy"))).abs().sum(1),
        "joint_pos_limits": ((s_abs > th_l).double() * (s_abs - th_l) / _f32(1.0 - R["joint_pos_limits"]["params"]["threshold"])
                             * table(names.index("joint_pos_limits"))).sum(1),
    }
    # progress: the kernel follows the reference's fp32 sequence bit for bit (value = f * w * dt, step_reward = value / dt as the manager
    # does); against fp64 it may differ by the two potentials' own fp32 rounding, measured per env (each within 4 ulp of ~6e4)
    cur32, prev32 = _potential(feed["root_pos_w"], dt, False), _potential(pot0, dt, True)
    k_prog = names.index("progress")
    w_prog, dt32 = np.float32(env.plan.reward_terms[k_prog].weight), np.float32(dt)
    exp32 = torch.from_numpy((((cur32 - prev32).numpy() * w_prog) * dt32) / dt32)
    assert torch.equal(env.reward_manager._step_reward[:, k_prog].cpu(), exp32), "progress: not the fp32 sequence"
    pot_round = ((cur32.double() - cur64.cpu()).abs() + (prev32.double() - prev64.cpu()).abs()).to(pos.device)
    ulp = 2.0 ** (torch.floor(torch.log2(cur64.abs())) - 23)
    assert bool((pot_round <= 8.0 * ulp).all()), float((pot_round / ulp).max())
    ok_up = (up - _f32(R["upright"]["params"]["threshold"])).abs() > 1e-5
    # joint_pos_limits: (|s| - th) / (1 - th) multiplies the fp32 rounding of the normalised position s (sub, mul, div: <= 2 ulp) by
    # 1 / (1 - th) = 100 for Ant's 0.99 -- the rounding the fp32 reference has as well
    ulp_s = 2.0 ** (torch.floor(torch.log2(s_abs.clamp_min(1e-30))) - 23)
    lim_round = ((s_abs > th_l - 1e-5).double() * table(names.index("joint_pos_limits")) * 2.0 * ulp_s
                 / _f32(1.0 - R["joint_pos_limits"]["params"]["threshold"])).sum(1)
    extra = {"progress": pot_round, "joint_pos_limits": lim_round}
    for k, name in enumerate(names):
        w = env.plan.reward_terms[k].weight
        got_k = env.reward_manager._step_reward[:, k].double() / _f32(w)
        val = ref[name]
        tol = FLOAT_TOL * val.abs().clamp_min(1.0) + extra.get(name, 0.0)
        mask = ok_up if name == "upright" else torch.ones_like(ok_up)
        err = (got_k - val).abs()
        assert bool((err <= tol)[mask].all()), (task, N, name, float((err - tol)[mask].max()))
    if N >= 63:
        assert bool((up < 0.93).any()) and bool((up > 0.93).any()) and bool(terminated.any())
        assert bool((s_abs > 0.99).any()) and bool((head < 0.8).any()) and bool((head > 0.8).any())
    env.close()


# ------------------------------------------------------------------------------------------------ potentials across reset() and steps
def test_potentials_follow_reset_and_steps():
    """env.reset() sets every potential to the 3-D formula of the reset state; each step then stores the planar potential, except for the
    envs it resets (3-D formula of that step's state); reset(env_ids) touches only those envs.  Bit for bit against the fp32 formula."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    task = "Isaac-Humanoid-v0"
    fx = load_task_cfg(task)
    N = 4097
    feed = StateFeed(ROBOTS["humanoid"], N, "cuda:0", seed=21, num_snapshots=3)
    _tweak(feed, torch.Generator().manual_seed(21))
    env = ManagerBasedRLEnv(fx, state_feed=feed)
    dt = env.step_dt
    env.reset()
    torch.cuda.synchronize()
    assert torch.equal(env._term_state[0].cpu(), _potential(feed["root_pos_w"], dt, True))
    env.episode_length_buf[::5] = int(env.max_episode_length) - 1  # time-outs too
    gen = torch.Generator().manual_seed(3)
    resets = 0
    for _ in range(4):
        env.step((torch.randn(N, 21, generator=gen) * 0.5).cuda())
        torch.cuda.synchronize()
        r = env.reset_buf.cpu()
        exp = torch.where(r, _potential(feed["root_pos_w"], dt, True), _potential(feed["root_pos_w"], dt, False))
        assert torch.equal(env._term_state[0].cpu(), exp)
        resets += int(r.sum())
    assert resets > 0
    before = env._term_state[0].clone()
    ids = torch.tensor([0, 7, 4096], device="cuda:0")
    env.reset(env_ids=ids)
    torch.cuda.synchronize()
    after = env._term_state[0]
    keep = torch.ones(N, dtype=torch.bool, device="cuda:0")
    keep[ids] = False
    assert torch.equal(after[keep], before[keep])
    assert torch.equal(after[ids].cpu(), _potential(feed["root_pos_w"], dt, True)[ids.cpu()])
    # set_term_cfg (the in-place plan copy) leaves the potentials alone
    env.reward_manager.set_term_cfg("progress", dict(env.reward_manager.get_term_cfg("progress").to_dict(), weight=2.0))
    assert torch.equal(env._term_state[0], after)
    env.close()


# ------------------------------------------------------------------------------------------------ fused rollout = split rollout
def test_three_launch_rollout_equals_six_launch_split_for_humanoid():
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg("Isaac-Humanoid-v0")
    out = {}
    for fuse in (False, True):
        torch.manual_seed(3)
        feed = StateFeed(ROBOTS["humanoid"], 2500, "cuda:0", seed=5, num_snapshots=4)
        _tweak(feed, torch.Generator().manual_seed(5))
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
        out[fuse].update(potentials=env._term_state.clone(), action=env._action.clone(), ep_len=env.episode_length_buf.clone(),
                         log_out=env._log_out.clone())
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

    fx = load_task_cfg(task)
    torch.manual_seed(seed)
    feed = StateFeed(ROBOTS[fx["robot"]], 4096, "cuda:0", seed=seed, num_snapshots=4)
    _tweak(feed, torch.Generator().manual_seed(seed))  # low torsos: terminations in every rollout
    env = RslRlVecEnvWrapper(ManagerBasedRLEnv(fx, state_feed=feed, own_managers=True, seed=seed))
    u = env.unwrapped
    assert u.event_manager.active_terms["reset"] == ["reset_base", "reset_robot_joints"]
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=8), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    u.episode_length_buf[::5] = int(u.max_episode_length) - 20  # time-outs inside the recorded rollout (steps 16-23): the reset events run
    # a graph runner warms up with one eager rollout before it captures (runner.collect): two replays follow three eager rollouts
    for _ in range(2 if use_graph else 3):
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    runner.learn(1)
    torch.cuda.synchronize()
    res["params"] = runner.alg.bucket.flat.clone()
    res["potentials"] = u._term_state.clone()
    res["sim_joint_pos"] = u.sim_writes["joint_pos"].clone()
    out = {k: v.cpu() for k, v in res.items()}
    env.close()
    return out


@pytest.mark.parametrize("task", TASKS)
def test_classic_4096_training_graph_equals_eager_and_reproduces(task):
    a = _train_once(task, 17, True)
    b = _train_once(task, 17, True)
    c = _train_once(task, 17, False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), f"{k}: not reproducible"
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert float(a["dones"].sum()) > 0 and float(a["rewards"].abs().sum()) > 0
    assert float(a["sim_joint_pos"].abs().sum()) > 0  # reset_joints_by_offset wrote joint states


# ------------------------------------------------------------------------------------------------ policy shapes at the training batch
@pytest.mark.parametrize("task,D,A", [("Isaac-Ant-v0", 60, 8), ("Isaac-Humanoid-v0", 87, 21)])
def test_update_gradient_at_classic_shapes(monkeypatch, task, D, A):
    """[400, 200, 100] ELU actor and critic at the tasks' D and A, M = 4096 envs x 32 steps / 4 minibatches = 32 768 rows, through the
    storage's own permutation and gather, against fp64 autograd (tests/_util.py tolerance rule)."""
    import isaaclab_amd.rsl_rl.ppo as ppo_mod
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    fx = load_task_cfg(task)
    plan = compile_plan(fx["env"], ROBOTS[fx["robot"]])
    assert (plan.obs_dim, plan.action_dim) == (D, A)
    agent = fx["agent"]
    T, nmb = int(agent["num_steps_per_env"]), int(agent["algorithm"]["num_mini_batches"])
    assert (T, nmb) == (32, 4)
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
    assert batch[0].shape[0] == 32_768
    for two_streams in (True, False):
        monkeypatch.setattr(ppo_mod, "FUSED_HEAD", "0")
        alg.two_streams = two_streams
        check_minibatch_gradients(alg, batch, f"{task} two_streams={two_streams}")
