"""GPU: ``PreTrainedPolicyAction`` on the fused path -- ``imx_pretrained_policy`` against the chain of existing launches (bit for bit), what
it may read and write, the recordings P1-P3 of the REAL class, and the env / manager / runner wiring on the
Isaac-Navigation-Flat-Anymal-C-v0 fixture.  Bounds: tests/_navigation_cases.py ``bound``."""

import copy
import ctypes

import pytest
import torch

import _navigation_cases as nc
import _navigation_oracle as no
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu

PAD = 3  # envs allocated past the N a launch is given: their rows hold NaN and must stay NaN
READ = ("root_quat_w", "root_lin_vel_w", "root_ang_vel_w", "root_pos_w", "joint_pos", "joint_vel", "default_joint_pos", "default_joint_vel")


def _synthetic_env(variant: str, n: int, fused: bool, tile_rows: int = 0, seed: int = 11):
    """An env on the variant's cfg and policy over a synthetic feed of n + PAD envs; every state tensor the low-level step does not read
    is NaN, and so are the rows past n of those it reads."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    g = nc.NavGolden(variant)
    feed = StateFeed(ROBOTS[g.meta["robot"]], n + PAD, "cuda:0", seed=seed, num_snapshots=2)
    for store in (feed._stack, feed._static):
        for name, t in store.items():
            if not t.is_floating_point():
                continue
            if name not in READ:
                t.fill_(float("nan"))
            elif store is feed._stack:
                t[:, n:] = float("nan")
            else:
                t[n:] = float("nan")
    env = ManagerBasedRLEnv(g.env_cfg(), state_feed=feed, low_level_policy=g.layers, noise_seed=seed, fused_low_level=fused,
                            low_level_tile_rows=tile_rows)
    return env, g


def _drive(variant: str, n: int, fused: bool, noise: str, tile_rows: int = 0, steps: int = 3):
    """``steps`` low-level steps on n envs of an env that holds n + PAD: the outputs of every step (rows < n) and the final full tensors."""
    env, g = _synthetic_env(variant, n, fused, tile_rows)
    D, A = g.meta["obs_dim"], g.meta["action_dim"]
    gen = torch.Generator().manual_seed(100 + n)
    nan = float("nan")
    env._processed_action.copy_(torch.randn(n + PAD, 3, generator=gen))
    env._processed_action[n:] = nan
    ep = torch.where(torch.rand(n + PAD, generator=gen) < 0.3, 0, 5)  # episode_length_buf: 0 on about a third of the envs
    ep[n:] = 5
    env._episode_length_buf.copy_(ep)
    env._ll_actions.copy_(torch.randn(n + PAD, A, generator=gen))  # (a carried low_level_actions; zeroed in the rows with episode_length_buf 0)
    for t in (env._ll_actions, env._ll_joint_pos_target, env._ll_prev):
        t[n:] = nan
    env._ll_obs_out = torch.full((n + PAD, D), nan, device=env.device)
    env._ll_obs.fill_(nan)
    env._ll_out.fill_(nan)
    env.num_envs = n  # the launches take n envs of the n + PAD the buffers hold
    outs = []
    for k in range(steps):
        env._ll_noise_u = None
        if noise == "recorded":
            u = torch.rand(n + PAD, D, generator=gen)
            u[n:] = nan
            env._ll_noise_u = u.cuda()
        env._ll_launch()
        obs = env._ll_obs_out if fused else env._ll_obs
        outs.append(tuple(x[:n].clone().cpu() for x in (obs, env._ll_actions, env._ll_joint_pos_target)))
        if k == 0:
            env._episode_length_buf.fill_(5)  # later steps carry the policy's own output
    torch.cuda.synchronize()
    tail = tuple(x[n:].clone().cpu() for x in (obs, env._ll_actions, env._ll_joint_pos_target))
    zero_rows = (ep[:n] == 0)
    env.close()
    return outs, tail, zero_rows


@pytest.mark.parametrize("noise", ["recorded", "kernel"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 64, 65, 256])
@pytest.mark.parametrize("variant", ["P1", "P2"])
def test_fused_equals_the_chain_bit_for_bit(variant, n, noise):
    """One launch against masked zero -> imx_observations -> imx_mlp_infer -> imx_action_process: the observation rows (through the debug
    pointer), low_level_actions and the joint targets of three consecutive low-level steps.  Same device functions, same summation
    order: equal bits.  Rows past N keep their NaN; NaN in every unread tensor and in the rows past N of the read ones reaches nothing."""
    fused, tail_f, zero_rows = _drive(variant, n, True, noise)
    chain, tail_c, _ = _drive(variant, n, False, noise)
    A = 12
    for k, (a, b) in enumerate(zip(fused, chain)):
        for name, x, y in zip(nc.LL_OUTPUTS, a, b):
            assert torch.isfinite(x).all(), f"{variant} n={n} step {k} {name}: not finite"
            assert torch.equal(x, y), f"{variant} n={n} {noise} step {k} {name}: {int((x != y).sum())} elements differ, max {float((x - y).abs().max()):.3g}"
    # the zeroed `actions` block (the group's last columns, no noise on them) exactly where episode_length_buf was 0
    blk = fused[0][0][:, -A:]
    assert (blk[zero_rows] == 0).all() and (n < 8 or (blk[~zero_rows] != 0).any())
    for name, x in zip(nc.LL_OUTPUTS, tail_f):
        assert torch.isnan(x).all(), f"{variant} n={n} {name}: the fused launch wrote past N"
    for x in tail_c[1:]:
        assert torch.isnan(x).all()


@pytest.mark.parametrize("variant", ["P1", "P2"])
def test_tile_heights(variant):
    """The 32-row kernel: against the chain where the chain's imx_mlp_infer runs 32-row tiles itself (more than 4096 rows for one network:
    bit for bit, ragged last tile), and against the 16-row kernel at a small N (another MFMA shape, another summation order: within
    FLOAT_TOL of each other, and both within it of the fp64 restatement through test_kernel_matches_the_reference)."""
    from isaaclab_amd import _lib

    n = 4128 + 7
    assert int(_lib.lib().imx_pretrained_policy_tile_rows(n)) == 32 and int(_lib.lib().imx_pretrained_policy_tile_rows(4096)) == 16
    big, tail, _ = _drive(variant, n, True, "kernel", tile_rows=32, steps=2)
    chain, _, _ = _drive(variant, n, False, "kernel", steps=2)
    for a, b in zip(big, chain):
        for name, x, y in zip(nc.LL_OUTPUTS, a, b):
            assert torch.isfinite(x).all() and torch.equal(x, y), f"{variant} {name}: 32-row tiles differ from the chain"
    assert all(torch.isnan(x).all() for x in tail)
    for m in (33, 70):
        a, tail, _ = _drive(variant, m, True, "recorded", tile_rows=32)
        b, _, _ = _drive(variant, m, True, "recorded", tile_rows=16)
        assert all(torch.isnan(x).all() for x in tail)
        assert torch.equal(a[0][0], b[0][0]), "the first step's observation rows do not depend on the tile height"
        for s32, s16 in zip(a, b):  # (later rows read the carried low_level_actions, which differ in their last bits)
            for x, y in zip(s32, s16):
                assert_close(x, y, FLOAT_TOL, f"{variant} n={m}: 32-row against 16-row tiles")


@pytest.mark.parametrize("tile_rows", [16, 32])
@pytest.mark.parametrize("variant", nc.VARIANTS)
def test_kernel_matches_the_reference(variant, tile_rows):
    """All 64 envs, every low-level step of the three env steps, the kernel carrying its own low_level_actions: each element within
    FLOAT_TOL (assert_close's rule) of the fp64 restatement or within twice the real class's own fp32 error against it."""
    g = nc.NavGolden(variant)
    got, r64 = nc.run_low_level(g, 64, low_level_tile_rows=tile_rows), nc.restated(variant)
    assert list(got) == g.low_level_steps()
    worst = {}
    for key, outs in got.items():
        for name, x, y in zip(nc.LL_OUTPUTS, outs, r64[key]):
            assert x.shape == y.shape == (64, y.shape[1]) and torch.isfinite(x).all()
            err, lim = (x.double() - y).abs(), nc.bound(y, nc.e_ref(variant, name))
            worst[name] = max(worst.get(name, 0.0), float((err / lim).max()))
            assert (err <= lim).all(), f"{variant} rows {tile_rows} step {key} {name}: max err {float(err.max()):.3g}, {int((err > lim).sum())} over"
    print(f"{variant} rows {tile_rows}: largest err / bound {worst}, e_ref {[nc.e_ref(variant, n_) for n_ in nc.LL_OUTPUTS]}")


def test_the_chain_matches_the_reference_too():
    g = nc.NavGolden("P2")
    got, r64 = nc.run_low_level(g, 64, fused_low_level=False), nc.restated("P2")
    for key, outs in got.items():
        for name, x, y in zip(nc.LL_OUTPUTS, outs, r64[key]):
            assert ((x.double() - y).abs() <= nc.bound(y, nc.e_ref("P2", name))).all(), (key, name)


def test_refused_calls_write_nothing():
    from isaaclab_amd import _lib

    env, g = _synthetic_env("P1", 8, True)
    L = _lib.lib()
    before = [x.clone() for x in (env._ll_actions, env._ll_joint_pos_target, env._ll_prev)]
    st, pol = env._ll_state(), env._ll_policy.struct

    def call(N=8, st=st, bf=env._ll_bufs, pol=pol, rows=0, plan=env._ll_plan_h):
        return L.imx_pretrained_policy(plan, N, ctypes.byref(st), ctypes.byref(bf), ctypes.byref(pol), None, 0, None, 1, 0, 1, rows, None,
                                       _lib.current_stream(env.device))

    bad_pol = type(pol).from_buffer_copy(bytes(pol))
    bad_pol.dims[4] = 11
    bad_bf = type(env._ll_bufs).from_buffer_copy(bytes(env._ll_bufs))
    bad_bf.episode_length_buf = None
    bad_st = type(st).from_buffer_copy(bytes(st))
    bad_st.command = None
    for kw, why in ((dict(N=0), "num_envs"), (dict(rows=24), "tile_rows 24"), (dict(pol=bad_pol), "11 outputs"), (dict(bf=bad_bf), "episode_length_buf"),
                    (dict(st=bad_st), "'command'"), (dict(plan=env._plan_h), "the low-level observation group has 10")):
        assert call(**kw) != 0, kw
        assert why in L.imx_last_error().decode(), (kw, L.imx_last_error().decode())
    torch.cuda.synchronize()
    for x, y in zip(before, (env._ll_actions, env._ll_joint_pos_target, env._ll_prev)):
        assert torch.equal(x, y), "a refused call wrote to an output"
    env.close()


# ------------------------------------------------------------------------------------------------ env, managers, runner
def _nav_env(N=256, seed=19, **kw):
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg(nc.task_path())
    feed = StateFeed(ROBOTS[fx["robot"]], N, "cuda:0", seed=seed, num_snapshots=4)
    return ManagerBasedRLEnv(fx, state_feed=feed, seed=seed, noise_seed=seed, **kw), fx


STATE_KEYS = READ + ("command", "net_forces_w_history")


def _cpu_state(env):
    return {k: env.feed[k].cpu().clone() for k in STATE_KEYS}


def test_navigation_env_steps_match_the_restatement():
    """256 envs, three steps of decimation 40 (ten low-level steps each) on ``load_task_cfg(path)``: low_level_actions and the joint targets
    after each env step, the policy observation, the reward and its terms, the terminations, the term's views -- against the fp64
    restatement on the same feed.  Every fourth env times out in step 1, so step 2 runs its ten low-level steps on a zeroed ``actions``
    block for them.  The low-level noise is fed (one (N, 48) array of uniforms for all low-level steps) so that the restatement sees it."""
    env, fx = _nav_env()
    N, pt = env.num_envs, env.plan.policy_terms[0]
    assert env.cfg_decimation == 40 and pt.low_level_decimation == 4 and N == 256 and env._ll_fused
    env.reset()
    term = env.action_manager.get_term(nc.TERM)
    assert term.action_dim == 3 and term.raw_actions.data_ptr() == term.processed_actions.data_ptr() == env._processed_action.data_ptr()
    assert term.low_level_actions.shape == (N, 12) and term.joint_pos_target.shape == (N, 12) and env.action_manager.total_action_dim == 3
    gen = torch.Generator().manual_seed(3)
    u = torch.rand(N, 48, generator=gen)
    env._ll_noise_u = u.cuda()
    robot = env.plan.robot
    layers = env._ll_policy.layers.layers
    o64 = no.LowLevelOracle(fx["env"]["actions"][nc.TERM], robot.joint_names, layers, dtype=torch.float64, gravity_dir=env.feed.gravity_dir)
    base = [robot.body_names.index("base")]
    lla = torch.zeros(N, 12, dtype=torch.float64)
    e_ref = {n_: nc.e_ref("P1", n_) for n_ in nc.LL_OUTPUTS}  # (the task's own cfg is variant P1)
    saw_zero = False
    for step in range(3):
        if step == 1:
            env.episode_length_buf = torch.where(torch.arange(N, device="cuda:0") % 4 == 0, env.max_episode_length - 1, env.episode_length_buf)
        ep = env.episode_length_buf.cpu().clone()
        st = _cpu_state(env)  # the feed moves on at the end of the physics: every low-level launch of this step reads this state
        action = torch.randn(N, 3, generator=gen)
        for _ in range(o64.launches(40)):
            obs64, lla, target64 = o64.low_level_step(st, action, lla, ep, u)
        saw_zero = saw_zero or (step > 0 and bool((ep == 0).any()) and bool((ep != 0).any()))
        obs, rew, terminated, time_outs, _ = env.step(action.cuda())
        torch.cuda.synchronize()
        assert torch.equal(term.raw_actions.cpu(), action) and torch.equal(env.action_manager.action.cpu()[~(terminated | time_outs).cpu()],
                                                                           action[~(terminated | time_outs).cpu()])
        for name, x, y in (("low_level_actions", term.low_level_actions, lla), ("joint_pos_target", term.joint_pos_target, target64)):
            err = (x.cpu().double() - y).abs()
            assert (err <= nc.bound(y, e_ref[name])).all(), f"step {step} {name}: max err {float(err.max()):.3g}"
        st1 = _cpu_state(env)
        to64, contact64 = no.terminations(st1, ep + 1, env.max_episode_length, base, 1.0, torch.float64)
        assert torch.equal(time_outs.cpu(), to64) and torch.equal(terminated.cpu(), contact64), step
        if step == 1:
            assert to64[::4].all()
        rew64, terms64 = no.rewards(fx["env"]["rewards"], st1, contact64, env.step_dt, torch.float64)
        assert_close(rew, rew64, FLOAT_TOL, f"step {step} reward")
        assert_close(env._step_reward, terms64, FLOAT_TOL, f"step {step} reward terms")
        assert_close(obs["policy"], no.policy_observation(st1, env.feed.gravity_dir, torch.float64), FLOAT_TOL, f"step {step} policy observation")
        assert obs["policy"].shape == (N, 10)
        assert torch.equal((env.episode_length_buf == 0).cpu(), to64 | contact64)
    assert saw_zero
    env.close()


def test_manager_calls_give_what_step_gives_and_show_the_zeroed_block():
    a = torch.randn(64, 3, generator=torch.Generator().manual_seed(9)).cuda()
    env, _ = _nav_env(64)
    env.reset()
    env.step(a)
    torch.cuda.synchronize()
    by_step = [x.clone() for x in (env._processed_action, env._ll_actions, env._ll_joint_pos_target)]
    env.close()
    env, _ = _nav_env(64)
    env.reset()
    am = env.action_manager
    term = am.get_term(nc.TERM)
    env._ll_obs_out = torch.zeros(64, 48, device="cuda:0")
    am.process_action(a)
    am.apply_action()  # the counter is 0: the first low-level step; all envs are at episode_length_buf 0
    torch.cuda.synchronize()
    assert (env._ll_obs_out[:, -12:] == 0).all() and torch.equal(env._ll_obs_out[:, 9:12], a) and float(term.low_level_actions.abs().sum()) > 0
    first = term.low_level_actions.clone()
    for _ in range(3):  # substeps 1-3: no launch
        am.apply_action()
    torch.cuda.synchronize()
    assert torch.equal(first, term.low_level_actions) and env._ll_counter == 4
    env._episode_length_buf[1::2] = 7  # half of the envs are past their first step: their `actions` block is the carried output
    am.apply_action()
    torch.cuda.synchronize()
    blk = env._ll_obs_out[:, -12:]
    assert (blk[0::2] == 0).all() and torch.equal(blk[1::2], first[1::2])
    env.close()
    # the same schedule by hand: process_action, then `decimation` apply_action calls
    env, _ = _nav_env(64)
    env.reset()
    am = env.action_manager
    am.process_action(a)
    for _ in range(40):
        am.apply_action()
    torch.cuda.synchronize()
    for x, y in zip(by_step, (env._processed_action, env._ll_actions, env._ll_joint_pos_target)):
        assert torch.equal(x, y)
    # ActionManager.reset: the manager's action is zeroed, nothing of the term (it has no reset)
    ids = torch.tensor([0, 5, 63], device="cuda:0")
    am.reset(ids)
    term = am.get_term(nc.TERM)
    assert float(am.action[ids].abs().sum()) == 0.0 and torch.equal(term.raw_actions, by_step[0]) and torch.equal(term.low_level_actions, by_step[1])
    assert env._ll_counter == 4  # (40 calls, a launch on every fourth: PreTrainedPolicyAction._counter)
    with pytest.raises(ValueError, match="PreTrainedPolicyAction.*command of the low-level policy.*joint_pos_target"):
        env.attach_actuator(object())
    env.close()


def test_env_refusals():
    from isaaclab_amd.env import ManagerBasedRLEnv

    fx = nc.fixture()
    for kw in (dict(command_term="pose_command"), dict(own_managers=True)):
        with pytest.raises(NotImplementedError, match=r"command_term='pose_command'.*UniformPose2dCommand.*no fused producer"):
            _nav_env(8, **kw)
    with pytest.raises(ValueError, match="maps 45 -> 12 columns; the low-level observation group has 48"):
        _nav_env(8, low_level_policy=nc.NavGolden("P2").layers)
    bad = copy.deepcopy(fx)
    bad["env"]["actions"][nc.TERM]["policy_path"] = "omniverse://nucleus/Policies/ANYmal-C/Blind/policy.pt"
    with pytest.raises(FileNotFoundError, match=r"Policy file 'omniverse://.*' does not exist\..*low_level_policy="):
        ManagerBasedRLEnv(bad, num_envs=8, device="cuda:0")
    with pytest.raises(ValueError, match="low_level_tile_rows=8"):
        _nav_env(8, low_level_tile_rows=8)
    with pytest.raises(ValueError, match="no PreTrainedPolicyAction"):
        ManagerBasedRLEnv("Isaac-Velocity-Flat-Anymal-C-v0", num_envs=8, device="cuda:0", low_level_policy=nc.ARCHIVE)


def test_a_schedule_that_does_not_divide_runs_eagerly_and_is_refused_under_capture():
    """decimation 7, low_level_decimation 2: launches on substeps 0, 2, 4, 6 of the first env step, 1, 3, 5 of the second (the counter runs
    across env steps, pre_trained_policy_action.py:94-100)."""
    g = nc.NavGolden("P2")
    fx = g.env_cfg()
    fx["env"]["decimation"] = 7
    from isaaclab_amd.env import ManagerBasedRLEnv

    env = ManagerBasedRLEnv(fx, state_feed=nc.recorded_feed(g, 16), low_level_policy=g.layers)
    env.reset()
    a = torch.zeros(16, 3, device="cuda:0")
    counts = []
    for _ in range(4):
        env.step(a)
        counts.append(env._ll_in_step)
    assert counts == [4, 3, 4, 3] and env._ll_stride > 4
    env._ll_check_schedule(capturing=False)
    with pytest.raises(NotImplementedError, match="decimation 7 is no multiple of low_level_decimation 2.*captured rollout cannot replay"):
        env._ll_check_schedule(capturing=True)
    env.close()


def _nav_rollout(use_graph, fused=True):
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    torch.manual_seed(31)
    u, fx = _nav_env(64, seed=31, fused_low_level=fused)
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone().cpu() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    res.update(low_level_actions=u._ll_actions.clone().cpu(), joint_pos_target=u._ll_joint_pos_target.clone().cpu(), processed=u._processed_action.clone().cpu())
    env.close()
    return res


def test_captured_rollout_equals_eager_on_navigation():
    a, c = _nav_rollout(True), _nav_rollout(False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert a["actions"].shape == (4, 64, 3) and a["observations"].shape == (4, 64, 10) and float(a["joint_pos_target"].abs().sum()) > 0.0
    # the chain gives the same rollout as the fused launch (in-kernel noise keyed alike)
    d = _nav_rollout(False, fused=False)
    for k in a:
        assert torch.equal(a[k], d[k]), f"{k}: fused and unfused rollouts differ"
