"""GPU: ``imx_mlp_infer_act2`` -- the rollout inference launch for an actor and a critic that read different rows -- and the runner's
three-launch step on envs with a "critic" observation group.

1. plain inference against two single-network ``imx_mlp_infer`` launches, bit for bit: six pairs of input widths, stacks of different
   depth, row-pitched inputs, the 16-row kernel (1 .. 1000 rows) and the 32-row kernel (the first row counts the dispatch rule sends
   there on this device; packed and row-layout weights); one case against the float64 modules;
2. the act variant against the plain call + ``imx_policy_act`` + ``imx_action_process`` + a copy of the critic rows, bit for bit, with a
   storage slot of sentinels on either side of the written one;
3. the runner on the kitchen fixture (64 envs, eager and captured; 2500 envs over a synthetic feed): ``fuse_launches`` False against
   True leaves bit-identical storages and env buffers, and the fused path is the one that ran;
4. a binary joint term beside a critic group (Lift-Cube plus a ``critic`` group), split against fused; the Lift-Cube plan under the
   actor head of the 32-row kernels (2081 rows, packed and row-layout weights), as part 2 compares.

The single-network reference of part 1: the 16- and the 32-row kernels sum a dot product in different orders (16x16x4 against 32x32x2
MFMAs), so a reference is only bit-comparable when it runs the tile height the launch under test ran.  The dispatch rule counts
workgroups (row tiles x networks), and ONE network at 2049 rows still gets 16-row tiles where two get 32-row ones.  The reference
launches for the 32-row cases therefore run on the same rows repeated up to the first row count that sends one network to the 32-row
kernel (4097 on 256 CUs); rows are independent, and the first M output rows are the ones compared."""

import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from _util import FLOAT_TOL, KITCHEN, Golden, assert_close

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
# (actor input width, critic input width, actions, actor hidden, critic hidden, row-pitched inputs with NaN pad columns)
SHAPES = [(48, 235, 12, [128, 64, 32], [96], False), (235, 48, 37, [64], [256, 128, 64], True), (1, 512, 12, [512, 256, 128], [32], False),
          (512, 1, 3, [32], [512, 256, 128], False), (33, 31, 37, [100, 50], [7], True), (64, 64, 12, [128, 128, 128], [128], False)]
ROWS = (1, 15, 16, 17, 33, 1000, "first32", "first32+31")


def _cus() -> int:
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _first32(nnets: int) -> int:
    """The smallest M the dispatch rule (16-row tiles while 2 * 32-row tiles * networks <= CUs) sends to the 32-row kernel."""
    tiles = _cus() // (2 * nnets) + 1
    return 32 * (tiles - 1) + 1


def _rows(spec) -> tuple[int, bool]:
    if isinstance(spec, int):
        assert spec < _first32(2)
        return spec, False
    return _first32(2) + (31 if spec.endswith("+31") else 0), True


_pairs: dict = {}


def _pair(i: int):
    """The policy of SHAPES[i], its two-input FusedInference and one single-network FusedInference per stack (built once)."""
    if i not in _pairs:
        from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
        from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

        Dp, Dc, A, ah, ch, _ = SHAPES[i]
        torch.manual_seed(100 + i)
        pol = ActorCritic(Dp, Dc, A, actor_hidden_dims=ah, critic_hidden_dims=ch, init_noise_std=0.7).cuda()
        with torch.no_grad():
            for lin in [m for m in list(pol.actor) + list(pol.critic) if isinstance(m, torch.nn.Linear)]:
                lin.bias.normal_(0.0, 0.3)
        two = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic), two_inputs=True)
        assert two.ok and two.two_inputs and two._wpk is not None
        _pairs[i] = (pol, two, FusedInference(_mlp_layers(pol.actor)), FusedInference(_mlp_layers(pol.critic)))
    return _pairs[i]


def _input(M: int, D: int, pitched: bool, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    pitch = D + 5 if pitched else D
    xb = torch.full((M, pitch), float("nan"))
    xb[:, :D] = torch.randn(M, D, generator=g)
    return xb.cuda()[:, :D]


def _single(inf, x: torch.Tensor, big: bool) -> torch.Tensor:
    """``imx_mlp_infer`` on one network, at the tile height of the launch under test (module docstring)."""
    from isaaclab_amd import _lib

    M = x.shape[0]
    if big and M < _first32(1):
        x = x[torch.arange(_first32(1), device=x.device) % M].contiguous()
    out = torch.full((x.shape[0], inf.out_features[0]), float("nan"), device="cuda")
    _lib.check(_lib.lib().imx_mlp_infer(x.shape[0], x.data_ptr(), x.stride(0), 1, inf._nl, inf._dims, inf._w, inf._pitch, inf._b, inf._alpha,
                                        (ctypes.c_void_p * 1)(out.data_ptr()), torch.cuda.current_stream().cuda_stream))
    return out[:M]


def _two(two, x, cx, packed: bool):
    M = x.shape[0]
    mu = torch.full((M + 40, two.out_features[0]), SENTINEL, device="cuda")  # (40 rows past M: a ragged last tile must not reach them)
    val = torch.full((M + 40, 1), SENTINEL, device="cuda")
    keep = two._wpk
    if not packed:
        two._wpk = None
    try:
        two(x, mu, val, critic_x=cx)
    finally:
        two._wpk = keep
    torch.cuda.synchronize()
    assert bool((mu[M:] == SENTINEL).all()) and bool((val[M:] == SENTINEL).all()), "rows beyond M were written"
    return mu[:M], val[:M]


# ------------------------------------------------------------------------------------------------ 1. plain inference
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_plain_two_input_inference_equals_two_single_network_launches(shape, rows):
    Dp, Dc, A, _, _, pitched = SHAPES[shape]
    M, big = _rows(rows)
    pol, two, actor1, critic1 = _pair(shape)
    x, cx = _input(M, Dp, pitched, 7 * M + shape), _input(M, Dc, pitched, 7 * M + shape + 1)
    assert (x.stride(0) > Dp) == pitched and (cx.stride(0) > Dc) == pitched
    mu_ref, val_ref = _single(actor1, x, big), _single(critic1, cx, big)
    assert bool(torch.isfinite(mu_ref).all()) and bool(torch.isfinite(val_ref).all())
    for packed in ((True, False) if big else (True,)):  # (the 16-row kernel reads the rows whether a packed image exists or not)
        mu, val = _two(two, x, cx, packed)
        assert torch.equal(mu, mu_ref), f"actor output, packed={packed}"
        assert torch.equal(val, val_ref), f"critic output, packed={packed}"
    if Dp == Dc:  # the same width is still another input
        assert not torch.equal(x, cx)


@pytest.mark.parametrize("rows", [33, "first32+31"])
def test_plain_two_input_inference_against_float64(rows):
    """Same arithmetic as ``FusedInference`` on a shared input: the bound of tests/test_policy_shapes_gpu.py (``check_fused_inference``)."""
    M, _ = _rows(rows)
    pol, two, _, _ = _pair(1)
    Dp, Dc, _, _, _, pitched = SHAPES[1]
    x, cx = _input(M, Dp, pitched, 11), _input(M, Dc, pitched, 12)
    mu, val = _two(two, x, cx, True)
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        assert_close(mu, p64.actor(x.double()), FLOAT_TOL, "mu")
        assert_close(val, p64.critic(cx.double()), FLOAT_TOL, "value")


def test_one_network_through_the_two_input_entry_point():
    """nnets == 1 is ``imx_mlp_infer`` on X_d[0]."""
    from isaaclab_amd import _lib

    pol, _, actor1, _ = _pair(0)
    x = _input(77, SHAPES[0][0], True, 3)
    ref = _single(actor1, x, False)
    out = torch.full_like(ref, float("nan"))
    _lib.check(_lib.lib().imx_mlp_infer_act2(77, (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int64 * 1)(x.stride(0)), 1, actor1._nl, actor1._dims,
                                             actor1._w, actor1._pitch, actor1._wpk, actor1._b, actor1._alpha,
                                             (ctypes.c_void_p * 1)(out.data_ptr()), None, None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ 2. the act variant
def _env(task: str, N: int):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    g = Golden(task)
    mesh, ext = g.mesh(), None
    if mesh is not None:
        ext = (float(np.abs(mesh[0][:, 0]).max()) - 2.0, float(np.abs(mesh[0][:, 1]).max()) - 2.0)
    feed = StateFeed(ROBOTS[g.fixture["robot"]], N, "cuda:0", seed=5, num_snapshots=2, extent_xy=ext)
    env = ManagerBasedRLEnv(g.fixture, state_feed=feed, terrain=mesh, noise_seed=11)
    env.reset()
    return env


def check_act_variant(env, pol, inf, x, cx, clip, norms=None, packed=True):
    """One launch with ``ImxPolicyAct`` against the launches it replaces, bit for bit: the plain call, ``imx_policy_act``, the env's action
    terms (``imx_action_process``) and a copy of the critic rows, with a storage slot of sentinels on either side of the written one.
    ``cx`` None: a shared-input ``inf`` (no critic rows are kept).  ``norms`` (the policy's and the critic's ``EmpiricalNormalization``):
    the one launch normalises the raw rows itself, the others start from ``apply``'s rows.  ``packed`` False: the row-layout weights."""
    from isaaclab_amd import _lib

    N, D, A = x.shape[0], x.shape[1], env.plan.action_dim
    Dc, seed = (cx.shape[1] if cx is not None else 0), 12345
    xr, cxr = (x, cx) if norms is None else (norms[0].apply(x), norms[1].apply(cx))
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(4)
    env._action.copy_(torch.randn(env._action.shape, generator=g))
    env._prev_action.copy_(torch.randn(env._prev_action.shape, generator=g))
    env.clip_actions = clip
    start = [b.clone() for b in (env._action, env._prev_action, env._processed_action)]
    stp = torch.tensor([5], dtype=torch.int32, device="cuda")

    def slots():  # three storage slots per output: the middle one is written
        S = lambda *sh: torch.full((3, *sh), SENTINEL, device="cuda")  # noqa: E731
        o = dict(actions=S(N, A), log_prob=S(N), mu=S(N, A), sigma=S(N, A), values=S(N, 1), observations=S(N, D))
        if cx is not None:
            o["privileged_observations"] = S(N, Dc)
        return o

    def env_buffers():
        return dict(action=env._action.clone(), prev_action=env._prev_action.clone(), processed_action=env._processed_action.clone())

    keep = inf._wpk
    if not packed:
        inf._wpk = None
    try:
        # the four launches
        ref = slots()
        mu, val = torch.empty(N, A, device="cuda"), torch.empty(N, 1, device="cuda")
        inf(xr, mu, val, **({} if cx is None else dict(critic_x=cxr)))
        _lib.check(L.imx_policy_act(N, A, D, mu.data_ptr(), pol.std.data_ptr(), val.data_ptr(), xr.data_ptr(), seed, stp.data_ptr(),
                                    ref["actions"][1].data_ptr(), ref["log_prob"][1].data_ptr(), ref["mu"][1].data_ptr(), ref["sigma"][1].data_ptr(),
                                    ref["values"][1].data_ptr(), ref["observations"][1].data_ptr(), None, s))
        env._process_action(ref["actions"][1])
        if cx is not None:
            ref["privileged_observations"][1].copy_(cxr)
        torch.cuda.synchronize()
        ref.update(env_buffers())
        # the one launch, from the same env buffers
        for b, b0 in zip((env._action, env._prev_action, env._processed_action), start):
            b.copy_(b0)
        got = slots()
        act = _lib.ImxPolicyAct(std_d=pol.std.data_ptr(), seed=seed, step_counter_d=stp.data_ptr(), actions_out_d=got["actions"][1].data_ptr(),
                                logp_out_d=got["log_prob"][1].data_ptr(), mu_out_d=got["mu"][1].data_ptr(), sigma_out_d=got["sigma"][1].data_ptr(),
                                obs_out_d=got["observations"][1].data_ptr(), plan=env._plan_h.value, state=ctypes.pointer(env._state()),
                                buf=ctypes.pointer(env._bufs), pre_clip=math.inf if clip is None else float(clip))
        inf(x, None, got["values"][1], act=act, norm=norms,
            **({} if cx is None else dict(critic_x=cx, critic_obs_out=got["privileged_observations"][1])))
        torch.cuda.synchronize()
    finally:
        inf._wpk = keep
    got.update(env_buffers())
    for k in ref:
        assert torch.equal(ref[k], got[k]), f"{k}: one launch differs from the four"
    for k in slots():
        assert bool((got[k][0] == SENTINEL).all()) and bool((got[k][2] == SENTINEL).all()), f"{k}: a slot beside the written one was touched"
        assert bool((got[k][1] != SENTINEL).all()) and bool(torch.isfinite(got[k][1]).all()), k
    assert torch.equal(got["observations"][1], xr) and (cx is None or torch.equal(got["privileged_observations"][1], cxr.contiguous()))
    assert not torch.equal(got["action"], start[0]) and torch.equal(got["prev_action"], start[0])
    if clip is not None:
        assert float(got["action"].abs().max()) <= float(np.float32(clip))


@pytest.mark.parametrize("task,A,rows,clip", [("Isaac-Velocity-Flat-Anymal-C-v0", 12, 33, None), ("Isaac-Velocity-Flat-Anymal-C-v0", 12, "first32", 0.8),
                                              ("Isaac-Velocity-Rough-G1-v0", 37, 33, 0.8), ("Isaac-Velocity-Rough-G1-v0", 37, "first32", None)])
def test_act_variant_equals_plain_call_policy_act_action_process_and_copy(task, A, rows, clip):
    """One launch against four.  Both row counts end in a ragged tile (33 = 2 x 16 + 1; the first 32-row count = 32 k + 1): the slot after
    the written one is where rows beyond M would land."""
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    N, big = _rows(rows)
    assert N % (32 if big else 16) == 1
    env = _env(task, N)
    D = env.plan.obs_dim
    assert env.plan.action_dim == A
    Dc = D + 13
    torch.manual_seed(5)
    pol = ActorCritic(D, Dc, A, actor_hidden_dims=[128, 64], critic_hidden_dims=[96], init_noise_std=0.7).cuda()
    two = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
    assert two.ok and two.two_inputs
    check_act_variant(env, pol, two, _input(N, D, False, 21), _input(N, Dc, True, 22), clip)
    env.close()


def binary_head_on_32_row_tiles(family: str, packed: bool):
    """The ``_binary`` 32-row kernels, which the Lift rollouts (257 envs: 16-row tiles) do not reach: the Lift-Cube plan (a binary joint
    term) under the actor head at the first 32-row count + 32 (2081 rows on 256 CUs: 66 tiles, one row in the last), input widths 48 and
    235 (one 64-column piece and four, neither a multiple of 32).  ``family``: "shared" (``imx_mlp_infer_act``), "two"
    (``imx_mlp_infer_act2``) or "normalised" (``imx_mlp_infer_act2n``)."""
    import _lift_cases as lc
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers
    from isaaclab_amd.state_feed import StateFeed

    N = _first32(2) + 32
    Dp, Dc = (48, 235) if family != "shared" else ((48, 48) if packed else (235, 235))
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=5, num_snapshots=2)
    lc.lift_tweak(feed, FRANKA_PANDA.body_names.index(lc.EE_BODY), torch.Generator().manual_seed(5))
    env = ManagerBasedRLEnv(lc.load_fixture(), state_feed=feed, noise_seed=11)
    env.reset()
    assert env.plan.processed_action_dim != env.plan.action_dim == lc.A  # the binary joint term
    torch.manual_seed(5)
    pol = ActorCritic(Dp, Dc, lc.A, actor_hidden_dims=[128, 64], critic_hidden_dims=[96], init_noise_std=0.7).cuda()
    inf = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
    assert inf.ok and inf._wpk is not None and inf.two_inputs == (family != "shared")
    norms = None
    if family == "normalised":
        norms = [EmpiricalNormalization([D]).cuda() for D in (Dp, Dc)]
        for n in norms:
            n._mean.copy_(torch.randn(n._mean.shape) * 2.0)
            n._std.copy_(torch.rand(n._std.shape) + 0.5)
    check_act_variant(env, pol, inf, _input(N, Dp, False, 21), None if family == "shared" else _input(N, Dc, True, 22), None, norms, packed)
    # both gripper targets were commanded: the epilogue's binary path ran on either side of zero
    grip = env._processed_action[:, 7]
    assert bool((grip == 0).any()) and bool((grip > 0).any())
    env.close()


@pytest.mark.parametrize("packed", [True, False])
def test_binary_head_of_the_two_input_launch_on_32_row_tiles(packed):
    binary_head_on_32_row_tiles("two", packed)


# ------------------------------------------------------------------------------------------------ 3. the runner, kitchen fixture
STORAGE = ("observations", "privileged_observations", "actions", "actions_log_prob", "mu", "sigma", "values", "rewards", "dones")


def _after_two_collects(build, fuse: bool) -> dict:
    from isaaclab_amd.rsl_rl.ppo import FusedInference

    env, venv, runner = build()
    runner.fuse_launches = fuse
    runner.train_mode()
    gen = torch.Generator().manual_seed(9)
    ep = torch.randint(0, int(venv.max_episode_length), (env.num_envs,), generator=gen)
    ep[::7] = int(venv.max_episode_length) - 2  # time-outs inside the rollout
    venv.episode_length_buf = ep.cuda()
    assert runner._fusable()
    for _ in range(2):  # with use_graph the second collect is a replay
        runner.collect()
    torch.cuda.synchronize()
    # the two-input inference ran, on either path
    assert isinstance(runner._infer, FusedInference) and runner._infer.ok and runner._infer.two_inputs
    assert runner.privileged_obs_type == "critic"
    st = runner.alg.storage
    out = {k: getattr(st, k).clone() for k in STORAGE}
    out.update(action=env._action.clone(), prev_action=env._prev_action.clone(), processed=env._processed_action.clone(),
               cur_rew=runner._cur_reward_sum.clone(), cur_len=runner._cur_episode_length.clone(), last_obs=runner.last_obs.clone(),
               last_critic_obs=runner.last_critic_obs.clone(), ep_len=env.episode_length_buf.clone(), reset_ids=env.reset_env_ids.clone(),
               log_out=env._log_out.clone(), log_accum=runner._log_accum.clone(), critic_buf=env.obs_buf["critic"].clone())
    out["ep_stats"] = runner._ep_stats.clone()
    with torch.no_grad():  # the stored values are the critic's on the stored critic rows, the means the actor's on the policy rows
        pol = runner.alg.policy
        assert_close(st.values, pol.critic(st.privileged_observations.flatten(0, 1)).view(st.values.shape), 1e-4, "values = critic(critic rows)")
        assert_close(st.mu, pol.actor(st.observations.flatten(0, 1)).view(st.mu.shape), 1e-4, "mu = actor(policy rows)")
    env.close()
    return out


@pytest.mark.parametrize("case", ["64-eager", "64-graph", "2500-eager", "2500-graph"])
def test_runner_with_a_critic_group_takes_the_three_launch_step(case):
    """64 envs: the recorded feed, 16-row tiles.  2500 envs over a synthetic feed on the fixture's mesh: 32-row tiles with a ragged last
    one wherever two networks on 2500 rows get them (79 tiles x 2 x 2 > CUs)."""
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    n, mode = case.split("-")
    N = int(n)

    def build():
        torch.manual_seed(3)
        g = Golden(KITCHEN)
        mesh = g.mesh()
        if N == g.N:
            env, T = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"), terrain=mesh, noise_seed=11), 6  # 6 recorded snapshots
        else:
            ext = (float(np.abs(mesh[0][:, 0]).max()) - 2.0, float(np.abs(mesh[0][:, 1]).max()) - 2.0)
            feed = StateFeed(ROBOTS[g.fixture["robot"]], N, "cuda:0", seed=5, num_snapshots=4, extent_xy=ext)
            env, T = ManagerBasedRLEnv(g.fixture, state_feed=feed, terrain=mesh, noise_seed=11), 4
        venv = RslRlVecEnvWrapper(env)
        runner = OnPolicyRunner(venv, dict(g.fixture["agent"], num_steps_per_env=T), log_dir=None, device="cuda:0", use_graph=mode == "graph")
        Dp, Dc = g.meta["obs_group_dims"]
        assert (venv.num_obs, venv.num_privileged_obs) == (Dp, Dc) and Dp != Dc
        return env, venv, runner

    a, b = _after_two_collects(build, False), _after_two_collects(build, True)
    for k in a:
        if k != "ep_stats":
            assert torch.equal(a[k], b[k]), f"{k}: fused and split rollouts differ"
    assert_close(b["ep_stats"], a["ep_stats"], 1e-5, "finished-episode statistics (float atomics: order differs)")
    assert float(a["dones"].sum()) > 0 and float(a["privileged_observations"].abs().sum()) > 0 and float(a["log_accum"].abs().sum()) > 0
    assert torch.equal(b["last_critic_obs"], b["critic_buf"])


# ------------------------------------------------------------------------------------------------ 4. a binary joint term beside a critic group
@pytest.mark.parametrize("clip", [None, 1.0e-30])
def test_binary_joint_term_beside_a_critic_group(clip):
    """Lift-Cube with a ``critic`` group (the policy group plus one more term): a 4-step rollout at N = 257, split against fused, as in
    tests/test_lift_gpu.py -- the ``_binary`` kernels of the two-input launch."""
    import _lift_cases as lc
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.rsl_rl.ppo import FusedInference
    from isaaclab_amd.state_feed import StateFeed

    fx = copy.deepcopy(lc.load_fixture())
    groups = fx["env"]["observations"]
    groups["critic"] = copy.deepcopy(groups["policy"])
    groups["critic"]["joint_pos_again"] = copy.deepcopy(groups["policy"]["joint_pos"])
    hand = FRANKA_PANDA.body_names.index(lc.EE_BODY)
    out = {}
    for fuse in (False, True):
        torch.manual_seed(3)
        feed = StateFeed(FRANKA_PANDA, 257, "cuda:0", seed=5, num_snapshots=4)
        lc.lift_tweak(feed, hand, torch.Generator().manual_seed(5))
        env = ManagerBasedRLEnv(fx, state_feed=feed, noise_seed=11)
        venv = RslRlVecEnvWrapper(env, clip_actions=clip)
        runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=True)
        runner.fuse_launches = fuse
        runner.train_mode()
        assert runner._fusable() and runner.privileged_obs_type == "critic"
        assert env.plan.processed_action_dim != env.plan.action_dim  # the binary joint term
        for _ in range(2):
            runner.collect()
        torch.cuda.synchronize()
        assert isinstance(runner._infer, FusedInference) and runner._infer.ok and runner._infer.two_inputs
        st = runner.alg.storage
        assert st.privileged_observations.shape == (4, 257, venv.num_obs + 9)
        out[fuse] = {k: getattr(st, k).cpu() for k in STORAGE}
        out[fuse].update(action=env._action.cpu(), prev_action=env._prev_action.cpu(), processed=env._processed_action.cpu(),
                         reset=env.reset_buf.cpu(), last_obs=runner.last_obs.cpu(), last_critic_obs=runner.last_critic_obs.cpu())
        env.close()
    a, b = out[False], out[True]
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: fused and split rollouts differ"
    keep = ~a["reset"]
    raw = a["action"][keep][:, 7:8]
    targets = torch.where(raw < 0, torch.zeros_like(raw), torch.full_like(raw, float(np.float32(0.04))))
    assert torch.equal(a["processed"][keep][:, 7:9], targets.expand(int(keep.sum()), 2))
    sampled = a["actions"][-1][keep][:, 7]
    assert bool((sampled < 0).any()) and bool((sampled > 0).any())
    # the critic group's extra term repeats the group's first nine columns (joint_pos_rel of the nine Franka joints)
    assert torch.equal(a["privileged_observations"][..., -9:], a["privileged_observations"][..., :9])
