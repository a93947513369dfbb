"""GPU: the fused rollout of an agent with ``empirical_normalization``.

1. ``EmpiricalNormalization.update_rows`` (``imx_empirical_normalization_update``: slab moments + finalize) followed by ``apply``
   against the float64 restatement, under ``_util.check_normalizer_step``'s rule and with ``_producer_cases.normalizer_case``'s input
   recipe; the slab cap, a pitched input, two groups in one call, the exact int64 count;
2. the ``until`` gate, taken on the device;
3. ``imx_mlp_infer_act2n`` on raw rows against ``apply`` + the existing launch, bit for bit (plain and with ``ImxPolicyAct``; 16- and
   32-row tiles, packed and row-layout weights, a null triple, a pitched input; the ``_binary`` epilogues through the Lift fixture), and
   one normalised forward against the float64 modules;
4. the runner: the five-launch step (``fuse_launches`` True) against the split comparator, eager and captured;
5. the runner's stored rows against the float64 restatement fed the raw rows of every step;
6. ``until`` reached inside a captured rollout;
7. the Repose fixture with its shipped agent cfg: captured = eager, ``learn(1)``;
8. ``fuse_normalization = False`` is the Python rollout; a checkpoint travels between the two.

A captured runner's first ``collect`` runs the rollout twice (the eager warm-up, then the first replay): two collects of a captured
runner are three rollouts, and are compared with three collects of an eager one (as tests/test_inhand_gpu.py does)."""

import copy
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _util import FLOAT_TOL, KITCHEN, Golden, assert_close, check_normalizer_step
from test_infer_two_inputs_gpu import STORAGE, _first32

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLAT = "Isaac-Velocity-Flat-Anymal-C-v0"


# ------------------------------------------------------------------------------------------------ 1. statistics against fp64
def _columns(D, g):
    """``normalizer_case``'s columns: |mean| up to 1e3, std down to 1e-2, column 0 pinned at 1e3 / 1e-2."""
    mu = torch.sign(torch.randn(D, generator=g)) * 10.0 ** (torch.rand(D, generator=g) * 4.0 - 1.0)
    sd = 10.0 ** (torch.rand(D, generator=g) * 2.5 - 2.0)
    mu[0], sd[0] = 1.0e3, 1.0e-2
    return mu, sd


def _on_gpu(x, pad):
    """The batch on the device; ``pad`` > 0: rows of pitch D + pad with NaN in the pad columns."""
    if not pad:
        return x.cuda()
    xb = torch.full((x.shape[0], x.shape[1] + pad), float("nan"))
    xb[:, :x.shape[1]] = x
    return xb.cuda()[:, :x.shape[1]]


def _statistics_case(D, batches, seed, pad=0):
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
    from oracle.rsl_rl_oracle import EmpiricalNormalizationOracle

    g = torch.Generator().manual_seed(seed)
    mu, sd = _columns(D, g)
    norm = EmpiricalNormalization([D]).cuda()
    o64, o32 = EmpiricalNormalizationOracle(D), EmpiricalNormalizationOracle(D)
    o64.mean, o64.var, o64.std = (t.to(F64) for t in (o64.mean, o64.var, o64.std))
    for k, N in enumerate(batches):
        x = (mu + sd * torch.randn(N, D, generator=g)).float()
        xg = _on_gpu(x, pad)
        assert xg.stride(0) == D + pad
        assert norm.update_rows(xg) is None
        out = norm.apply(xg)
        check_normalizer_step(norm, out, o64, o32, x, f"update_rows + apply D={D} batch {k} (N={N})")
    assert norm.count.dtype == torch.int64 and int(norm.count) == o64.count == sum(batches) == norm._host_count
    return norm


@pytest.mark.parametrize("D", [1, 64, 65, 235])
def test_statistics_against_float64(D):
    _statistics_case(D, (1, 2, 63, 64, 65, 4097), seed=700 + D)
    _statistics_case(D, (4097, 65, 1), seed=800 + D)


def test_statistics_at_the_slab_cap():
    """100 003 rows: 64 slabs of 1563 rows (the last one shorter), then a small batch onto the large count."""
    _statistics_case(65, (100003, 17), seed=901)


def test_statistics_of_a_pitched_input():
    _statistics_case(65, (65, 4097, 2), seed=902, pad=3)


def test_two_groups_in_one_call_equal_two_calls():
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization, update_rows_together

    g = torch.Generator().manual_seed(903)
    shapes = ((4097, 235), (65, 64))  # (different row counts as well: each group has its own slabs)
    xs = []
    for N, D in shapes:
        mu, sd = _columns(D, g)
        xs.append([(mu + sd * torch.randn(n, D, generator=g)).float().cuda() for n in (N, 33)])
    pair = [EmpiricalNormalization([D]).cuda() for _, D in shapes]
    single = [EmpiricalNormalization([D]).cuda() for _, D in shapes]
    for k in range(2):
        update_rows_together((pair[0], xs[0][k]), (pair[1], xs[1][k]))
        for n, x in zip(single, xs):
            n.update_rows(x[k])
    torch.cuda.synchronize()
    for a, b, (N, _) in zip(pair, single, shapes):
        for name in ("_mean", "_var", "_std", "count"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert int(a.count) == N + 33 == a._host_count == b._host_count
        assert float(a._mean.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ 2. until
def test_until_is_taken_on_the_device():
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization

    norm = EmpiricalNormalization([7], until=5).cuda()
    g = torch.Generator().manual_seed(5)
    seen = []
    for k in range(3):
        before = [t.clone() for t in (norm._mean, norm._var, norm._std, norm.count)]
        norm.update_rows(torch.randn(4, 7, generator=g).cuda() * 3.0 + 1.0)
        torch.cuda.synchronize()
        same = [torch.equal(a, b) for a, b in zip(before, (norm._mean, norm._var, norm._std, norm.count))]
        seen.append(int(norm.count))
        assert norm._host_count == int(norm.count)
        assert all(same) if k == 2 else not any(same), (k, same)
    assert seen == [4, 8, 8]


# ------------------------------------------------------------------------------------------------ 3. the normalising launch
WIDTHS = [(48, 48, True), (235, 239, False), (5, 512, False)]  # (policy width, critic width, shared input)
_built: dict = {}


def _stacks(i):
    if i not in _built:
        from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
        from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
        from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

        Dp, Dc, shared = WIDTHS[i]
        torch.manual_seed(300 + i)
        pol = ActorCritic(Dp, Dc, 12, actor_hidden_dims=[128, 64], critic_hidden_dims=[96, 32], init_noise_std=0.7).cuda()
        inf = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
        assert inf.ok and inf.two_inputs == (not shared) and inf._wpk is not None
        norms = []
        for D in (Dp, Dc):
            n = EmpiricalNormalization([D]).cuda()
            n._mean.copy_(torch.randn(1, D) * 2.0)
            n._std.copy_(torch.rand(1, D) + 0.5)
            norms.append(n)
        _built[i] = (pol, inf, norms)
    return _built[i]


def _rows(spec):
    return spec if isinstance(spec, int) else _first32(2) + (31 if spec.endswith("+31") else 0)


def _raw(M, D, seed, pad):
    g = torch.Generator().manual_seed(seed)
    return _on_gpu(torch.randn(M, D, generator=g) * 3.0, pad)


def _launch(inf, x, cx, shared, packed, norm, with_act, std):
    """One inference launch into fresh sentinel buffers (40 rows past M: a ragged last tile must not reach them)."""
    from isaaclab_amd import _lib

    M, A = x.shape[0], inf.out_features[0]
    S = lambda *sh: torch.full((M + 40, *sh), -7777.0, device="cuda")  # noqa: E731
    o = dict(mu=S(A), values=S(1), actions=S(A), logp=S(), sigma=S(A), obs=S(x.shape[1]), cobs=S(cx.shape[1]))
    act = None
    if with_act:
        stp = torch.tensor([3], dtype=torch.int32, device="cuda")
        act = _lib.ImxPolicyAct(std_d=std.data_ptr(), seed=99, step_counter_d=stp.data_ptr(), actions_out_d=o["actions"].data_ptr(),
                                logp_out_d=o["logp"].data_ptr(), mu_out_d=o["mu"].data_ptr(), sigma_out_d=o["sigma"].data_ptr(),
                                obs_out_d=o["obs"].data_ptr(), plan=None, state=None, buf=None, pre_clip=math.inf)
    kw = {} if shared else dict(critic_x=cx, critic_obs_out=o["cobs"][:M] if with_act else None)
    keep = inf._wpk
    if not packed:
        inf._wpk = None
    try:
        inf(x, None if with_act else o["mu"][:M], o["values"][:M], act=act, norm=norm, **kw)
    finally:
        inf._wpk = keep
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v[M:] == -7777.0).all()), f"{k}: rows beyond M were written"
    return {k: v[:M] for k, v in o.items()}


@pytest.mark.parametrize("rows", [33, "first32", "first32+31"])
@pytest.mark.parametrize("widths", range(len(WIDTHS)))
def test_normalising_launch_equals_apply_then_the_existing_launch(widths, rows):
    Dp, Dc, shared = WIDTHS[widths]
    M = _rows(rows)
    pol, inf, (pn, cn) = _stacks(widths)
    pad = 5 if widths == 1 else 0
    x = _raw(M, Dp, 40 * widths + 1, pad)
    cx = x if shared else _raw(M, Dc, 40 * widths + 2, pad)
    cnorm = pn if shared else cn  # (no critic group: the policy statistics for both networks)
    xn, cxn = pn.apply(x), (pn.apply(x) if shared else cn.apply(cx))
    for packed in ((True, False) if M >= _first32(2) else (True,)):
        for with_act in (False, True):
            ref = _launch(inf, xn, cxn, shared, packed, None, with_act, pol.std)
            got = _launch(inf, x, cx, shared, packed, (pn, cnorm), with_act, pol.std)
            keys = ("values", "mu") + (("actions", "logp", "sigma", "obs") + (() if shared else ("cobs",)) if with_act else ())
            for k in keys:
                assert torch.equal(ref[k], got[k]), f"{k}: packed={packed} act={with_act}"
                assert bool(torch.isfinite(got[k]).all()) and not bool((got[k] == -7777.0).all()), k
            if with_act:
                assert torch.equal(got["obs"], xn) and (shared or torch.equal(got["cobs"], cxn))
    if not shared:  # one null triple: that network reads its rows as they are
        ref = _launch(inf, xn, cx, shared, True, None, True, pol.std)
        got = _launch(inf, x, cx, shared, True, (pn, None), True, pol.std)
        for k in ref:
            assert torch.equal(ref[k], got[k]), f"{k}: null critic triple"
        assert torch.equal(got["cobs"], cx.contiguous())
        ref = _launch(inf, x, cxn, shared, True, None, True, pol.std)
        got = _launch(inf, x, cx, shared, True, (None, cn), True, pol.std)
        for k in ref:
            assert torch.equal(ref[k], got[k]), f"{k}: null policy triple"


def test_normalised_forward_against_float64():
    """(33, 235): the bound of the existing float64 inference test (tests/test_infer_two_inputs_gpu.py), on the normalised rows."""
    pol, inf, (pn, cn) = _stacks(1)
    Dp, Dc, _ = WIDTHS[1]
    x, cx = _raw(33, Dp, 61, 5), _raw(33, Dc, 62, 5)
    got = _launch(inf, x, cx, False, True, (pn, cn), False, pol.std)
    p64 = copy.deepcopy(pol).double()
    n64 = lambda n, v: (v.double() - n._mean.double()) / (n._std.double() + n.eps)  # noqa: E731
    with torch.no_grad():
        assert_close(got["mu"], p64.actor(n64(pn, x)), FLOAT_TOL, "mu")
        assert_close(got["values"], p64.critic(n64(cn, cx)), FLOAT_TOL, "value")


# ------------------------------------------------------------------------------------------------ 4. the runner, fused = split
def _norm_state(runner):
    out = {}
    for tag, n in (("obs_norm", runner.obs_normalizer), ("priv_norm", runner.privileged_obs_normalizer)):
        out.update({f"{tag}/{k}": getattr(n, k).clone() for k in ("_mean", "_var", "_std", "count")})
    return out


def _collect(build, fuse, collects, until=None, fuse_normalization=True):
    """``collects`` collects of a fresh runner; storage, last rows, env buffers and both normalisers' statistics."""
    env, venv, runner = build()
    runner.fuse_launches = fuse
    runner.fuse_normalization = fuse_normalization
    runner.train_mode()
    if until is not None:
        runner.obs_normalizer.until = until
    gen = torch.Generator().manual_seed(9)
    ep = torch.randint(0, int(venv.max_episode_length), (env.num_envs,), generator=gen)
    ep[::7] = int(venv.max_episode_length) - 2  # time-outs inside the rollout
    venv.episode_length_buf = ep.cuda()
    assert not runner._fusable() and runner._fusable_normalized()
    for _ in range(collects):
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    out = {k: getattr(st, k).clone() for k in STORAGE if getattr(st, k) is not None}
    out.update(last_obs=runner.last_obs.clone(), last_critic_obs=runner.last_critic_obs.clone(), action=env._action.clone(),
               processed=env._processed_action.clone(), cur_rew=runner._cur_reward_sum.clone(), log_accum=runner._log_accum.clone())
    out.update(_norm_state(runner))
    out["ep_stats"] = runner._ep_stats.clone()
    info = dict(host=(runner.obs_normalizer._host_count, runner.privileged_obs_normalizer._host_count), priv=runner.privileged_obs_type,
                T=runner.num_steps_per_env, N=env.num_envs, infer=runner._infer)
    env.close()
    return out, info


def _builder(case):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    task, n, mode = case.split(":")
    N = int(n)

    def build():
        torch.manual_seed(3)
        g = Golden(KITCHEN if task == "kitchen" else FLAT)
        mesh = g.mesh()
        if N == g.N:
            env, T = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"), terrain=mesh, noise_seed=11), (6 if task == "kitchen" else 4)
        else:
            ext = (float(np.abs(mesh[0][:, 0]).max()) - 2.0, float(np.abs(mesh[0][:, 1]).max()) - 2.0)
            feed = StateFeed(ROBOTS[g.fixture["robot"]], N, "cuda:0", seed=5, num_snapshots=4, extent_xy=ext)
            env, T = ManagerBasedRLEnv(g.fixture, state_feed=feed, terrain=mesh, noise_seed=11), 4
        venv = RslRlVecEnvWrapper(env)
        cfg = dict(g.fixture["agent"], num_steps_per_env=T, empirical_normalization=True)
        return env, venv, OnPolicyRunner(venv, cfg, log_dir=None, device="cuda:0", use_graph=mode == "graph")

    return build, mode


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if k != "ep_stats":
            assert torch.equal(a[k], b[k]), f"{k}: {what}"
    assert_close(b["ep_stats"], a["ep_stats"], 1e-5, "finished-episode statistics (float atomics: order differs)")


@pytest.mark.parametrize("case", ["flat:64:eager", "flat:64:graph", "kitchen:64:eager", "kitchen:64:graph", "kitchen:2500:eager", "kitchen:2500:graph"])
def test_runner_five_launch_step_equals_the_split_comparator(case):
    """Flat Anymal-C at 64 envs: shared input, 16-row tiles.  The kitchen config: a critic group; 16-row tiles at 64 envs, ragged 32-row
    tiles at 2500."""
    from isaaclab_amd.rsl_rl.ppo import FusedInference

    build, mode = _builder(case)
    (a, ia), (b, ib) = _collect(build, False, 2), _collect(build, True, 2)
    _assert_same(a, b, "fused and split normalised rollouts differ")
    rollouts = 3 if mode == "graph" else 2  # (module docstring)
    for out, info in ((a, ia), (b, ib)):
        T, N = info["T"], info["N"]
        assert isinstance(info["infer"], FusedInference) and info["infer"].ok and info["infer"].two_inputs == (info["priv"] is not None)
        assert out["obs_norm/count"].dtype == torch.int64 and int(out["obs_norm/count"]) == T * N * rollouts == info["host"][0]
        assert int(out["priv_norm/count"]) == (T * N * rollouts if info["priv"] is not None else 0) == info["host"][1]
        if info["priv"] is None:
            assert "privileged_observations" not in out and torch.equal(out["last_obs"], out["last_critic_obs"])
            assert bool((out["priv_norm/_mean"] == 0).all()) and bool((out["priv_norm/_var"] == 1).all())
        else:
            assert float(out["privileged_observations"].abs().sum()) > 0 and float(out["priv_norm/_mean"].abs().sum()) > 0
        assert float(out["dones"].sum()) > 0 and float(out["obs_norm/_mean"].abs().sum()) > 0 and float(out["log_accum"].abs().sum()) > 0
        assert bool(torch.isfinite(out["observations"]).all())


@pytest.mark.parametrize("N", [257, "first32+31"])
def test_binary_epilogues_of_the_normalising_launch(N):
    """Lift-Cube (a binary joint term) with a ``critic`` group, as tests/test_infer_two_inputs_gpu.py builds it: 257 envs run the
    16-row ``_binary`` kernel, the first 32-row count + 31 the 32-row one."""
    import _lift_cases as lc
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    N = _rows(N)
    fx = copy.deepcopy(lc.load_fixture())
    groups = fx["env"]["observations"]
    groups["critic"] = copy.deepcopy(groups["policy"])
    groups["critic"]["joint_pos_again"] = copy.deepcopy(groups["policy"]["joint_pos"])
    hand = FRANKA_PANDA.body_names.index(lc.EE_BODY)

    def build():
        torch.manual_seed(3)
        feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=5, num_snapshots=4)
        lc.lift_tweak(feed, hand, torch.Generator().manual_seed(5))
        env = ManagerBasedRLEnv(fx, state_feed=feed, noise_seed=11)
        venv = RslRlVecEnvWrapper(env)
        runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=4, empirical_normalization=True), log_dir=None, device="cuda:0", use_graph=True)
        assert env.plan.processed_action_dim != env.plan.action_dim  # the binary joint term
        return env, venv, runner

    (a, ia), (b, ib) = _collect(build, False, 2), _collect(build, True, 2)
    _assert_same(a, b, "fused and split normalised rollouts differ")
    assert ib["priv"] == "critic" and int(b["obs_norm/count"]) == 4 * N * 3 == int(b["priv_norm/count"])


def test_binary_epilogue_of_the_normalising_launch_on_row_layout_weights():
    """The runner above reads packed weights: ``k_mlp_infer2n_binary<false>`` at 2081 rows against ``apply`` + the plain launch +
    ``imx_policy_act`` + the action terms."""
    from test_infer_two_inputs_gpu import binary_head_on_32_row_tiles

    binary_head_on_32_row_tiles("normalised", False)


# ------------------------------------------------------------------------------------------------ 5. the runner against fp64
def test_runner_rows_against_the_float64_restatement():
    """The eager split path on flat Anymal-C: every step's raw rows (kept by a wrapper around ``update_rows``) through the restatement
    in float64 and fp32; the rows the next step stored are the normalised ones, under the normaliser's rule."""
    from oracle.rsl_rl_oracle import EmpiricalNormalizationOracle

    build, _ = _builder("flat:64:eager")
    env, venv, runner = build()
    runner.fuse_launches = False
    runner.train_mode()
    norm = runner.obs_normalizer
    raw, stats = [], []
    inner = norm.update_rows

    def keeping(x, **kw):
        inner(x, **kw)
        raw.append(x.clone())
        stats.append(types.SimpleNamespace(_mean=norm._mean.clone(), _var=norm._var.clone(), _std=norm._std.clone(), eps=norm.eps))

    norm.update_rows = keeping
    first = venv.get_observations()[0].clone()
    assert not runner._fusable() and runner._fusable_normalized()
    D = first.shape[1]
    o64, o32 = EmpiricalNormalizationOracle(D), EmpiricalNormalizationOracle(D)
    o64.mean, o64.var, o64.std = (t.to(F64) for t in (o64.mean, o64.var, o64.std))
    T = runner.num_steps_per_env
    for c in range(2):
        raw.clear(), stats.clear()
        start = runner.last_obs.clone() if c else first
        runner.collect()
        torch.cuda.synchronize()
        st = runner.alg.storage
        assert len(raw) == T
        assert torch.equal(st.observations[0], start)  # the first rollout's step 0 is raw; afterwards the last rollout's normalised last rows
        for t in range(T):
            out = st.observations[t + 1] if t + 1 < T else runner.last_obs
            check_normalizer_step(stats[t], out, o64, o32, raw[t].cpu(), f"collect {c} step {t}")
    assert int(norm.count) == o64.count == 2 * T * 64
    env.close()


# ------------------------------------------------------------------------------------------------ 6. until inside a captured rollout
def test_until_inside_a_captured_rollout():
    """``until`` = 5 batches of 64 rows, T = 4: the gate closes after the first step of the second rollout, inside the captured graph
    on its first replay.  Captured (two collects), eager and split (three) agree on everything."""
    until = 5 * 64
    (g, ig) = _collect(_builder("flat:64:graph")[0], True, 2, until=until)
    (e, ie) = _collect(_builder("flat:64:eager")[0], True, 3, until=until)
    (s, i_s) = _collect(_builder("flat:64:eager")[0], False, 3, until=until)
    _assert_same(e, g, "captured and eager differ")
    _assert_same(s, e, "fused and split differ")
    for out, info in ((g, ig), (e, ie), (s, i_s)):
        assert int(out["obs_norm/count"]) == until == info["host"][0] and info["T"] == 4
    free, _ = _collect(_builder("flat:64:eager")[0], True, 3)
    assert int(free["obs_norm/count"]) == 12 * 64 and not torch.equal(free["obs_norm/_mean"], e["obs_norm/_mean"])


# ------------------------------------------------------------------------------------------------ 7. the Repose fixture
def _repose(use_graph):
    import _inhand_cases as ic
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import ALLEGRO_HAND
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    fx = ic.load_fixture(ic.TASK)
    assert fx["agent"]["empirical_normalization"] is True
    torch.manual_seed(23)
    feed = StateFeed(ALLEGRO_HAND, 64, "cuda:0", seed=23, num_snapshots=3)
    ic.inhand_tweak(feed, torch.Generator().manual_seed(23))
    u = ManagerBasedRLEnv(fx, state_feed=feed, seed=23, noise_seed=23)
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=3), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    assert not runner._fusable() and runner._fusable_normalized()
    u.episode_length_buf[::5] = int(u.max_episode_length) - 2
    for _ in range(2 if use_graph else 3):
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    out = {k: getattr(st, k).clone() for k in STORAGE if getattr(st, k) is not None}
    out.update(_norm_state(runner), last_obs=runner.last_obs.clone(), processed=u._processed_action.clone())
    return out, runner, env


def test_repose_fixture_with_its_shipped_agent_cfg():
    a, ra, ea = _repose(True)
    ea.close()
    c, rc, ec = _repose(False)
    for k in a:
        assert bool(torch.isfinite(a[k].float()).all()), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert int(c["obs_norm/count"]) == 3 * 3 * 64 == rc.obs_normalizer._host_count == ra.obs_normalizer._host_count
    assert float(a["dones"].sum()) > 0 and float(a["obs_norm/_mean"].abs().sum()) > 0
    rc.learn(1)
    torch.cuda.synchronize()
    s = rc.alg.loss_dict()
    assert all(np.isfinite(v) for v in s.values()), s
    assert int(rc.obs_normalizer.count) == 4 * 3 * 64 == rc.obs_normalizer._host_count
    ec.close()


# ------------------------------------------------------------------------------------------------ 8. the switch, and checkpoints
def test_fuse_normalization_off_is_the_python_rollout_and_checkpoints_travel(tmp_path):
    build, _ = _builder("flat:64:eager")
    calls = {}
    runners = {}
    for fuse in (True, False):
        env, venv, runner = build()
        runner.fuse_normalization = fuse
        runner.train_mode()
        inner = runner.obs_normalizer.forward
        calls[fuse] = 0

        def counting(x, inner=inner, fuse=fuse):
            calls[fuse] += 1
            return inner(x)

        runner.obs_normalizer.forward = counting
        runner.collect()
        torch.cuda.synchronize()
        runners[fuse] = (env, runner)
    T = runners[True][1].num_steps_per_env
    assert calls == {True: 0, False: T}
    fused, python = runners[True][1], runners[False][1]
    assert int(fused.obs_normalizer.count) == T * 64 == int(python.obs_normalizer.count)
    assert fused._infer is not None and python._infer is None  # (the Python rollout goes through alg.act)
    fused.collect()
    ck = str(tmp_path / "model.pt")
    fused.save(ck)
    python.load(ck)
    for name in ("obs_normalizer", "privileged_obs_normalizer"):
        for k in ("_mean", "_var", "_std", "count"):
            assert torch.equal(getattr(getattr(fused, name), k), getattr(getattr(python, name), k)), (name, k)
    assert python.obs_normalizer._host_count == 2 * T * 64 == fused.obs_normalizer._host_count
    python.alg.storage.clear()  # (the Python rollout appends: upstream clears in update())
    python.collect()
    torch.cuda.synchronize()
    assert calls[False] == 2 * T and int(python.obs_normalizer.count) == 3 * T * 64
    for env, _ in runners.values():
        env.close()
