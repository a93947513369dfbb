"""GPU: the PPO update and the rollout inference at every policy shape the reference's agent cfgs ship, against float64 references.

The per-kernel parity tests (test_kernels_gpu.py) and the whole-update tests run toy networks.  Here the COMPOSED update
(``PPO.minibatch_step``: imx_mlp_fwd_elu, imx_mlp_dw[_elu], the imx_mlp_head_* family, imx_ppo_loss_*, library GEMMs between them)
runs at the batch sizes the tasks train with (4096 envs x num_steps_per_env / num_mini_batches = 24 576 rows), on minibatches drawn
through the storage's own permutation / gather (the row-pitched observation buffers), and the rollout (imx_mlp_infer_act) at 4096 envs.

Tolerances (tests/_util.py): gradients per parameter tensor within max(1e-5 * max|g_ref|, 2 * e_torch) of float64 autograd, where e_torch
is fp32 torch autograd's own error against the same reference; forward outputs (mu, values, log-probs) within ``assert_close`` (1e-5,
relative above |x| = 1); the packed / row-layout, fused / split and graph / eager comparisons bit for bit.
"""

import copy

import numpy as np
import pytest
import torch

from _util import (FLOAT_TOL, assert_close, check_fused_inference, check_infer_act, check_minibatch_gradients, fill_storage,
                   reference_update, update_params_agree)

pytestmark = pytest.mark.gpu

NUM_ENVS = 4096

# The five tasks of isaaclab_amd/configs (hidden dims, num_steps_per_env and num_mini_batches come from their agent cfgs, D and A from the
# compiled plan): rough locomotion [512, 256, 128] (rough Anymal-C, rough G1, flat Spot), flat locomotion [128, 128, 128] (flat Anymal-C),
# Cartpole [32, 32].
TASKS = ("Isaac-Cartpole-v0", "Isaac-Velocity-Flat-Anymal-C-v0", "Isaac-Velocity-Flat-Spot-v0", "Isaac-Velocity-Rough-Anymal-C-v0",
         "Isaac-Velocity-Rough-G1-v0")

# The other policy shapes of the reference's agent cfgs (source/isaaclab_tasks/isaaclab_tasks/<path>/agents/rsl_rl_ppo_cfg.py).  No task
# here runs them: D and A are REPRESENTATIVE odd widths, not the tasks' exact observation / action widths.
# name: (actor hidden dims, critic hidden dims, D, A)
OTHER_SHAPES = {
    # manager_based/classic/humanoid, manager_based/classic/ant (also direct/humanoid, direct/ant)
    "classic-400-200-100": ([400, 200, 100], [400, 200, 100], 87, 21),
    # manager_based/locomotion/velocity/config/g1 (flat cfg)
    "g1-flat-256-128-128": ([256, 128, 128], [256, 128, 128], 123, 37),
    # manager_based/manipulation/lift/config/franka, manager_based/manipulation/cabinet/config/franka (also direct/franka_cabinet)
    "manip-256-128-64": ([256, 128, 64], [256, 128, 64], 60, 8),
    # manager_based/navigation/config/anymal_c
    "nav-128-128": ([128, 128], [128, 128], 36, 8),
    # manager_based/manipulation/reach/config/franka, manager_based/manipulation/reach/config/ur_10
    "reach-64-64": ([64, 64], [64, 64], 32, 7),
    # manager_based/classic/cartpole, direct/cartpole
    "cartpole-32-32": ([32, 32], [32, 32], 5, 1),
}
# Direct-workflow shapes that do not fit imx_mlp_infer (5 Linear layers, or wider than 512): FusedInference reports ok = False and the
# rollout / update take the library path.  D, A representative as above.
DIRECT_SHAPES = {
    "allegro-1024-512-256-128": ([1024, 512, 256, 128], [1024, 512, 256, 128], 124, 16),  # direct/allegro_hand
    "shadow-512-512-256-128": ([512, 512, 256, 128], [512, 512, 256, 128], 157, 20),  # direct/shadow_hand (PPO cfg)
    "shadow-ff-400-400-200-100": ([400, 400, 200, 100], [512, 512, 256, 128], 157, 20),  # direct/shadow_hand (OpenAI FF cfg)
    "shadow-lstm-1024-512-512-256-128": ([1024, 512, 512, 256, 128], [1024, 512, 512, 256, 128], 157, 20),  # direct/shadow_hand (OpenAI LSTM cfg)
}
ODD_SHAPE = OTHER_SHAPES["classic-400-200-100"]  # every ragged path: widths 400 / 200 / 100, a stacked 800-wide first layer, K = 100 heads


def _task(task):
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS

    fx = load_task_cfg(task)
    plan = compile_plan(fx["env"], ROBOTS[fx["robot"]])
    return fx, plan.obs_dim, plan.action_dim


def _alg_kw(agent):
    return {k: v for k, v in agent["algorithm"].items() if k != "class_name"}


def _ppo(D, A, actor_hidden, critic_hidden, agent, activation="elu", seed=0):
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    torch.manual_seed(seed)
    pol = ActorCritic(D, D, A, actor_hidden_dims=list(actor_hidden), critic_hidden_dims=list(critic_hidden), activation=activation,
                      init_noise_std=agent["policy"]["init_noise_std"], noise_std_type=agent["policy"]["noise_std_type"])
    return PPO(pol, device="cuda:0", **_alg_kw(agent))


def _head_variants(alg):
    """FUSED_HEAD settings that change the code path: "1" only where imx_mlp_head_fwd_bwd takes an output layer (128 / 256 in-features)."""
    from isaaclab_amd.rsl_rl.ppo import HEAD_MAX_OUT

    takes = any(layers[-1][0].in_features in (128, 256) and layers[-1][0].out_features <= min(16, HEAD_MAX_OUT)
                for layers in (alg._actor_layers, alg._critic_layers))
    return ("0", "1") if takes else ("0",)


def _gradient_parity(monkeypatch, alg, T, nmb, what, seed=1):
    """Minibatch 0 of a fresh permutation of a seeded storage, through the storage's own draw / gather; one minibatch_step per stream /
    head configuration, each against float64 autograd."""
    import isaaclab_amd.rsl_rl.ppo as ppo_mod

    alg.init_storage("rl", NUM_ENVS, T, (alg.policy.actor[0].in_features,), (0,), (alg.policy.actor[-1].out_features,))
    fill_storage(alg, seed)
    torch.manual_seed(seed)
    alg.storage.draw_permutation(nmb)
    batch = alg.storage.gather_minibatch(0, nmb)
    assert batch[0].shape[0] == NUM_ENVS * T // nmb
    for two_streams in (True, False):
        for fused_head in _head_variants(alg):
            monkeypatch.setattr(ppo_mod, "FUSED_HEAD", fused_head)
            alg.two_streams = two_streams
            check_minibatch_gradients(alg, batch, f"{what} two_streams={two_streams} FUSED_HEAD={fused_head}")


# ---------------------------------------------------------------------------------------------------- 1. gradients at the task shapes
@pytest.mark.parametrize("task", TASKS)
def test_update_gradient_at_task_shapes(monkeypatch, task):
    fx, D, A = _task(task)
    agent = fx["agent"]
    hidden = agent["policy"]["actor_hidden_dims"], agent["policy"]["critic_hidden_dims"]
    alg = _ppo(D, A, *hidden, agent, activation=agent["policy"]["activation"])
    if task == "Isaac-Velocity-Rough-Anymal-C-v0":
        assert (D, A) == (235, 12)
    if task == "Isaac-Velocity-Rough-G1-v0":
        assert (D, A) == (310, 37)
    _gradient_parity(monkeypatch, alg, int(agent["num_steps_per_env"]), int(agent["algorithm"]["num_mini_batches"]), task)


# ---------------------------------------------------------------------------------------------------- 2. the whole update, rough Anymal-C
ROUGH = "Isaac-Velocity-Rough-Anymal-C-v0"


def test_update_graph_replay_equals_eager_update_at_rough_anymal_c():
    """PPO.update as one hipGraph replay against the eager update at 4096 envs x 24 steps, 5 epochs x 4 minibatches: parameters, Adam
    moments, learning rate and logged losses bit for bit over six updates (test_update_graph_replay_equals_eager_update at task size)."""
    fx, D, A = _task(ROUGH)
    agent = fx["agent"]
    T = int(agent["num_steps_per_env"])
    results = []
    for graph in (False, True):
        alg = _ppo(D, A, agent["policy"]["actor_hidden_dims"], agent["policy"]["critic_hidden_dims"], agent)
        alg.update_graph = graph
        alg.init_storage("rl", NUM_ENVS, T, (D,), (0,), (A,))
        torch.manual_seed(1234)
        stats = []
        for it in range(6):  # graph mode: eager, eager (timed), capture + replay, replay (timed), choice, chosen
            if graph and it == 4:
                alg._update_t = "graph"  # pin the choice: this test is about the equality
            fill_storage(alg, 100 + it)
            alg.update()
            stats.append(alg.loss_dict())
        torch.cuda.synchronize()
        assert (alg._update_g is not None) == graph
        results.append((alg.bucket.flat.clone(), alg.bucket.exp_avg.clone(), alg.bucket.exp_avg_sq.clone(), alg.learning_rate, stats))
    (p0, m0, v0, lr0, s0), (p1, m1, v1, lr1, s1) = results
    assert lr0 == lr1 and s0 == s1
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert bool(torch.isfinite(p1).all())


def test_whole_update_at_rough_anymal_c_matches_torch_reference():
    """One PPO.update (5 epochs x 4 minibatches of 24 576 rows) against torch autograd + Adam + the rsl_rl restatement on the same data
    and permutation, with the outlier-tolerant criterion of tools/fuzz_kernels.py::case_update."""
    fx, D, A = _task(ROUGH)
    agent = fx["agent"]
    kw = _alg_kw(agent)
    T, nmb, nep = int(agent["num_steps_per_env"]), int(kw["num_mini_batches"]), int(kw["num_learning_epochs"])
    alg = _ppo(D, A, agent["policy"]["actor_hidden_dims"], agent["policy"]["critic_hidden_dims"], agent)
    ref_pol = copy.deepcopy(alg.policy)
    alg.init_storage("rl", NUM_ENVS, T, (D,), (0,), (A,))
    fill_storage(alg, 7)
    st = alg.storage
    data = [x.flatten(0, 1).clone() for x in (st.observations, st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu,
                                              st.sigma, st.observations)]
    torch.manual_seed(99)
    alg.update()
    torch.cuda.synchronize()
    torch.manual_seed(99)
    perm = torch.randperm(NUM_ENVS * T // nmb * nmb, device="cuda:0")
    lr = reference_update(ref_pol, data, perm, nmb, nep, kw)
    assert abs(alg.learning_rate - lr) <= 1e-9 * max(1.0, lr), (alg.learning_rate, lr)
    ok, err, msg = update_params_agree(alg.policy, ref_pol, nep * nmb)
    assert ok, f"parameters after {nep * nmb} optimiser steps: err {err:.2e}; {msg}"


# ---------------------------------------------------------------------------------------------------- 3. rollout at the task shapes
def _runner(task, num_envs, use_graph=True, policy=None, seed=3):
    from bench import build_env
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    fx, env, _ = build_env(task, num_envs, torch.device("cuda:0"), seed, 4, (4, 4))
    agent = dict(fx["agent"])
    agent["policy"] = dict(agent["policy"], **(policy or {}))
    venv = RslRlVecEnvWrapper(env, clip_actions=agent.get("clip_actions"))
    torch.manual_seed(seed)
    runner = OnPolicyRunner(venv, agent, log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    g = torch.Generator().manual_seed(seed)
    venv.episode_length_buf = torch.randint(0, int(venv.max_episode_length), (num_envs,), generator=g).cuda()
    return runner


def _check_storage_against_fp64(runner, what):
    """Every slot of the rollout storage against the float64 policy: mu and values from the stored observations, sigma = std, the log-prob
    of the stored actions; the normalised action noise (a - mu) / sigma has mean ~0 and variance ~1 (a loose bound: it catches a wrong
    noise scale, not a wrong element)."""
    st, pol = runner.alg.storage, runner.alg.policy
    p64 = copy.deepcopy(pol).double()
    std64 = p64._std(torch.zeros(1, st.actions.shape[-1], dtype=torch.float64, device="cuda:0"))
    zs = []
    with torch.no_grad():
        for t in range(runner.num_steps_per_env):
            obs = st.observations[t].double()
            assert bool(torch.isfinite(obs).all()), f"{what}: observations[{t}]"
            mu64 = p64.actor(obs)
            assert_close(st.mu[t], mu64, FLOAT_TOL, f"{what}: mu[{t}]")
            assert_close(st.values[t], p64.critic(obs), FLOAT_TOL, f"{what}: values[{t}]")
            assert torch.equal(st.sigma[t], pol._std(st.mu[t])), f"{what}: sigma[{t}]"
            logp64 = torch.distributions.Normal(mu64, std64.expand_as(mu64)).log_prob(st.actions[t].double()).sum(-1, keepdim=True)
            assert_close(st.actions_log_prob[t], logp64, FLOAT_TOL, f"{what}: log-prob[{t}]")
            zs.append(((st.actions[t] - st.mu[t]) / st.sigma[t]).double().flatten())
    z = torch.cat(zs)
    n = z.numel()
    assert abs(float(z.mean())) < 6.0 / n ** 0.5, f"{what}: action noise mean {float(z.mean()):.4f} over {n} draws"
    assert abs(float(z.var()) - 1.0) < 6.0 * (2.0 / n) ** 0.5, f"{what}: action noise variance {float(z.var()):.4f} over {n} draws"


@pytest.mark.parametrize("task", TASKS)
def test_rollout_storage_against_fp64(task):
    """One fused collect() (warm-up, hipGraph capture, replay) at 4096 envs; the storage it leaves against the float64 policy."""
    runner = _runner(task, NUM_ENVS)
    assert runner._fusable() and runner.use_graph
    runner.collect()
    torch.cuda.synchronize()
    assert runner._infer.ok and runner._graph is not None
    _check_storage_against_fp64(runner, task)
    runner.env.unwrapped.close()


# ---------------------------------------------------------------------------------------------------- 4. the other shipped shapes
@pytest.mark.parametrize("shape", list(OTHER_SHAPES))
def test_fused_inference_at_shipped_shapes(shape):
    """FusedInference (imx_mlp_infer, 16- and 32-sample tiles, ragged last tile) against float64, and imx_mlp_infer_act against the
    split launches, at the policy shapes no task here runs."""
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic

    ah, ch, D, A = OTHER_SHAPES[shape]
    torch.manual_seed(len(shape))
    pol = ActorCritic(D, D, A, actor_hidden_dims=ah, critic_hidden_dims=ch, init_noise_std=0.7).cuda()
    for M in (1, 33, 2048, 4096 + 17):
        check_fused_inference(pol, M, seed=M, what=f"{shape} M={M}")
        check_infer_act(pol, M, seed=M + 1, step=M % 97, what=f"{shape} M={M}")


@pytest.mark.parametrize("shape", list(OTHER_SHAPES) + list(DIRECT_SHAPES))
def test_update_gradient_at_shipped_shapes(monkeypatch, shape):
    """Item 1's gradient parity at M = 24 576 (4096 envs x 24 steps / 4 minibatches) for the shapes of no task here; the direct-workflow
    shapes do not fit the fused inference (ok = False) and their update runs the library path everywhere it has to."""
    from isaaclab_amd.rsl_rl.ppo import FusedInference

    fx, _, _ = _task(ROUGH)
    ah, ch, D, A = {**OTHER_SHAPES, **DIRECT_SHAPES}[shape]
    alg = _ppo(D, A, ah, ch, fx["agent"])
    inf = FusedInference(alg._actor_layers, alg._critic_layers)
    assert inf.ok == (shape in OTHER_SHAPES)
    inf.refresh()
    _gradient_parity(monkeypatch, alg, 24, 4, shape)


# ---------------------------------------------------------------------------------------------------- 5. other activations, non-fusable policies
@pytest.mark.parametrize("activation", ["elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "crelu", "identity"])
def test_update_gradient_for_every_activation(monkeypatch, activation):
    """Gradient parity for every activation ActorCritic accepts at [400, 200, 100]: the activation backward of the explicit update, imx_mlp_dw
    on the (pre-activation, output) pairs the forward saves, the output layers without a pending ELU."""
    from isaaclab_amd.rsl_rl.actor_critic import _ACT

    assert activation in _ACT
    fx, _, _ = _task(ROUGH)
    ah, ch, D, A = ODD_SHAPE
    alg = _ppo(D, A, ah, ch, fx["agent"], activation=activation)
    _gradient_parity(monkeypatch, alg, 24, 4, activation)


def test_activation_list_is_covered():
    from isaaclab_amd.rsl_rl.actor_critic import _ACT

    assert set(_ACT) == {"elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "crelu", "identity"}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("policy", [{"activation": "tanh"}, {"actor_hidden_dims": [512, 512, 256, 128], "critic_hidden_dims": [512, 512, 256, 128]}],
                         ids=["tanh", "elu-5-linear"])
def test_runner_trains_a_policy_the_fused_inference_does_not_take(policy, use_graph):
    """OnPolicyRunner.learn on flat Anymal-C with a policy that imx_mlp_infer does not take (FusedInference.ok False): the rollout runs the
    library forward + imx_policy_act and must survive refresh() on every rollout after the first (it raised AttributeError); with
    use_graph five iterations also capture and replay the update (a non-ELU activation backward inside the capture).  Then one more
    rollout, checked against the float64 policy."""
    runner = _runner("Isaac-Velocity-Flat-Anymal-C-v0", 256, use_graph=use_graph, policy=policy)
    p0 = runner.alg.bucket.flat.clone()
    runner.learn(5)
    torch.cuda.synchronize()
    assert not runner._infer.ok
    assert int(runner.alg._adam[1]) == 5 * 5 * 4
    p = runner.alg.bucket.flat
    assert bool(torch.isfinite(p).all()) and not torch.equal(p0, p)
    assert all(np.isfinite(v) for v in runner.alg.loss_dict().values())
    if use_graph:
        assert runner._graph is not None and runner.alg._update_t in ("eager", "graph")
    runner.collect()
    torch.cuda.synchronize()
    _check_storage_against_fp64(runner, str(policy))
    runner.env.unwrapped.close()
