"""CPU: the C-ABI library loads, exports every symbol include/imx.h declares, validates plans on the host, and
the product package never reaches into oracle/.  (That the binding equals the header is tests/test_abi.py's.)"""

import ctypes
import os
import re

import numpy as np
import pytest

from _util import KITCHEN, TASKS
from isaaclab_amd import _abi, _lib, plan as planmod
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.robots import ROBOTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(libimx):
    decl = sorted(_abi.FUNCTIONS)
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(libimx, name), f"{name} declared in include/imx.h but not exported by libimx.so"
    assert set(decl) == set(_lib.EXPORTS), set(decl) ^ set(_lib.EXPORTS)
    assert b"gfx950" in libimx.imx_version()


@pytest.mark.parametrize("task", TASKS + (KITCHEN,))
def test_plan_blob_validates_through_the_c_abi(libimx, task):
    fx = load_task_cfg(task)
    p = planmod.compile_plan(fx["env"], ROBOTS[fx["robot"]])
    blob = np.ascontiguousarray(p.blob, np.int32)
    h = ctypes.c_void_p()
    rc = libimx.imx_plan_create(blob.ctypes.data, blob.size, ctypes.byref(h))
    assert rc == 0, libimx.imx_last_error()
    assert libimx.imx_plan_obs_dim(h) == p.obs_dim
    assert libimx.imx_plan_scratch_bytes(h, 4096) > 0
    libimx.imx_plan_destroy(h)


def test_plan_update_in_place_accepts_same_shape_only(libimx):
    """imx_plan_update = RewardManager/TerminationManager.set_term_cfg: a recompiled blob of the same shape replaces the tables, a
    different shape (another observation width) is refused."""
    import copy

    fx = load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")
    robot = ROBOTS[fx["robot"]]
    p = planmod.compile_plan(fx["env"], robot)
    blob = np.ascontiguousarray(p.blob, np.int32)
    h = ctypes.c_void_p()
    assert libimx.imx_plan_create(blob.ctypes.data, blob.size, ctypes.byref(h)) == 0
    cfg = copy.deepcopy(fx["env"])
    cfg["rewards"]["flat_orientation_l2"]["weight"] = 0.0  # non-zero -> zero: same shape in plan v3
    cfg["rewards"]["dof_pos_limits"]["weight"] = -1.0      # zero -> non-zero
    cfg["terminations"]["base_contact"]["params"]["threshold"] = 2.0
    b2 = np.ascontiguousarray(planmod.compile_plan(cfg, robot).blob, np.int32)
    assert b2.size == blob.size
    assert libimx.imx_plan_update(h, b2.ctypes.data, b2.size, None) == 0, libimx.imx_last_error()
    del cfg["observations"]["policy"]["actions"]
    b3 = np.ascontiguousarray(planmod.compile_plan(cfg, robot).blob, np.int32)
    assert libimx.imx_plan_update(h, b3.ctypes.data, b3.size, None) != 0 and b"different shape" in libimx.imx_last_error()
    libimx.imx_plan_destroy(h)


def test_plan_rejects_corrupt_blobs(libimx):
    fx = load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")
    p = planmod.compile_plan(fx["env"], ROBOTS[fx["robot"]])
    h = ctypes.c_void_p()

    def create(b):
        b = np.ascontiguousarray(b, np.int32)
        return libimx.imx_plan_create(b.ctypes.data, b.size, ctypes.byref(h))

    bad = p.blob.copy(); bad[planmod.H["MAGIC"]] = 0
    assert create(bad) != 0 and b"magic" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[planmod.H["TOTAL_WORDS"]] += 1
    assert create(bad) != 0
    assert create(p.blob[:10]) != 0
    # a joint index outside [0, J)
    bad = p.blob.copy()
    rec = bad[planmod.H["REW_OFF"]] + 4 * planmod.REC_WORDS  # dof_torques_l2
    bad[bad[rec + planmod.R["IDS_OFF"]]] = 99
    assert create(bad) != 0 and b"outside" in libimx.imx_last_error()
    # an observation column written twice
    bad = p.blob.copy()
    rec = bad[planmod.H["OBS_OFF"]] + 1 * planmod.REC_WORDS
    bad[rec + planmod.R["OUT"]] = 0
    assert create(bad) != 0


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "isaaclab_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                if f.endswith(".py"):  # nothing in the product may read the reference at run time
                    assert "/root/reference" not in src, f


def test_env_fails_loudly_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from isaaclab_amd.env import ManagerBasedRLEnv

    with pytest.raises(_lib.ImxError):
        ManagerBasedRLEnv("Isaac-Cartpole-v0", num_envs=8)


def test_runner_refuses_policy_and_algorithm_classes_it_does_not_build():
    """isaaclab_rl/rsl_rl/rl_cfg.py:22,86-99,166: ActorCriticRecurrent / ActorCriticCascade / PPOCA / Distillation cfgs must not train
    a plain feed-forward PPO silently."""
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.rsl_rl import OnPolicyRunner
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    agent = load_task_cfg("Isaac-Cartpole-v0")["agent"]
    for section, name in (("policy", "ActorCriticRecurrent"), ("policy", "ActorCriticCascade"), ("algorithm", "PPOCA"), ("algorithm", "Distillation")):
        cfg = {**agent, section: {**agent[section], "class_name": name}}
        with pytest.raises(NotImplementedError, match=name):
            OnPolicyRunner(env=None, train_cfg=cfg, device="cpu")  # refused before the env is touched
    with pytest.raises(NotImplementedError, match="rnn_type"):
        ActorCritic(4, 4, 1, rnn_type="lstm", rnn_hidden_dim=64, rnn_num_layers=1)
    pol = ActorCritic(4, 4, 1, actor_hidden_dims=[8], critic_hidden_dims=[8])
    with pytest.raises(NotImplementedError, match="teacher_coef"):
        PPO(pol, teacher_coef=1.0)


def test_seed_is_callable_on_the_class_like_the_reference_staticmethod():
    """envs/manager_based_env.py:425-443: ``ManagerBasedEnv.seed`` is a @staticmethod."""
    import torch

    from isaaclab_amd.env import ManagerBasedRLEnv

    assert ManagerBasedRLEnv.seed(42) == 42
    a = torch.rand(3)
    assert ManagerBasedRLEnv.seed(42) == 42
    assert torch.equal(a, torch.rand(3))


def test_only_observation_minibatch_buffers_carry_a_row_pitch():
    """The minibatch buffers of the update: observation rows start on 16-byte boundaries (their consumers -- GEMMs, imx_mlp_dw,
    imx_mlp_fwd_elu -- take a row pitch), every per-sample array (actions, old mu / sigma, values ...) is dense: the loss kernels index
    them as (M, A) without a pitch.  Padding those too (round 2 until the end of round 3) fed the update wrong columns for action counts
    >= 16 that are not a multiple of four (G1: 37)."""
    from isaaclab_amd.rsl_rl.storage import RolloutStorage

    for D, Dc, A in ((310, 0, 37), (235, 187, 17), (48, 0, 12), (37, 53, 18)):
        st = RolloutStorage(8, 4, (D,), (Dc,), (A,), device="cpu")
        st._minibatch_setup(2)
        n_obs = 2 if Dc else 1
        for dst in st._mb_dst_sets:
            for k, buf in enumerate(dst):
                if k < n_obs and buf.shape[1] >= 16:
                    assert buf.stride(0) % 4 == 0 and buf.stride(0) - buf.shape[1] < 4, (D, Dc, A, k, buf.stride())
                else:
                    assert buf.is_contiguous(), (D, Dc, A, k, tuple(buf.shape), buf.stride())


@pytest.mark.parametrize("activation,hidden", [("tanh", [128, 128]), ("relu", [400, 200, 100]), ("elu", [512, 512, 256, 128]),
                                               ("elu", [1024, 512, 256, 128])])
def test_fused_inference_of_a_stack_that_does_not_fit_is_off_and_refresh_is_a_no_op(activation, hidden):
    """FusedInference takes ELU stacks of at most 4 Linear layers and 512 features.  Anything else reports ok = False, and the
    runner still calls refresh() at the start of every rollout after the first: that must do nothing (it raised AttributeError)."""
    import torch

    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    pol = ActorCritic(87, 87, 21, actor_hidden_dims=hidden, critic_hidden_dims=hidden, activation=activation)
    before = [p.detach().clone() for p in pol.parameters()]
    for nets in ((pol.actor, pol.critic), (pol.critic,)):
        inf = FusedInference(*[_mlp_layers(n) for n in nets])
        assert not inf.ok
        inf.refresh()
        inf.refresh()
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), before))


@pytest.mark.parametrize("activation", ["elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "crelu", "identity"])
def test_activation_backward_of_the_update_equals_autograd_under_inference_mode(activation):
    """The explicit backward of PPO.update takes every hidden activation but ELU through ppo._act_backward; the update is captured
    into a hipGraph under inference mode, where autograd records nothing.  Its result must equal autograd's, bit for bit."""
    import torch

    from isaaclab_amd.rsl_rl.actor_critic import _ACT
    from isaaclab_amd.rsl_rl.ppo import _act_backward

    act = _ACT[activation]()
    g = torch.Generator().manual_seed(1)
    z = 3.0 * torch.randn(257, 33, generator=g)
    z[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    dh = torch.randn(257, 33, generator=g)
    zz = z.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(act(zz), zz, dh)
    with torch.inference_mode():
        zi, di = z.clone(), dh.clone()
        got = _act_backward(act, di, zi, act(zi))
    assert torch.equal(got, ref)


def test_normalizer_state_dict_round_trip_keeps_count_and_until():
    """The running count is upstream's long ``count`` buffer; loading a state dict restores the host-side count that decides ``until``,
    so a resumed run stops updating where the saved one would have.  Checkpoints of the earlier layout (a float ``_count_f``) still load."""
    import torch

    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization

    a = EmpiricalNormalization([5], until=1000)
    a.count.fill_(100003 * 170)  # past 2^24: an fp32 count could not hold it
    a._host_count = int(a.count)
    a._mean.normal_()
    sd = a.state_dict()
    assert set(sd) == {"_mean", "_var", "_std", "count"} and sd["count"].dtype == torch.int64 and sd["count"].dim() == 0
    b = EmpiricalNormalization([5], until=1000)
    assert b.updating()
    b.load_state_dict(sd)
    assert int(b.count) == 100003 * 170 and b._host_count == 100003 * 170
    assert torch.equal(b._mean, a._mean)
    assert not b.updating()  # past ``until``: forward no longer folds batches in
    c = EmpiricalNormalization([5], until=10 ** 8)
    c.load_state_dict(sd)
    assert c.updating()
    c.eval()
    assert not c.updating()
    old = {"_mean": sd["_mean"], "_var": sd["_var"], "_std": sd["_std"], "_count_f": torch.tensor([4096.0 * 3])}
    d = EmpiricalNormalization([5], until=4096 * 3)
    d.load_state_dict(old)
    assert int(d.count) == 4096 * 3 and d.count.dtype == torch.int64 and not d.updating()
