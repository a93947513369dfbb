"""GPU: ``DifferentialInverseKinematicsAction`` on the fused path -- the stand-alone kernel (``imx_diff_ik``) against the fixtures of the
REAL class (tools/gen_golden_diff_ik.py) through the env's schedule, its modes, what it may read and write, its argument checks, and the
env / manager / runner wiring on the Franka IK fixtures.  The tolerances are those of tests/_diff_ik_cases.py."""


import numpy as np
import pytest
import torch

import _diff_ik_cases as ikc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the stand-alone kernel
@pytest.mark.parametrize("n", [256, 1, 63, 64, 65])
@pytest.mark.parametrize("variant", ikc.VARIANTS)
def test_diff_ik_kernel_matches_reference(variant, n):
    """Mode 1, then mode 2 twice per step, all 6 steps, against the fp64 recording of the real class; the first n envs: the whole
    fixture, a single lane, a partial wave, a full wave, one lane past it.  n in {6, 7} joints, ND in {9, 12}, column offset 0 and 6."""
    _, worst = ikc.run_kernel(ikc.IkGolden(variant, n))
    print(f"{variant} n={n}: largest rho {worst:.3g}, bound {ikc.FACTOR * ikc.META[variant]['rho_ref']:.3g}")


@pytest.mark.parametrize("variant", ikc.VARIANTS)
def test_diff_ik_mode3_equals_mode1_then_mode2(variant):
    g = ikc.IkGolden(variant, 130)
    split, _ = ikc.run_kernel(g)
    merged, _ = ikc.run_kernel(g, merged_first=True)
    # split: (1, 2, 2) per step; merged: (3, 2) per step
    for t in range(g.steps):
        for a, b in ((split[3 * t + 1], merged[2 * t]), (split[3 * t + 2], merged[2 * t + 1])):
            for x, y in zip(a, b):
                assert torch.equal(x, y), f"{variant} step {t}: mode 3 differs from mode 1 followed by mode 2"


@pytest.mark.parametrize("variant", ikc.VARIANTS)
def test_diff_ik_reads_only_its_rows_and_columns(variant):
    """NaN in every body row of the Jacobians but the term's and in every column it does not control, in every other body's pose and in
    the uncontrolled joints: the outputs stay finite and equal to the clean run bit for bit; the sentinel row after N and the sentinel
    column after the term's joints stay untouched (KernelTerm.outputs asserts it after every call)."""
    g = ikc.IkGolden(variant, 70)
    clean, _ = ikc.run_kernel(g)
    poisoned, _ = ikc.run_kernel(g, fill=float("nan"))
    for k, (a, b) in enumerate(zip(clean, poisoned)):
        for x, y in zip(a, b):
            assert torch.isfinite(y).all() and torch.equal(x, y), f"{variant} call {k}: the poisoned run differs"


def test_diff_ik_argument_checks_launch_nothing():
    from isaaclab_amd import _lib

    g = ikc.IkGolden("V1", 8)
    k = ikc.KernelTerm(g.ik, g.N)
    st, p = g.state(0, 0), ikc.processed_full(g, 0)
    assert k.call(3, p, st) == 0
    torch.cuda.synchronize()
    before = [x.clone() for x in (k.ee_pos_des, k.ee_quat_des, k.joint_pos_des)]
    p2 = p + 1.0  # a launch would change every output

    def bad_cfg(**kw):
        c = type(k.cfg).from_buffer_copy(bytes(k.cfg))
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, name)[v[0]] = v[1]
            else:
                setattr(c, name, v)
        return c

    cases = {
        "mode 0": dict(mode=0), "mode 4": dict(mode=4), "N = 0": dict(N=0),
        "null processed action": dict(processed=None), "null root_pos": dict(root_pos=None), "null root_quat": dict(root_quat=None),
        "null body_pos": dict(body_pos=None), "null body_quat": dict(body_quat=None), "null jacobians": dict(jac=None),
        "null joint_pos": dict(joint_pos=None), "null ee_pos_des": dict(pos_des=None), "null ee_quat_des": dict(quat_des=None),
        "null joint_pos_des": dict(q_des=None), "body_idx past B": dict(B=g.ik.body_idx), "jacobi_body_idx past NB": dict(NB=g.ik.jacobi_body_idx),
        "column past ND": dict(ND=6), "joint id past J": dict(J=6), "processed columns past PA": dict(PA=5), "ld_des < n": dict(ld=6),
        "nine joints": dict(cfg=bad_cfg(num_joints=9)), "no joints": dict(cfg=bad_cfg(num_joints=0)),
        "negative column": dict(cfg=bad_cfg(jacobi_joint_ids=(2, -1))), "negative joint": dict(cfg=bad_cfg(joint_ids=(0, -3))),
        "negative body": dict(cfg=bad_cfg(body_idx=-1)), "negative Jacobian row": dict(cfg=bad_cfg(jacobi_body_idx=-1)),
        "unknown method": dict(cfg=bad_cfg(ik_method=2)), "unknown command": dict(cfg=bad_cfg(command_type=5)),
        "negative processed column": dict(cfg=bad_cfg(processed_col=-1)),
    }
    for name, kw in cases.items():
        kw = dict(kw)
        mode, cfg = kw.pop("mode", 3), kw.pop("cfg", None)
        assert k.call(mode, p2, st, cfg=cfg, **kw) != 0, f"{name}: accepted"
        assert _lib.lib().imx_last_error().decode().startswith("imx_diff_ik:"), name
    assert _lib.lib().imx_diff_ik(None, g.N, 3, None, 6, None, None, None, None, 11, None, 10, 9, None, 9, None, None, None, 8, None) != 0, "null cfg: accepted"
    torch.cuda.synchronize()
    for x, y in zip(before, (k.ee_pos_des, k.ee_quat_des, k.joint_pos_des)):
        assert torch.equal(x, y), "a refused call wrote to an output"


# ------------------------------------------------------------------------------------------------ env, managers, runner
HAND = 8  # panda_hand among FRANKA_PANDA.body_names


def _ik_env(task, N=64, seed=23, **kw):
    """An env on the task's fixture over a synthetic feed whose hand sits within the fixtures' 0.4 m of the root (the distribution E_ref
    and rho_ref were measured on; the feed's own body positions lie around the world origin, metres from an env's root)."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg(ikc.task_path(task))
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=seed, num_snapshots=4)
    g = torch.Generator().manual_seed(seed + 1)
    feed._stack["body_pos_w"][:, :, HAND] = feed._stack["root_pos_w"] + (torch.randn(4, N, 3, generator=g) * 0.4).cuda()
    return ManagerBasedRLEnv(fx, state_feed=feed, seed=seed, noise_seed=seed, **kw), fx


def _cpu_state(env):
    f = env.feed
    return {k: f[k].cpu().clone() for k in ("root_pos_w", "root_quat_w", "body_pos_w", "body_quat_w", "jacobians", "joint_pos")}


def _check_against_fp64(env, o64, dq64, kappa, step):
    """The env's three IK tensors against the fp64 restatement with the tolerances of variant V1 (the IK-Rel tasks' own cfg)."""
    m = ikc.META["V1"]
    for name, got, ref in (("ee_pos_des", env._ee_pos_des, o64.ee_pos_des), ("ee_quat_des", env._ee_quat_des, o64.ee_quat_des)):
        ref = ref.numpy()
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        tol = np.maximum(ikc.FACTOR * m["E_ref"][name], 2.0 ** -23 * np.maximum(1.0, np.abs(ref)))
        assert (err <= tol).all(), f"step {step} {name}: max error {err.max():.3g}"
    r = ikc.rho(env._joint_pos_des.cpu().numpy(), o64.joint_pos_des.numpy(), dq64.numpy(), kappa.numpy())
    assert (r <= ikc.FACTOR * m["rho_ref"]).all(), f"step {step} joint_pos_des: rho {r.max():.3g}, bound {ikc.FACTOR * m['rho_ref']:.3g}"


def test_reach_ik_rel_env_steps_match_the_restatement():
    from _diff_ik_oracle import DiffIKOracle

    env, fx = _ik_env("Isaac-Reach-Franka-IK-Rel-v0")
    N, ik = env.num_envs, env.plan.ik_terms[0]
    assert env.cfg_decimation == 2 and ik.width == 6
    env.reset()
    o32, o64 = DiffIKOracle(ik, N), DiffIKOracle(ik, N, torch.float64)
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        action = torch.randn(N, 6, generator=g)
        st = _cpu_state(env)  # the feed moves on at the end of the physics: every launch of this step reads this state
        st64 = {k: v.double() for k, v in st.items()}
        o32.process_actions(action)
        o64.process_actions(action.double())
        o64.processed_actions = o32.processed_actions.double()  # (the kernel's input is the fp32 processed action)
        o64.set_command(st64)
        for _ in range(2):
            o64.apply_actions(st64)
        jac = o64.frame_jacobian(st64)
        kappa = torch.linalg.cond(jac @ jac.transpose(1, 2) + ik.lambda_val ** 2 * torch.eye(6, dtype=torch.float64))
        dq64 = o64.joint_pos_des - st64["joint_pos"][:, ik.joint_ids]
        obs = env.step(action.cuda())[0]["policy"]
        torch.cuda.synchronize()
        term = env.action_manager.get_term("arm_action")
        assert torch.equal(term.raw_actions.cpu(), action) and torch.equal(term.processed_actions.cpu(), o32.processed_actions), step
        assert torch.equal(obs[:, -6:].cpu(), action), "the observation's last_action columns"
        assert term.joint_pos_des.shape == (N, 7) and term.joint_pos_des.data_ptr() == env._joint_pos_des.data_ptr()
        _check_against_fp64(env, o64, dq64, kappa, step)
    env.close()


def test_manager_calls_give_what_step_gives_and_reset_keeps_the_desired_pose():
    a = torch.randn(64, 6, generator=torch.Generator().manual_seed(9)).cuda()
    env, _ = _ik_env("Isaac-Reach-Franka-IK-Rel-v0")
    env.reset()
    env.step(a)
    torch.cuda.synchronize()
    by_step = [x.clone() for x in (env._processed_action, env._ee_pos_des, env._ee_quat_des, env._joint_pos_des)]
    env.close()
    env, _ = _ik_env("Isaac-Reach-Franka-IK-Rel-v0")
    env.reset()
    am = env.action_manager
    am.process_action(a)
    torch.cuda.synchronize()
    assert torch.equal(env._ee_pos_des, by_step[1]) and float(env._joint_pos_des.abs().sum()) == 0.0  # the command is set, nothing applied yet
    for _ in range(2):
        am.apply_action()
    torch.cuda.synchronize()
    for x, y in zip(by_step, (env._processed_action, env._ee_pos_des, env._ee_quat_des, env._joint_pos_des)):
        assert torch.equal(x, y)
    # ActionTerm.reset zeroes the raw action only; the desired pose stays until the next action
    ids = torch.tensor([0, 5, 63], device="cuda:0")
    am.reset(ids)
    term = am.get_term("arm_action")
    assert float(term.raw_actions[ids].abs().sum()) == 0.0 and float(term.raw_actions[1].abs().sum()) > 0.0
    assert torch.equal(term.ee_pos_des, by_step[1]) and torch.equal(term.ee_quat_des, by_step[2])
    am.process_action(-a)
    torch.cuda.synchronize()
    assert not torch.equal(term.ee_pos_des[ids], by_step[1][ids])
    with pytest.raises(ValueError, match="DifferentialInverseKinematicsAction.*task-space command.*joint_pos_des"):
        env.attach_actuator(object())
    env.close()


def test_lift_ik_rel_gripper_columns_sit_behind_the_ik_columns():
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    env, _ = _ik_env("Isaac-Lift-Cube-Franka-IK-Rel-v0")
    assert env.plan.action_dim == 7 and env.plan.processed_action_dim == 8
    base = ManagerBasedRLEnv(ikc.task_path("Isaac-Lift-Cube-Franka-v0"), state_feed=StateFeed(FRANKA_PANDA, 64, "cuda:0", seed=23, num_snapshots=4))
    assert base.plan.action_dim == 8 and base.plan.processed_action_dim == 9
    g = torch.Generator().manual_seed(3)
    grip = torch.randn(64, 1, generator=g)
    grip[:4, 0] = torch.tensor([0.0, -0.0, -1.0e-30, 1.0e-30])
    env.reset()
    base.reset()
    arm = torch.randn(64, 6, generator=g)
    env.step(torch.cat([arm, grip], dim=1).cuda())
    base.step(torch.cat([torch.randn(64, 7, generator=g), grip], dim=1).cuda())
    torch.cuda.synchronize()
    assert torch.equal(env._processed_action[:, 6:8], base._processed_action[:, 7:9])
    assert torch.equal(env.action_manager.get_term("gripper_action").processed_actions, env._processed_action[:, 6:8])
    assert torch.equal(env._processed_action[:, :6].cpu(), arm * 0.5)
    assert torch.isfinite(env._joint_pos_des).all() and float(env._joint_pos_des.abs().sum()) > 0.0
    env.close()
    base.close()


def _ik_abs_rollout(use_graph):
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    torch.manual_seed(31)
    u, fx = _ik_env("Isaac-Reach-Franka-IK-Abs-v0", seed=31)
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(fx["agent"], num_steps_per_env=4), log_dir=None, device="cuda:0", use_graph=use_graph)
    runner.train_mode()
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone().cpu() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    res.update(joint_pos_des=u._joint_pos_des.clone().cpu(), ee_pos_des=u._ee_pos_des.clone().cpu(), ee_quat_des=u._ee_quat_des.clone().cpu(),
               processed=u._processed_action.clone().cpu())
    env.close()
    return res


def test_captured_rollout_equals_eager_on_reach_ik_abs():
    a, c = _ik_abs_rollout(True), _ik_abs_rollout(False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert a["actions"].shape == (4, 64, 7) and float(a["joint_pos_des"].abs().sum()) > 0.0
    # the absolute command is the processed action itself
    assert torch.equal(a["ee_pos_des"], a["processed"][:, 0:3]) and torch.equal(a["ee_quat_des"], a["processed"][:, 3:7])
