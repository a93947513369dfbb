"""CPU: Isaac-Reach-Franka-v0 and Isaac-Reach-UR10-v0 compile to the fused path -- the manipulation/reach/mdp rewards, the 7-wide pose
command, the arm robot tables and the feed's body_quat_w / pose command -- and nothing of the existing tasks' plans or feeds moves."""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _reach_cases import REACH, TASKS
from _util import GOLDEN, Golden

from isaaclab_amd import plan as planmod
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import O_OPS, W_OPS, compile_plan
from isaaclab_amd.robots import ANYMAL_C, FRANKA_PANDA, ROBOTS, UR10
from isaaclab_amd.state_feed import DYNAMIC, EXTRA, STATIC, StateFeed


def _recs(p, off_key, n):
    off = p.blob[planmod.H[off_key]]
    return [p.blob[off + i * planmod.REC_WORDS: off + (i + 1) * planmod.REC_WORDS] for i in range(n)]


@pytest.mark.parametrize("task", list(TASKS))
def test_reach_task_compiles_with_no_python_term(task):
    robot_name, ee, D, A, _ = TASKS[task]
    fx = load_task_cfg(task)
    assert fx["robot"] == robot_name
    robot = ROBOTS[robot_name]
    p = compile_plan(fx["env"], robot)
    assert p.n_ext_rew == p.n_ext_term == p.n_ext_obs == 0
    assert (p.obs_dim, p.action_dim, p.cmd_dim) == (D, A, 7) and p.blob[planmod.H["CMD_DIM"]] == 7
    assert [t.op for t in p.reward_terms] == [W_OPS[k] for k in ("POSITION_COMMAND_ERROR", "POSITION_COMMAND_ERROR_TANH",
                                                                    "ORIENTATION_COMMAND_ERROR", "ACTION_RATE_L2", "JOINT_VEL_L2")]
    assert [t.weight for t in p.reward_terms][:3] == [-0.2, 0.1, -0.1]
    assert [t.op for t in p.obs_terms] == [O_OPS[k] for k in ("JOINT_POS_REL", "JOINT_VEL_REL", "GENERATED_COMMANDS", "LAST_ACTION")]
    assert [t.dim for t in p.obs_terms] == [robot.num_joints, robot.num_joints, 7, A]
    assert [t.name for t in p.termination_terms] == ["time_out"]
    assert p.max_episode_length == 360 and abs(p.step_dt - 1.0 / 30.0) < 1e-12
    rew = _recs(p, "REW_OFF", 3)
    for r in rew:  # one body: asset_cfg.body_ids[0]
        assert r[planmod.R["NIDS"]] == 1 and p.blob[r[planmod.R["IDS_OFF"]]] == robot.body_names.index(ee)
    std = np.frombuffer(np.asarray(rew[1][planmod.R["P0"]], np.int32).tobytes(), np.float32)[0]
    assert std == np.float32(0.1)
    # the live cfg object compiles to the very same blob (recorded by tools/gen_golden_reach.py)
    z = np.load(os.path.join(GOLDEN, task + ".npz"))
    assert np.array_equal(np.asarray(p.blob), z["live_cfg/blob"])
    # the action: JointPositionAction, scale 0.5, default offset, panda_joint.* (7 of 9) / .* (6)
    act = fx["env"]["actions"]["arm_action"]
    assert act["scale"] == 0.5 and act["use_default_offset"] is True
    ag = fx["agent"]
    assert ag["policy"]["actor_hidden_dims"] == [64, 64] and ag["policy"]["critic_hidden_dims"] == [64, 64]
    assert ag["num_steps_per_env"] == 24 and ag["algorithm"]["num_learning_epochs"] == 8 and ag["algorithm"]["num_mini_batches"] == 4


def test_reach_side_files_and_robot_tables():
    for task, (robot_name, ee, _, _, _) in TASKS.items():
        robot = ROBOTS[robot_name]
        side = json.load(open(os.path.join(os.path.dirname(planmod.__file__), "configs", task + ".managers.json")))
        ev = side["events"]["reset_robot_joints"]
        assert ev["func"].endswith(":reset_joints_by_scale")
        assert ev["params"]["position_range"] == ([0.5, 1.5] if robot is FRANKA_PANDA else [0.75, 1.25])
        assert sorted(v["func"].rpartition(":")[2] for v in side["curriculum"].values()) == ["modify_reward_weight"] * 2
        assert side["scene"]["robot"]["init_state"]["pos"] == [0.0, 0.0, 0.0]
        assert robot.body_names[-1] in (ee, "panda_rightfinger") and ee in robot.body_names
        cmd = load_task_cfg(task)["env"]["commands"]["ee_pose"]
        assert cmd["class_type"].endswith("pose_command:UniformPoseCommand") and cmd["make_quat_unique"] is False
    assert FRANKA_PANDA.num_joints == 9 and FRANKA_PANDA.num_bodies == 11 and UR10.num_joints == 6 and UR10.num_bodies == 8
    assert FRANKA_PANDA.default_joint_pos_list() == [0.0, -0.569, 0.0, -2.81, 0.0, 3.037, 0.741, 0.04, 0.04]
    assert UR10.default_joint_pos_list() == [0.0, -1.712, 1.712, 0.0, 0.0, 0.0]
    assert FRANKA_PANDA.command_dim == UR10.command_dim == 7 and ANYMAL_C.command_dim == 3


def test_unknown_reach_reward_raises():
    fx = load_task_cfg("Isaac-Reach-Franka-v0")
    env = json.loads(json.dumps(fx["env"]))
    env["rewards"]["end_effector_position_tracking"]["func"] = f"{REACH}:not_a_reach_term"
    with pytest.raises(NotImplementedError):
        compile_plan(env, FRANKA_PANDA)


def test_reach_reward_needs_the_pose_command():
    """The reach rewards read the (N, 7) pose command; a velocity command (3 wide) is an error, and generated_commands follows the
    command term's class."""
    fx = load_task_cfg("Isaac-Reach-UR10-v0")
    env = json.loads(json.dumps(fx["env"]))
    env["commands"]["ee_pose"]["class_type"] = "isaaclab.envs.mdp.commands.velocity_command:UniformVelocityCommand"
    with pytest.raises(ValueError, match="UniformPoseCommand"):
        compile_plan(env, UR10)
    for name in ("end_effector_position_tracking", "end_effector_position_tracking_fine_grained", "end_effector_orientation_tracking"):
        env["rewards"][name]["weight"] = 0.0
        env["rewards"][name]["func"] = "isaaclab.envs.mdp.rewards:is_alive"
    p = compile_plan(env, UR10)
    assert p.cmd_dim == 3 and [t.dim for t in p.obs_terms][2] == 3


@pytest.mark.parametrize("robot", [FRANKA_PANDA, UR10])
def test_arm_feed_serves_a_pose_command_and_unit_body_quaternions(robot):
    f = StateFeed(robot, 257, seed=3, num_snapshots=3)
    for _ in range(3):
        c, q = f["command"], f["body_quat_w"]
        assert c.shape == (257, 7) and c.dtype == torch.float32
        lo = torch.tensor([0.35, -0.2, 0.15])
        hi = torch.tensor([0.65, 0.2, 0.5])
        assert bool(((c[:, :3] >= lo) & (c[:, :3] <= hi)).all())
        assert torch.allclose(c[:, 3:].norm(dim=-1), torch.ones(257), atol=1e-6)
        assert bool((c[:, 3] < 0).any()) and bool((c[:, 3] > 0).any())
        assert q.shape == (257, robot.num_bodies, 4)
        assert torch.allclose(q.norm(dim=-1), torch.ones(257, robot.num_bodies), atol=1e-6)
        f.advance()


def test_existing_feeds_are_unchanged_by_body_quat_w():
    """A feed regenerated with a fixture's seed reproduces every tensor the Anymal-C fixture recorded; body_quat_w comes from a generator
    of its own and the velocity command stays 3 wide."""
    g = Golden("Isaac-Velocity-Flat-Anymal-C-v0")
    f = StateFeed(g.robot, g.N, "cpu", seed=g.meta["seed"], num_snapshots=g.steps + 1)
    assert "body_quat_w" in f.names() and "body_quat_w" in EXTRA
    assert f["command"].shape == (g.N, 3)
    for k, tag in enumerate(["reset"] + [f"step{t}" for t in range(g.steps)]):
        for n in DYNAMIC:
            assert torch.equal(f._stack[n][k], g.t(f"{tag}/in/{n}")), (tag, n)
    for n in STATIC:
        assert torch.equal(f[n], g.t(f"static/{n}")), n
    f2 = StateFeed(ANYMAL_C, 64, "cpu", seed=9, num_snapshots=2)
    assert torch.allclose(f2["body_quat_w"].norm(dim=-1), torch.ones(64, ANYMAL_C.num_bodies), atol=1e-6)


def test_libimx_exports_the_reach_kernels():
    """The reach reward ops live in their own k_term_rew instantiation of libimx.so."""
    from isaaclab_amd import _lib

    path = _lib.LIB_PATH
    data = open(path, "rb").read()
    assert b"_Z10k_term_rewILb0ELb1EE" in data  # k_term_rew<false, true>
    assert b"_Z10k_term_rewILb1ELb0EE" in data and b"_Z10k_term_rewILb0ELb0EE" in data
    ctypes.CDLL(path)


def test_reach_golden_fixtures_exercise_every_branch():
    from _reach_cases import reach_terms

    for task, (robot_name, ee, _, _, pitch) in TASKS.items():
        g = Golden(task)
        b = ROBOTS[robot_name].body_names.index(ee)
        assert g.meta["ee_body_id"] == b and g.meta["command_w_negative"] > 0 and g.meta["ee_quat_w_negative"] > 0
        if pitch == np.pi:
            assert g.meta["command_w_near_zero"] > 0
        vals = {k: [] for k in ("position_command_error", "orientation_command_error")}
        for t in range(g.steps):
            s = {n: g.t(f"step{t}/in/{n}") for n in ("root_pos_w", "root_quat_w", "command", "body_pos_w", "body_quat_w")}
            r = reach_terms(s, b, 0.1)
            for k in vals:
                vals[k].append(r[k])
            # the recorded rewards are the fp64 statements within fp32 rounding
            sr = g.t(f"step{t}/step_reward").double()
            for j, k in enumerate(("position_command_error", "position_command_error_tanh", "orientation_command_error")):
                assert torch.allclose(sr[:, j] / [-0.2, 0.1, -0.1][j], r[k], atol=2e-5, rtol=1e-5), (task, t, k)
        pos, ori = torch.cat(vals["position_command_error"]), torch.cat(vals["orientation_command_error"])
        assert bool((pos < 1e-5).any()) and bool(((pos > 0.09) & (pos < 0.11)).any()) and bool((pos > 0.2).any())
        assert bool((ori < 1e-5).any()) and bool((ori > np.pi - 2e-3).any())
