"""CPU: Isaac-Lift-Cube-Franka-v0 compiles to the fused path -- the binary gripper action (1 action column, 2 joint targets), the scene's
rigid object and frame transformer, the manipulation/lift/mdp terms -- nothing of the existing tasks' plans or feeds moves, and the fp64
statements of tests/_lift_cases.py reproduce what the reference's managers recorded (which licenses them as the oracle of the GPU sweep)."""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import _lift_cases as lc
from _util import FLOAT_TOL, Golden

from isaaclab_amd import plan as planmod
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import O_OPS, T_OPS, W_OPS, compile_plan
from isaaclab_amd.robots import FRANKA_PANDA, ROBOTS, SceneEntityResolver
from isaaclab_amd.state_feed import DYNAMIC, EXTRA, STATIC, StateFeed

H, R, REC = planmod.H, planmod.R, planmod.REC_WORDS
HAND = FRANKA_PANDA.body_names.index(lc.EE_BODY)


def _recs(blob, off_key, n):
    off = blob[H[off_key]]
    return [blob[off + i * REC: off + (i + 1) * REC] for i in range(n)]


def _floats(blob, off, n):
    return np.asarray(blob[off:off + n], np.int32).view(np.float32).tolist()


def _wf(word):
    return float(np.asarray(word, np.int32).view(np.float32))


def _env():
    return copy.deepcopy(lc.load_fixture()["env"])


def test_lift_fixture_compiles_to_the_live_cfg_blob_with_no_python_term():
    fx = lc.load_fixture()
    assert fx["task"] == lc.TASK and fx["robot"] == lc.ROBOT
    p = compile_plan(fx["env"], FRANKA_PANDA)
    z = np.load(os.path.join(os.path.dirname(lc.FIXTURE), lc.TASK + ".npz"))
    assert np.array_equal(np.asarray(p.blob), z["live_cfg/blob"])  # what the live cfg object compiled to (tools/gen_golden_lift.py)
    assert (p.action_dim, p.processed_action_dim, p.obs_dim, p.cmd_dim) == (lc.A, lc.PA, lc.D, 7)
    assert p.blob[H["A"]] == 8 and p.blob[H["PA"]] == 9
    assert p.n_ext_rew == p.n_ext_term == p.n_ext_obs == 0
    assert p.max_episode_length == 250 and abs(p.step_dt - 0.02) < 1e-12
    assert [t.op for t in p.obs_terms] == [O_OPS[k] for k in ("JOINT_POS_REL", "JOINT_VEL_REL", "OBJECT_POSITION_IN_ROBOT_ROOT_FRAME",
                                                                "GENERATED_COMMANDS", "LAST_ACTION")]
    assert [t.dim for t in p.obs_terms] == [9, 9, 3, 7, 8]
    assert [t.op for t in p.reward_terms] == [W_OPS[k] for k in ("OBJECT_EE_DISTANCE", "OBJECT_IS_LIFTED", "OBJECT_GOAL_DISTANCE",
                                                                    "OBJECT_GOAL_DISTANCE", "ACTION_RATE_L2", "JOINT_VEL_L2")]
    assert [t.weight for t in p.reward_terms] == [1.0, 15.0, 16.0, 5.0, -1e-4, -1e-4]
    assert [t.op for t in p.termination_terms] == [T_OPS["TIME_OUT"], T_OPS["ROOT_HEIGHT_BELOW_MIN"]]
    term = _recs(p.blob, "TERM_OFF", 2)
    assert term[1][R["AUX0"]] == 1 and _wf(term[1][R["P0"]]) == lc.f32(lc.DROP_HEIGHT)  # the object's root, not the robot's
    rew = _recs(p.blob, "REW_OFF", 4)
    assert rew[0][R["NIDS"]] == 1 and p.blob[rew[0][R["IDS_OFF"]]] == HAND  # the ee frame: body + offset position
    assert [_wf(rew[0][R[k]]) for k in ("P0", "P1", "P2", "P3")] == [lc.f32(lc.STD_EE), 0.0, 0.0, lc.f32(0.1034)]
    assert _wf(rew[1][R["P0"]]) == lc.f32(lc.MIN_HEIGHT)
    assert [(_wf(r[R["P0"]]), _wf(r[R["P1"]])) for r in rew[2:]] == [(lc.f32(0.3), lc.f32(0.04)), (lc.f32(0.05), lc.f32(0.04))]
    # actions: the arm's 7 affine columns, then the binary gripper term -- 1 raw column, 2 joints from processed column 7
    arm, grip = _recs(p.blob, "ACT_OFF", 2)
    assert (arm[R["OP"]], arm[R["OUT"]], arm[R["DIM"]], arm[R["NIDS"]], arm[R["P2"]]) == (planmod.A_JOINT_AFFINE, 0, 7, 7, 0)
    assert (grip[R["OP"]], grip[R["OUT"]], grip[R["DIM"]], grip[R["NIDS"]], grip[R["P2"]]) == (planmod.A_BINARY_JOINT, 7, 1, 2, 0)
    assert list(p.blob[grip[R["IDS_OFF"]]:grip[R["IDS_OFF"]] + 2]) == [7, 8]
    assert _floats(p.blob, grip[R["AUX0"]], 2) == [lc.f32(0.04)] * 2 and _floats(p.blob, grip[R["AUX1"]], 2) == [0.0, 0.0]
    assert [(t.name, t.dim, t.processed_col, t.processed_dim) for t in p.action_terms] == [("arm_action", 7, 0, 7), ("gripper_action", 1, 7, 2)]
    ag = fx["agent"]
    assert ag["policy"]["actor_hidden_dims"] == [256, 128, 64] and ag["num_steps_per_env"] == 24


def test_every_existing_fixture_keeps_the_new_words_zero():
    """No existing blob changes: header word 45 (the processed width) and the action records' first-processed-column word stay 0, the
    state struct grows at its end only."""
    cfg_dir = os.path.join(os.path.dirname(planmod.__file__), "configs")
    tasks = sorted(f[:-5] for f in os.listdir(cfg_dir) if f.endswith(".json") and not f.endswith(".managers.json"))
    assert len(tasks) >= 15 and lc.TASK not in tasks
    for task in tasks:
        fx = load_task_cfg(task)
        p = compile_plan(fx["env"], ROBOTS[fx["robot"]])
        assert p.blob[H["PA"]] == 0 and list(p.blob[45:48]) == [0, 0, 0], task
        assert p.processed_action_dim == p.action_dim, task
        for r in _recs(p.blob, "ACT_OFF", p.blob[H["NACT"]]):
            assert r[R["OP"]] == planmod.A_JOINT_AFFINE and r[R["P2"]] == 0 and r[R["P3"]] == 0, task
        for r in _recs(p.blob, "TERM_OFF", p.blob[H["NTERM"]]):
            assert r[R["OP"]] != T_OPS["ROOT_HEIGHT_BELOW_MIN"] or r[R["AUX0"]] == 0, task
    from isaaclab_amd import _lib

    assert _lib.STATE_FIELDS[-1] == "object_root_pos_w" and _lib.STATE_FIELDS[-2] == "body_quat_w"


def test_lift_blob_validates_through_the_c_abi_and_the_library_has_the_lift_kernel(libimx):
    p = compile_plan(lc.load_fixture()["env"], FRANKA_PANDA)
    blob = np.ascontiguousarray(p.blob, np.int32)
    h = ctypes.c_void_p()
    assert libimx.imx_plan_create(blob.ctypes.data, blob.size, ctypes.byref(h)) == 0, libimx.imx_last_error()
    assert libimx.imx_plan_obs_dim(h) == lc.D
    libimx.imx_plan_destroy(h)

    def create(b):
        b = np.ascontiguousarray(b, np.int32)
        return libimx.imx_plan_create(b.ctypes.data, b.size, ctypes.byref(h))

    bad = p.blob.copy(); bad[H["PA"]] = 8  # the terms write 9 processed columns
    assert create(bad) != 0 and b"processed columns" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[bad[H["ACT_OFF"]] + REC + R["AUX1"]] = int(bad[H["TOTAL_WORDS"]]) - 1  # a close table past the blob
    assert create(bad) != 0 and b"open / close table" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[bad[H["TERM_OFF"]] + REC + R["AUX0"]] = 2
    assert create(bad) != 0 and b"asset selector" in libimx.imx_last_error()
    from isaaclab_amd import _lib

    data = open(_lib.LIB_PATH, "rb").read()
    assert b"_Z15k_term_rew_lift" in data


def test_lift_refusals():
    # the lift.mdp module is closed: a function of it without a table entry is refused in every manager, never Python-evaluated
    for kind, path in (("rewards", ("rewards", "lifting_object")), ("terminations", ("terminations", "object_dropping")),
                       ("observations", ("observations", "policy", "object_position"))):
        env = _env()
        node = env
        for k in path:
            node = node[k]
        node["func"] = f"{lc.LIFT}.{kind}:not_a_lift_term"
        with pytest.raises(NotImplementedError, match="has no fused op"):
            compile_plan(env, FRANKA_PANDA)
    env = _env()  # a rotated target-frame offset
    env["scene"]["ee_frame"]["target_frames"][0]["offset"]["rot"] = [0.0, 1.0, 0.0, 0.0]
    with pytest.raises(NotImplementedError, match="reaching_object.*offset rotation"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()  # a target frame on a body the robot does not have
    env["scene"]["ee_frame"]["target_frames"][0]["prim_path"] = "{ENV_REGEX_NS}/Robot/panda_tool"
    with pytest.raises(ValueError, match="reaching_object.*panda_tool"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()  # two rigid objects
    env["scene"]["object2"] = dict(env["scene"]["object"], prim_path="{ENV_REGEX_NS}/Object2")
    with pytest.raises(NotImplementedError, match="2 rigid objects"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()  # no object in the scene
    del env["scene"]["object"]
    with pytest.raises(ValueError, match="'object'"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()  # the command must be a pose command, and must exist
    env["rewards"]["object_goal_tracking"]["params"]["command_name"] = "nothing"
    with pytest.raises(ValueError, match="object_goal_tracking.*'nothing'"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()
    env["commands"]["object_pose"]["class_type"] = "isaaclab.envs.mdp.commands.velocity_command:UniformVelocityCommand"
    with pytest.raises(ValueError, match="UniformPoseCommand"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()  # BinaryJointAction.__init__'s own errors
    env["actions"]["gripper_action"]["close_command_expr"] = {"panda_finger_joint1": 0.0}
    with pytest.raises(ValueError, match="Could not resolve all joints for the action term. Missing: {'panda_finger_joint2'}"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()
    env["actions"]["gripper_action"]["class_type"] = "isaaclab.envs.mdp.actions.task_space_actions:DifferentialInverseKinematicsAction"
    with pytest.raises(NotImplementedError, match="not on the fused path"):  # the IK variants of the task stay out
        compile_plan(env, FRANKA_PANDA)


def test_binary_velocity_action_and_term_order_variants():
    """BinaryJointVelocityAction is the same arithmetic; a binary term FIRST shifts the affine term's processed columns (P2 word);
    object_reached_goal compiles with its defaults."""
    env = _env()
    env["actions"] = {"gripper_action": dict(env["actions"]["gripper_action"], class_type="isaaclab.envs.mdp.actions.binary_joint_actions:BinaryJointVelocityAction",
                                            open_command_expr={"panda_finger_joint1": 0.5, "panda_finger_joint2": -0.25}),
                      "arm_action": env["actions"]["arm_action"]}
    env["terminations"]["reached"] = {"func": f"{lc.LIFT}.terminations:object_reached_goal", "params": {}, "time_out": False}
    p = compile_plan(env, FRANKA_PANDA)
    grip, arm = _recs(p.blob, "ACT_OFF", 2)
    assert (grip[R["OP"]], grip[R["OUT"]], grip[R["DIM"]], grip[R["NIDS"]], grip[R["P2"]]) == (planmod.A_BINARY_JOINT, 0, 1, 2, 0)
    assert _floats(p.blob, grip[R["AUX0"]], 2) == [0.5, -0.25]
    assert (arm[R["OUT"]], arm[R["DIM"]], arm[R["P2"]]) == (1, 7, 2)
    t = _recs(p.blob, "TERM_OFF", 3)[2]
    assert t[R["OP"]] == T_OPS["OBJECT_REACHED_GOAL"] and _wf(t[R["P0"]]) == lc.f32(0.02)


def test_scene_entities_and_fixture_path_form():
    fx = lc.load_fixture()
    sc = fx["env"]["scene"]
    assert sc["object"]["class_type"].endswith(":RigidObject") and sc["ee_frame"]["class_type"].endswith(":FrameTransformer")
    r = SceneEntityResolver(FRANKA_PANDA, sc)
    assert r.rigid_objects == {"object": "Object"} and r.names("object", "body") == ["Object"] and r.names("object", "joint") == []
    assert r.frame("ee_frame") == ("panda_hand", (0.0, 0.0, 0.1034), (1.0, 0.0, 0.0, 0.0))
    assert r.ids({"name": "object", "body_names": None, "body_ids": "slice(None, None, None)"}, "body") == [0]
    with pytest.raises(ValueError, match="does not exist"):
        r.names("table", "body")
    with pytest.raises(ValueError, match="does not exist"):
        SceneEntityResolver(FRANKA_PANDA).names("object", "body")
    # task names keep resolving as before; a path that does not exist is an error
    assert load_task_cfg("Isaac-Reach-Franka-v0")["task"] == "Isaac-Reach-Franka-v0"
    with pytest.raises(FileNotFoundError):
        load_task_cfg(os.path.join(os.path.dirname(lc.FIXTURE), "no-such-task.json"))
    with pytest.raises(FileNotFoundError):
        load_task_cfg(lc.TASK)  # data derived from the reference lives under tests/golden only
    ev = fx["env"]["events"]
    assert sorted(ev) == ["reset_all", "reset_object_position"] and ev["reset_object_position"]["func"].endswith(":reset_root_state_uniform")


def test_object_feed_and_existing_feeds_unchanged():
    """object_root_pos_w comes from a generator of its own: a feed regenerated with a fixture's seed still reproduces every recorded
    tensor; the object lies next to the robot root, its height over about -0.15 ... 0.5 m."""
    g = Golden("Isaac-Velocity-Flat-Anymal-C-v0")
    f = StateFeed(g.robot, g.N, "cpu", seed=g.meta["seed"], num_snapshots=g.steps + 1)
    assert "object_root_pos_w" in f.names() and EXTRA[-1] == "object_root_pos_w"
    for k, tag in enumerate(["reset"] + [f"step{t}" for t in range(g.steps)]):
        for n in DYNAMIC:
            assert torch.equal(f._stack[n][k], g.t(f"{tag}/in/{n}")), (tag, n)
    for n in STATIC:
        assert torch.equal(f[n], g.t(f"static/{n}")), n
    r = Golden("Isaac-Reach-Franka-v0")
    f = StateFeed(r.robot, r.N, "cpu", seed=r.meta["seed"], num_snapshots=r.steps + 1)
    assert torch.equal(f._stack["joint_pos"][0], r.t("reset/in/joint_pos"))
    assert torch.equal(f._stack["command"][0][:, :3], r.t("reset/in/command")[:, :3])  # (the fixture's tweak turned orientations only)
    f = StateFeed(FRANKA_PANDA, 4099, "cpu", seed=5, num_snapshots=3)
    for _ in range(3):
        rel = f["object_root_pos_w"] - f["root_pos_w"]
        assert rel.shape == (4099, 3) and rel.dtype == torch.float32
        assert abs(float(rel[:, 0].mean()) - 0.5) < 0.02 and abs(float(rel[:, 1].mean())) < 0.02
        z = f["object_root_pos_w"][:, 2]
        assert float(z.min()) < -0.1 and float(z.max()) > 0.45 and float(z.min()) > -0.3 and float(z.max()) < 0.65
        assert bool((z < -0.05).any()) and bool(((z > -0.05) & (z < 0.04)).any()) and bool((z > 0.04).any())
        f.advance()


def test_golden_takes_every_branch():
    g = lc.golden()
    b = dict(g.meta["branches"])
    assert g.meta["ee_body_id"] == HAND and g.meta["processed_action_dim"] == lc.PA and g.meta["action_dim"] == lc.A
    assert g.N == 64 and g.steps == 5 and g.meta["obs_dim"] == lc.D
    assert b.pop("gripper_nan") == 0
    assert all(v > 0 for v in b.values()), b
    # what the recorded branch counts say is what the recorded tensors hold
    names = ("root_pos_w", "root_quat_w", "command", "body_pos_w", "body_quat_w", "object_root_pos_w")
    snaps = [{n: g.t(f"step{t}/in/{n}") for n in names} for t in range(g.steps)]
    again = lc.branch_counts(snaps, HAND, [g.t(f"step{t}/action") for t in range(g.steps)])
    assert again == g.meta["branches"]
    drops = sum(int(g.t(f"step{t}/term_dones/object_dropping").sum()) for t in range(g.steps))
    assert drops == g.meta["branches"]["dropped"] > 0


def test_fp64_formulas_reproduce_the_reference_golden():
    """The per-term values the reference's managers recorded against the fp64 statements of tests/_lift_cases.py: FLOAT_TOL, plus the
    fp32 rounding of world coordinates (position_rounding; over std for the tanh kernels).  Thresholds and the binary action: exact."""
    g = lc.golden()
    names = ("root_pos_w", "root_quat_w", "command", "body_pos_w", "body_quat_w", "object_root_pos_w")
    terms = g.meta["reward_terms"]
    assert terms[:4] == ["reaching_object", "lifting_object", "object_goal_tracking", "object_goal_tracking_fine_grained"]
    for t in range(g.steps):
        tag = f"step{t}"
        s = {n: g.t(f"{tag}/in/{n}") for n in names}
        ref = lc.lift_terms(s, HAND)
        ulp = lc.position_rounding(s, HAND)
        sr = g.t(f"{tag}/step_reward").double()
        for col, (key, w, extra) in enumerate((("object_ee_distance", 1.0, ulp / lc.STD_EE), ("object_is_lifted", 15.0, 0.0),
                                               ("object_goal_distance", 16.0, ulp / lc.STD_GOAL),
                                               ("object_goal_distance_fine", 5.0, ulp / lc.STD_GOAL_FINE))):
            got, val = sr[:, col] / w, ref[key]
            err = (got - val).abs()
            assert bool((err <= FLOAT_TOL * val.abs().clamp_min(1.0) + extra).all()), (tag, key, float(err.max()))
        assert torch.equal((sr[:, 1] > 7.5).double(), ref["object_is_lifted"])  # (the recorded value is f * w * dt / dt in fp32)
        assert torch.equal(g.t(f"{tag}/term_dones/object_dropping"), ref["object_dropping"])
        obs = g.t(f"{tag}/obs").double()[:, 18:21]
        err = (obs - ref["object_position"]).abs()
        assert bool((err <= FLOAT_TOL * ref["object_position"].abs().clamp_min(1.0) + ulp[:, None]).all()), (tag, float(err.max()))
        # the binary gripper term: where(a < 0, close, open) on both finger joints; +0.0, -0.0 and everything not < 0 open
        a = g.t(f"{tag}/action")[:, lc.GRIPPER_COL]
        want = torch.where(a < 0, torch.tensor(0.0), torch.tensor(np.float32(0.04)))
        pa = g.t(f"{tag}/processed_actions")
        assert pa.shape == (g.N, lc.PA)
        assert torch.equal(pa[:, 7], want) and torch.equal(pa[:, 8], want)
        m = torch.arange(g.N) % 8
        assert bool((want[m == 0] == np.float32(0.04)).all()) and bool((want[m == 1] == np.float32(0.04)).all())
        assert bool((want[m == 2] == 0).all()) and bool((want[m == 3] == 0).all())


def test_binary_action_clip_is_folded_into_both_tables():
    """``clip`` on a binary term: the reference clamps the selected table (binary_joint_actions.py:129-132), which is the selection of the
    clamped tables.  Its clip tensor is (N, action_dim = 1, 2), so only a one-joint term can carry one; several joints are refused."""
    env = _env()
    one = dict(env["actions"]["gripper_action"], class_type="isaaclab.envs.mdp.actions.binary_joint_actions:BinaryJointVelocityAction",
               joint_names=["panda_finger_joint1"], open_command_expr={"panda_finger_joint1": 0.5},
               close_command_expr={"panda_finger_joint1": -0.5}, clip={"panda_finger_joint1": (-0.1, 0.3)})
    env["actions"] = {"arm_action": env["actions"]["arm_action"], "gripper_action": one}
    p = compile_plan(env, FRANKA_PANDA)
    assert (p.action_dim, p.processed_action_dim) == (8, 8) and p.blob[H["PA"]] == 0  # one joint: as wide as its raw column
    grip = _recs(p.blob, "ACT_OFF", 2)[1]
    assert (grip[R["OP"]], grip[R["DIM"]], grip[R["NIDS"]], grip[R["P2"]], grip[R["FLAGS"]]) == (planmod.A_BINARY_JOINT, 1, 1, 0, 0)
    assert _floats(p.blob, grip[R["AUX0"]], 1) == [lc.f32(0.3)] and _floats(p.blob, grip[R["AUX1"]], 1) == [lc.f32(-0.1)]
    one["clip"] = {"panda_finger_joint1": (-1.0, 1.0)}  # a clip that does not bind leaves the tables
    p = compile_plan(env, FRANKA_PANDA)
    grip = _recs(p.blob, "ACT_OFF", 2)[1]
    assert _floats(p.blob, grip[R["AUX0"]], 1) == [0.5] and _floats(p.blob, grip[R["AUX1"]], 1) == [-0.5]
    one["clip"] = [-1.0, 1.0]
    with pytest.raises(ValueError, match="Unsupported clip type"):
        compile_plan(env, FRANKA_PANDA)
    env = _env()
    env["actions"]["gripper_action"]["clip"] = {"panda_finger_.*": (0.0, 0.02)}
    with pytest.raises(NotImplementedError, match="gripper_action.*clip on a binary action term over 2 joints"):
        compile_plan(env, FRANKA_PANDA)
