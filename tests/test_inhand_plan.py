"""CPU: Isaac-Repose-Cube-Allegro-v0 and its NoVelObs variant compile to the fused path -- the in-hand rewards and terminations, the
root observations on the scene's rigid object, goal_quat_diff -- nothing of the existing tasks' plans moves, what the term compiler
refuses is refused with its reason, and the C interface carries the new state pointers and the stand-alone command term."""

import copy
import ctypes
import os

import numpy as np
import pytest

import _inhand_cases as ic

from isaaclab_amd import plan as planmod
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import O_OPS, T_OPS, W_OPS, compile_plan
from isaaclab_amd.robots import ALLEGRO_HAND, ANYMAL_C, ROBOTS

H, R, REC = planmod.H, planmod.R, planmod.REC_WORDS
OBJECT = {"name": "object"}
NEW_STATE = ("object_root_quat_w", "object_root_lin_vel_w", "object_root_ang_vel_w", "command_consecutive_success")


def _recs(blob, off_key, n):
    off = blob[H[off_key]]
    return [blob[off + i * REC: off + (i + 1) * REC] for i in range(n)]


def _wf(word):
    return float(np.asarray(word, np.int32).view(np.float32))


def _env(task=ic.TASK):
    return copy.deepcopy(ic.load_fixture(task)["env"])


def test_robot_spec():
    r = ROBOTS["allegro_hand"]
    assert r is ALLEGRO_HAND and r.num_joints == 16 and r.fixed_base and r.command_dim == 7 and r.default_root_height == 0.5
    assert r.joint_names[:5] == ["index_joint_0", "middle_joint_0", "ring_joint_0", "thumb_joint_0", "index_joint_1"]
    assert r.joint_names[-3:] == ["thumb_joint_1", "thumb_joint_2", "thumb_joint_3"] and len(set(r.joint_names)) == 16
    assert r.body_names[0] == "palm_link" and len(set(r.body_names)) == r.num_bodies == 17
    d = r.default_joint_pos_list()
    assert d[r.joint_names.index("thumb_joint_0")] == 0.28 and sum(d) == 0.28


def test_fixture_compiles_to_the_live_cfg_blob_with_no_python_term():
    fx = ic.load_fixture()
    assert fx["task"] == ic.TASK and fx["robot"] == ic.ROBOT
    p = compile_plan(fx["env"], ALLEGRO_HAND)
    z = np.load(os.path.join(ic.GOLDEN_DIR, ic.TASK + ".npz"))
    assert np.array_equal(np.asarray(p.blob), z["live_cfg/blob"])  # what the live cfg object compiled to (tools/gen_golden_inhand.py)
    assert (p.action_dim, p.processed_action_dim, p.obs_dim, p.cmd_dim) == (ic.A, ic.A, ic.D, 7)
    assert p.n_ext_rew == 0 and p.n_ext_term == 0 and p.n_ext_obs == 0
    assert p.state_reads == tuple(sorted(NEW_STATE))
    term = _recs(p.blob, "TERM_OFF", 3)
    assert [t[R["OP"]] for t in term] == [T_OPS["TIME_OUT"], T_OPS["MAX_CONSECUTIVE_SUCCESS"], T_OPS["OBJECT_AWAY_FROM_ROBOT"]]
    assert _wf(term[1][R["P0"]]) == 50.0 and _wf(term[2][R["P0"]]) == ic.f32(ic.REACH)
    rew = _recs(p.blob, "REW_OFF", 5)
    assert [r[R["OP"]] for r in rew[:2]] == [W_OPS["TRACK_ORIENTATION_INV_L2"], W_OPS["SUCCESS_BONUS"]]
    assert _wf(rew[0][R["P0"]]) == ic.f32(ic.ROT_EPS)
    assert _wf(rew[1][R["P0"]]) == ic.f32(ic.SUCCESS_THRESHOLD) and _wf(rew[1][R["WEIGHT"]]) == 250.0  # the threshold comes from the command cfg
    act = _recs(p.blob, "ACT_OFF", 1)[0]
    assert act[R["FLAGS"]] & planmod.F_ACT_EMA and act[R["FLAGS"]] & planmod.F_ACT_TO_LIMITS and _wf(act[R["P1"]]) == ic.f32(0.95)
    ag = fx["agent"]
    assert ag["policy"]["actor_hidden_dims"] == [512, 256, 128]


def test_observation_layouts_and_asset_words():
    for task, cols, width in ((ic.TASK, ic.COLS, ic.D), (ic.TASK_NOVEL, ic.COLS_NOVEL, ic.D_NOVEL)):
        p = compile_plan(ic.load_fixture(task)["env"], ALLEGRO_HAND)
        g = p.obs_groups[0]
        assert g.dim == width == p.obs_dim and g.enable_corruption and [t.name for t in g.terms] == list(cols)
        assert [hi - lo for lo, hi in cols.values()] == g.term_widths
        recs = {t.name: r for t, r in zip(g.terms, _recs(p.blob, "OBS_OFF", len(g.terms)))}
        for name, (lo, hi) in cols.items():
            assert recs[name][R["OUT"]] == lo and recs[name][R["DIM"]] == hi - lo, (task, name)
        for name, op in (("object_pos", "ROOT_POS_W"), ("object_quat", "ROOT_QUAT_W"), ("object_lin_vel", "ROOT_LIN_VEL_W"), ("object_ang_vel", "ROOT_ANG_VEL_W")):
            if name in cols:
                assert recs[name][R["OP"]] == O_OPS[op] and recs[name][R["AUX0"]] == 1, (task, name)
        assert recs["goal_quat_diff"][R["OP"]] == O_OPS["GOAL_QUAT_DIFF"] and not recs["goal_quat_diff"][R["FLAGS"]] & planmod.F_QUAT_UNIQUE
        assert recs["object_pos"][R["FLAGS"]] & planmod.F_NOISE_GAUSS and _wf(recs["object_pos"][R["NOISE_HI"]]) == ic.f32(0.002)
        assert p.state_reads == (tuple(sorted(NEW_STATE)) if task == ic.TASK else ("command_consecutive_success", "object_root_quat_w"))
    # make_quat_unique sets the flag on both quaternion terms
    env = _env()
    for name in ("object_quat", "goal_quat_diff"):
        env["observations"]["policy"][name]["params"]["make_quat_unique"] = True
    p = compile_plan(env, ALLEGRO_HAND)
    recs = _recs(p.blob, "OBS_OFF", 9)
    assert recs[3][R["FLAGS"]] & planmod.F_QUAT_UNIQUE and recs[7][R["FLAGS"]] & planmod.F_QUAT_UNIQUE


def test_root_observations_on_the_robot_keep_their_blob():
    """asset word 0 = the robot: a robot-only plan is word for word the same with asset_cfg=SceneEntityCfg("robot") written out; the
    object's word is 1; anything else is refused."""
    fx = load_task_cfg("Isaac-Velocity-Rough-Anymal-C-v0-kitchen")
    env = copy.deepcopy(fx["env"])
    obs = env["observations"]["policy"]
    obs.update({f"extra_{f}": {"func": f"{ic.MDP}.observations:{f}", "params": {}} for f in ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w")})
    base = compile_plan(env, ANYMAL_C)
    for f in ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w"):
        obs[f"extra_{f}"]["params"] = {"asset_cfg": {"name": "robot"}}
    explicit = compile_plan(env, ANYMAL_C)
    assert np.array_equal(base.blob, explicit.blob) and explicit.state_reads == ()
    n = len(explicit.obs_groups[0].terms)
    assert all(r[R["AUX0"]] == 0 for r in _recs(explicit.blob, "OBS_OFF", n)[-4:])
    obs["extra_root_pos_w"]["params"] = {"asset_cfg": {"name": "object"}}
    with pytest.raises(ValueError, match="'object' does not exist"):
        compile_plan(env, ANYMAL_C)
    obs["extra_root_pos_w"]["params"] = {"asset_cfg": {"name": "contact_forces"}}
    with pytest.raises(NotImplementedError, match="the robot or of the scene's rigid object"):
        compile_plan(env, ANYMAL_C)
    env = _env()
    env["scene"]["second"] = dict(env["scene"]["object"], prim_path="{ENV_REGEX_NS}/second")
    with pytest.raises(NotImplementedError, match="2 rigid objects"):
        compile_plan(env, ALLEGRO_HAND)


def test_every_existing_fixture_keeps_its_blob_free_of_the_new_ops():
    cfg_dir = os.path.join(os.path.dirname(planmod.__file__), "configs")
    tasks = sorted(f[:-5] for f in os.listdir(cfg_dir) if f.endswith(".json") and not f.endswith(".managers.json"))
    assert len(tasks) >= 15 and ic.TASK not in tasks
    for task in tasks:
        fx = load_task_cfg(task)
        p = compile_plan(fx["env"], ROBOTS[fx["robot"]])
        assert p.state_reads == (), task
        for r in _recs(p.blob, "OBS_OFF", p.blob[H["NOBS"]]):
            assert r[R["OP"]] < O_OPS["GOAL_QUAT_DIFF"], task
            assert not (O_OPS["ROOT_POS_W"] <= r[R["OP"]] <= O_OPS["ROOT_ANG_VEL_W"]) or r[R["AUX0"]] == 0, task
        assert all(r[R["OP"]] < W_OPS["TRACK_ORIENTATION_INV_L2"] for r in _recs(p.blob, "REW_OFF", p.blob[H["NREW"]])), task
        assert all(r[R["OP"]] < T_OPS["MAX_CONSECUTIVE_SUCCESS"] for r in _recs(p.blob, "TERM_OFF", p.blob[H["NTERM"]])), task
    with pytest.raises(FileNotFoundError):
        load_task_cfg(ic.TASK)  # data derived from the reference lives under tests/golden only


def test_the_module_is_closed_in_all_three_managers():
    for kind, path in (("rewards", ("rewards", "success_bonus")), ("terminations", ("terminations", "max_consecutive_success")),
                       ("observations", ("observations", "policy", "goal_quat_diff"))):
        env = _env()
        node = env
        for k in path:
            node = node[k]
        node["func"] = f"{ic.INHAND}.{kind}:not_an_inhand_term"
        with pytest.raises(NotImplementedError, match="has no fused op"):
            compile_plan(env, ALLEGRO_HAND)


def test_the_terms_the_task_cfg_leaves_out_compile_too():
    env = _env()
    env["rewards"]["track_pos"] = {"func": f"{ic.INHAND}.rewards:track_pos_l2", "weight": -1.0, "params": {"object_cfg": OBJECT, "command_name": "object_pose"}}
    env["terminations"]["away"] = {"func": f"{ic.INHAND}.terminations:object_away_from_goal", "time_out": False,
                                   "params": {"threshold": ic.GOAL_REACH, "command_name": "object_pose"}}
    env["terminations"]["dropped"] = {"func": f"{ic.MDP}.terminations:root_height_below_minimum", "time_out": False,
                                      "params": {"minimum_height": 0.2, "asset_cfg": OBJECT}}
    p = compile_plan(env, ALLEGRO_HAND)
    assert _recs(p.blob, "REW_OFF", 6)[5][R["OP"]] == W_OPS["TRACK_POS_L2"]
    t = _recs(p.blob, "TERM_OFF", 5)
    assert t[3][R["OP"]] == T_OPS["OBJECT_AWAY_FROM_GOAL"] and _wf(t[3][R["P0"]]) == ic.f32(ic.GOAL_REACH)
    assert t[4][R["OP"]] == T_OPS["ROOT_HEIGHT_BELOW_MIN"] and t[4][R["AUX0"]] == 1
    del env["rewards"]["track_orientation_inv_l2"]["params"]["rot_eps"]  # the function's default
    assert _wf(_recs(compile_plan(env, ALLEGRO_HAND).blob, "REW_OFF", 1)[0][R["P0"]]) == ic.f32(1.0e-3)


def test_command_refusals():
    for kind, name in (("rewards", "success_bonus"), ("rewards", "track_orientation_inv_l2"), ("terminations", "max_consecutive_success")):
        env = _env()
        env[kind][name]["params"]["command_name"] = "no_such_command"
        with pytest.raises(ValueError, match="'no_such_command' is not a command term of the cfg"):
            compile_plan(env, ALLEGRO_HAND)
    env = _env()
    env["observations"]["policy"]["goal_quat_diff"]["params"]["command_name"] = "missing"
    with pytest.raises(ValueError, match="'missing' is not a command term of the cfg"):
        compile_plan(env, ALLEGRO_HAND)
    # a 3-wide (velocity) command: not 7 wide
    env = _env()
    env["commands"]["object_pose"] = {"class_type": "isaaclab.envs.mdp.commands.velocity_command:UniformVelocityCommand"}
    del env["observations"]["policy"]["goal_pose"]
    with pytest.raises(ValueError, match=r"must be an InHandReOrientationCommand \(N, 7\); it is 3 wide"):
        compile_plan(env, ALLEGRO_HAND)
    # a 7-wide command without the threshold: a UniformPoseCommand
    for kind, name in (("rewards", "success_bonus"), ("terminations", "max_consecutive_success")):
        env = _env()
        env["commands"]["object_pose"] = {"class_type": "isaaclab.envs.mdp.commands.pose_command:UniformPoseCommand", "body_name": "palm_link"}
        if kind == "terminations":
            del env["rewards"]["success_bonus"]
        with pytest.raises(NotImplementedError, match="has no orientation_success_threshold.*UniformPoseCommand does not have"):
            compile_plan(env, ALLEGRO_HAND)
    env = _env()  # the terms that read the goal only compile against either 7-wide command
    env["commands"]["object_pose"] = {"class_type": "isaaclab.envs.mdp.commands.pose_command:UniformPoseCommand", "body_name": "palm_link"}
    del env["rewards"]["success_bonus"], env["terminations"]["max_consecutive_success"]
    assert compile_plan(env, ALLEGRO_HAND).cmd_dim == 7
    env = _env()
    env["terminations"]["object_out_of_reach"]["params"]["asset_cfg"] = OBJECT  # the robot's place
    with pytest.raises(NotImplementedError, match="reads the robot's root state"):
        compile_plan(env, ALLEGRO_HAND)
    env = _env()
    del env["observations"]["policy"]["goal_quat_diff"]["params"]["asset_cfg"]
    with pytest.raises(KeyError, match="asset_cfg"):
        compile_plan(env, ALLEGRO_HAND)


def test_blobs_validate_through_the_c_abi_and_the_library_has_the_kernels(libimx):
    from isaaclab_amd import _abi, _lib

    h = ctypes.c_void_p()

    def create(b):
        b = np.ascontiguousarray(b, np.int32)
        return libimx.imx_plan_create(b.ctypes.data, b.size, ctypes.byref(h))

    for task, width in ((ic.TASK, ic.D), (ic.TASK_NOVEL, ic.D_NOVEL)):
        p = compile_plan(ic.load_fixture(task)["env"], ALLEGRO_HAND)
        assert create(p.blob) == 0, libimx.imx_last_error()
        assert libimx.imx_plan_obs_dim(h) == width
        assert libimx.imx_observations_kernel_name(h) == b"k_obs_inhand<false>"  # (gaussian noise: not the lean instantiation)
        libimx.imx_plan_destroy(h)
    off = p.blob[H["OBS_OFF"]]
    bad = p.blob.copy(); bad[off + 1 * REC + R["AUX0"]] = 2  # object_pos
    assert create(bad) != 0 and b"asset selector" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[H["CMD_DIM"]] = 3
    assert create(bad) != 0
    bad = p.blob.copy(); bad[bad[H["REW_OFF"]] + R["OP"]] = W_OPS["TRACK_POS_L2"] + 1
    assert create(bad) != 0 and b"unknown reward op" in libimx.imx_last_error()
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"_Z17k_term_rew_inhand" in data and b"_Z12k_obs_inhandILb1EE" in data and b"_Z12k_obs_inhandILb0EE" in data and b"_Z16k_inhand_command" in data
    # the state struct keeps its size and its last field: the new tensors and the command term travel in structs of their own
    assert _lib.STATE_FIELDS[-1] == "object_root_pos_w" and ctypes.sizeof(_lib.ImxState) == 248 == int(libimx.imx_struct_size(0))
    assert _lib.OBJECT_STATE_FIELDS == NEW_STATE and int(libimx.imx_struct_size(16)) == ctypes.sizeof(_lib.ImxObjectState) == 32
    assert int(libimx.imx_struct_size(5)) == 1944 == ctypes.sizeof(_lib.ImxOrch)
    assert int(libimx.imx_struct_size(15)) == ctypes.sizeof(_lib.ImxInhandCommand) > 0 and int(libimx.imx_struct_size(17)) == 0
    assert '#include "imx_object_state.h"' in open(_abi.HEADER).read()
    res, args = _lib._SIGNATURES["imx_plan_bind_object_state"]
    assert res is ctypes.c_int and len(args) == 2 and args[1] is ctypes.POINTER(_lib.ImxObjectState)
    assert libimx.imx_plan_bind_object_state(None, None) != 0 and b"null plan" in libimx.imx_last_error()
    p = compile_plan(ic.load_fixture()["env"], ALLEGRO_HAND)
    assert create(p.blob) == 0
    assert libimx.imx_plan_bind_object_state(h, ctypes.byref(_lib.ImxObjectState())) == 0 and libimx.imx_plan_bind_object_state(h, None) == 0
    libimx.imx_plan_destroy(h)
    text = open(_abi.HEADER).read()
    assert '#include "imx_inhand_command_struct.h"' in text and "orientation_command.py:22-124" in text
    res, args = _lib._SIGNATURES["imx_inhand_command"]
    assert res is ctypes.c_int and len(args) == 5 and args[0] is ctypes.POINTER(_lib.ImxInhandCommand)
    # the entry point's argument checks need no GPU: nothing is launched with what they name
    c = _lib.ImxInhandCommand()
    assert libimx.imx_inhand_command(ctypes.byref(c), 8, 0.1, 1, None) != 0 and b"resampling_time_range" in libimx.imx_last_error()
    c.cfg[0], c.cfg[1], c.cfg[2] = 1.0, 2.0, 0.1
    assert libimx.imx_inhand_command(ctypes.byref(c), 8, 0.1, 1, None) != 0 and b"pos_command_w missing" in libimx.imx_last_error()
    assert libimx.imx_inhand_command(ctypes.byref(c), 8, 0.1, 0, None) != 0 and b"nothing to do" in libimx.imx_last_error()
    assert libimx.imx_inhand_command(ctypes.byref(c), 0, 0.1, 1, None) != 0 and b"N out of range" in libimx.imx_last_error()
    assert libimx.imx_inhand_command(ctypes.byref(c), 8, 0.1, 2, None) != 0 and b"unknown flags" in libimx.imx_last_error()
