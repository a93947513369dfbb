"""CPU: Isaac-Open-Drawer-Franka-v0 compiles to the fused path -- the seven manipulation/cabinet rewards, the frame observations, the
joint observations on the scene's second articulation, the plan's frame table -- nothing of the existing tasks' plans moves, what the
resolver and the term compiler refuse is refused with its reason, the C interface carries the new state struct, and the restatement
of tests/_cabinet_oracle.py and the host program reproduce the fixtures of the real reference."""

import copy
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import _cabinet_cases as cc
import _cabinet_oracle as co
from _task_space_cases import ROOT, build_host_program, host_compiler
from _util import FLOAT_TOL, assert_close

from isaaclab_amd import plan as planmod
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import O_OPS, T_OPS, W_OPS, compile_plan
from isaaclab_amd.robots import FRANKA_PANDA, FRANKA_PANDA_CABINET, ROBOTS, SceneEntityResolver

H, R, REC = planmod.H, planmod.R, planmod.REC_WORDS
NEW_STATE = ("joint_pos", "joint_vel", "body_pos_w", "body_quat_w")
READS = ("articulation_body_pos_w", "articulation_body_quat_w", "articulation_joint_pos", "articulation_joint_vel")
CABINET_REWARDS = ("APPROACH_EE_HANDLE", "ALIGN_EE_HANDLE", "APPROACH_GRIPPER_HANDLE", "ALIGN_GRASP_AROUND_HANDLE", "GRASP_HANDLE", "OPEN_DRAWER_BONUS",
                   "MULTI_STAGE_OPEN_DRAWER")


def _recs(blob, off_key, n):
    off = blob[H[off_key]]
    return [blob[off + i * REC: off + (i + 1) * REC] for i in range(n)]


def _wf(word):
    return float(np.asarray(word, np.int32).view(np.float32))


def _env():
    return copy.deepcopy(cc.load_fixture()["env"])


def _frame(blob, ft, index):
    w = blob[ft + 4 + 9 * index: ft + 4 + 9 * (index + 1)]
    return int(w[0]), int(w[1]), tuple(_wf(x) for x in w[2:5]), tuple(_wf(x) for x in w[5:9])


def test_robot_spec_and_second_articulation():
    r = ROBOTS["franka_panda_cabinet"]
    assert r is FRANKA_PANDA_CABINET and r.command_dim == 3 and r.joint_names == FRANKA_PANDA.joint_names and r.body_names == FRANKA_PANDA.body_names
    fx = cc.load_fixture()
    res = SceneEntityResolver(r, fx["env"]["scene"])
    s = res.second
    assert list(res.articulations) == ["cabinet"] and s.joint_names == cc.CABINET_JOINTS and s.body_names == cc.CABINET_BODIES
    assert s.default_joint_pos == [0.0] * 4 and s.default_joint_vel == [0.0] * 4 and s.root_pos == (0.8, 0.0, 0.4) and s.root_rot == (0.0, 0.0, 0.0, 1.0)
    assert res.ids({"name": "cabinet", "joint_names": ["drawer_top_joint"]}, "joint") == [3]
    assert res.ids({"name": "cabinet", "body_names": "drawer_handle_top"}, "body") == [8]
    ee, cab = res.frame_table("ee_frame"), res.frame_table("cabinet_frame")
    assert ee.asset == 0 and ee.target_frame_names == ["ee_tcp", "tool_leftfinger", "tool_rightfinger"] and ee.source.body == "panda_link0"
    assert [f.body for f in ee.targets] == ["panda_hand", "panda_leftfinger", "panda_rightfinger"] and ee.targets[0].pos == (0.0, 0.0, 0.1034)
    assert cab.asset == 1 and cab.source.body == "sektion" and cab.targets[0].body == "drawer_handle_top" and cab.targets[0].body_id == 8
    assert cab.targets[0].pos == (0.305, 0.0, 0.01) and cab.targets[0].rot == (0.5, 0.5, -0.5, -0.5)
    assert res.frame("ee_frame") == ("panda_hand", (0.0, 0.0, 0.1034), (1.0, 0.0, 0.0, 0.0))  # the Lift call site's form is unchanged


def test_fixture_compiles_to_the_live_cfg_blob_with_no_python_term():
    fx = cc.load_fixture()
    assert fx["task"] == cc.TASK and fx["robot"] == cc.ROBOT
    p = compile_plan(fx["env"], FRANKA_PANDA_CABINET)
    z = np.load(os.path.join(cc.GOLDEN_DIR, cc.TASK + ".npz"))
    assert np.array_equal(np.asarray(p.blob), z["live_cfg/blob"])  # what the live cfg object compiled to (tools/gen_golden_cabinet.py)
    assert (p.action_dim, p.processed_action_dim, p.obs_dim, p.cmd_dim) == (cc.A, cc.PA, cc.D, 3)
    assert p.n_ext_rew == 0 and p.n_ext_term == 0 and p.n_ext_obs == 0
    assert p.state_reads == READS
    assert [t.name for t in p.reward_terms] == list(cc.REWARDS)
    rew = _recs(p.blob, "REW_OFF", 9)
    assert [r[R["OP"]] for r in rew] == [W_OPS[o] for o in CABINET_REWARDS] + [W_OPS["ACTION_RATE_L2"], W_OPS["JOINT_VEL_L2"]]
    assert W_OPS["APPROACH_EE_HANDLE"] == W_OPS["TRACK_POS_L2"] + 2  # (the op number in between stays reserved)
    ft = p.frame_table_off
    assert ft > 0 and all(r[R["AUX0"]] == ft for r in rew[:7])
    assert _wf(rew[0][R["P0"]]) == cc.f32(cc.APPROACH_THRESHOLD) and _wf(rew[2][R["P0"]]) == cc.f32(cc.OFFSET)
    assert _wf(rew[4][R["P0"]]) == cc.f32(cc.GRASP_THRESHOLD) and _wf(rew[4][R["P1"]]) == cc.f32(cc.OPEN_JOINT_POS)
    gl = rew[4]
    assert list(p.blob[gl[R["IDS_OFF"]]: gl[R["IDS_OFF"]] + gl[R["NIDS"]]]) == [7, 8]  # the robot's finger joints
    for r in rew[5:7]:  # the drawer joint of the second articulation
        assert r[R["AUX1"]] == 1 and r[R["NIDS"]] == 1 and p.blob[r[R["IDS_OFF"]]] == 3
    assert [_wf(r[R["WEIGHT"]]) for r in rew[:7]] == [cc.f32(cc.WEIGHTS[n]) for n in cc.REWARDS[:7]]
    term = _recs(p.blob, "TERM_OFF", 1)
    assert [t[R["OP"]] for t in term] == [T_OPS["TIME_OUT"]]
    # the frame table: widths of the second articulation, target counts, then source and targets of both sensors
    assert list(p.blob[ft: ft + 4]) == [4, 9, 3, 1]
    names = FRANKA_PANDA.body_names
    assert _frame(p.blob, ft, 0) == (names.index("panda_link0"), 0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    assert _frame(p.blob, ft, 1) == (names.index("panda_hand"), 0, (0.0, 0.0, cc.f32(0.1034)), (1.0, 0.0, 0.0, 0.0))
    assert _frame(p.blob, ft, 2) == (names.index("panda_leftfinger"), 0, (0.0, 0.0, cc.f32(0.046)), (1.0, 0.0, 0.0, 0.0))
    assert _frame(p.blob, ft, 3) == (names.index("panda_rightfinger"), 0, (0.0, 0.0, cc.f32(0.046)), (1.0, 0.0, 0.0, 0.0))
    assert _frame(p.blob, ft, 4) == (0, 1, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    assert _frame(p.blob, ft, 5) == (8, 1, (cc.f32(0.305), 0.0, cc.f32(0.01)), (0.5, 0.5, -0.5, -0.5))
    assert set(p.frame_tables) == {"ee_frame", "cabinet_frame"}
    # observations
    g = p.obs_groups[0]
    assert [t.name for t in g.terms] == list(cc.COLS) and [hi - lo for lo, hi in cc.COLS.values()] == g.term_widths and g.enable_corruption
    obs = {t.name: r for t, r in zip(g.terms, _recs(p.blob, "OBS_OFF", len(g.terms)))}
    assert obs["joint_pos"][R["OP"]] == O_OPS["JOINT_POS_REL"] and obs["joint_vel"][R["OP"]] == O_OPS["JOINT_VEL_REL"]
    for name, op in (("cabinet_joint_pos", "ARTICULATION_JOINT_POS_REL"), ("cabinet_joint_vel", "ARTICULATION_JOINT_VEL_REL")):
        r = obs[name]
        assert r[R["OP"]] == O_OPS[op] and r[R["NIDS"]] == 1 and p.blob[r[R["IDS_OFF"]]] == 3 and r[R["AUX0"]] == ft and _wf(p.blob[r[R["P2"]]]) == 0.0
    assert obs["rel_ee_drawer_distance"][R["OP"]] == O_OPS["REL_EE_DRAWER_DISTANCE"] and obs["rel_ee_drawer_distance"][R["AUX0"]] == ft
    act = _recs(p.blob, "ACT_OFF", 2)
    assert act[0][R["OP"]] == planmod.A_JOINT_AFFINE and act[1][R["OP"]] == planmod.A_BINARY_JOINT and p.blob[H["PA"]] == cc.PA
    ag = fx["agent"]
    assert ag["policy"]["actor_hidden_dims"] == [256, 128, 64] and ag["num_steps_per_env"] == 96 and ag["empirical_normalization"] is False


@pytest.mark.parametrize("task,relative", [(cc.TASK_IK_ABS, False), (cc.TASK_IK_REL, True)])
def test_the_ik_variants_compile_to_the_live_cfg_blob(task, relative):
    fx = cc.load_fixture(task)
    assert fx["task"] == task and fx["robot"] == cc.ROBOT
    p = compile_plan(fx["env"], FRANKA_PANDA_CABINET)
    z = np.load(os.path.join(cc.GOLDEN_DIR, task + ".npz"))
    assert np.array_equal(np.asarray(p.blob), z["live_cfg/blob"])
    assert (p.action_dim, p.processed_action_dim, p.obs_dim) == cc.DIMS[task] and p.n_ext_rew == p.n_ext_term == p.n_ext_obs == 0
    assert p.state_reads == READS and p.frame_table_off > 0
    (ik,) = p.ik_terms
    assert (ik.command_type, ik.use_relative_mode, ik.ik_method, ik.body_name, ik.offset_pos) == ("pose", relative, "dls", "panda_hand", (0.0, 0.0, 0.107))
    assert ik.joint_ids == list(range(7)) and ik.width == (6 if relative else 7) and [t.name for t in p.action_terms] == ["arm_action", "gripper_action"]
    assert [r[R["OP"]] for r in _recs(p.blob, "REW_OFF", 7)] == [W_OPS[o] for o in CABINET_REWARDS]
    meta = json.loads(str(z["meta_json"]))
    assert cc.margins_hold(meta["branches"]) and (meta["num_envs"], meta["steps"]) == (32, 2) and "step0/in/jacobians" in z.files


def test_the_terms_the_task_cfg_leaves_out_compile_too():
    env = _env()
    pol = env["observations"]["policy"]
    pol["ee_pos"] = {"func": f"{cc.CABINET}.observations:ee_pos", "params": {}}
    pol["ee_quat"] = {"func": f"{cc.CABINET}.observations:ee_quat", "params": {}}
    pol["ee_quat_raw"] = {"func": f"{cc.CABINET}.observations:ee_quat", "params": {"make_quat_unique": False}}
    pol["fingertips_pos"] = {"func": f"{cc.CABINET}.observations:fingertips_pos", "params": {}}
    p = compile_plan(env, FRANKA_PANDA_CABINET)
    assert p.obs_dim == cc.D + 3 + 4 + 4 + 6
    recs = {t.name: r for t, r in zip(p.obs_groups[0].terms, _recs(p.blob, "OBS_OFF", len(p.obs_groups[0].terms)))}
    assert recs["ee_pos"][R["OP"]] == O_OPS["EE_POS"] and recs["ee_pos"][R["DIM"]] == 3
    assert recs["ee_quat"][R["OP"]] == O_OPS["EE_QUAT"] and recs["ee_quat"][R["FLAGS"]] & planmod.F_QUAT_UNIQUE  # (the function's default)
    assert not recs["ee_quat_raw"][R["FLAGS"]] & planmod.F_QUAT_UNIQUE
    assert recs["fingertips_pos"][R["OP"]] == O_OPS["FINGERTIPS_POS"] and recs["fingertips_pos"][R["DIM"]] == 6
    assert all(recs[n][R["AUX0"]] == p.frame_table_off for n in ("ee_pos", "ee_quat", "fingertips_pos"))
    del env["rewards"]["approach_gripper_handle"]["params"]["offset"]  # the function's default
    assert _wf(_recs(compile_plan(env, FRANKA_PANDA_CABINET).blob, "REW_OFF", 3)[2][R["P0"]]) == cc.f32(0.04)
    # a plan that reads only the joints of the second articulation still carries the table (its widths)
    env = _env()
    env["rewards"] = {k: v for k, v in env["rewards"].items() if k in ("action_rate_l2", "joint_vel")}
    del env["observations"]["policy"]["rel_ee_drawer_distance"]
    p = compile_plan(env, FRANKA_PANDA_CABINET)
    assert p.state_reads == ("articulation_joint_pos", "articulation_joint_vel") and list(p.blob[p.frame_table_off: p.frame_table_off + 2]) == [4, 9]


def test_the_module_is_closed_in_all_three_managers():
    for kind, path in (("rewards", ("rewards", "grasp_handle")), ("observations", ("observations", "policy", "rel_ee_drawer_distance"))):
        env = _env()
        node = env
        for k in path:
            node = node[k]
        node["func"] = f"{cc.CABINET}.{kind}:not_a_cabinet_term"
        with pytest.raises(NotImplementedError, match="has no fused op"):
            compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["terminations"]["t"] = {"func": f"{cc.CABINET}.rewards:align_grasp_around_handle", "time_out": False, "params": {}}
    with pytest.raises(NotImplementedError, match="has no fused op"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()  # rel_ee_object_distance reads a scene entity "object" the task does not have: no op
    env["observations"]["policy"]["rel_ee_drawer_distance"]["func"] = f"{cc.CABINET}.observations:rel_ee_object_distance"
    with pytest.raises(NotImplementedError, match="has no fused op"):
        compile_plan(env, FRANKA_PANDA_CABINET)


def test_resolver_and_compiler_refusals():
    env = _env()
    env["scene"]["ee_frame"]["target_frames"][1]["prim_path"] = "{ENV_REGEX_NS}/Robot/panda_thumb"
    with pytest.raises(ValueError, match="frame 'tool_leftfinger' sits on 'panda_thumb', which is a body neither of the robot"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["scene"]["ee_frame"]["target_frames"][2]["prim_path"] = "{ENV_REGEX_NS}/Cabinet/drawer_top"
    with pytest.raises(NotImplementedError, match="its frames sit on bodies of the robot and of 'cabinet'.*one articulation"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["scene"]["cupboard"] = copy.deepcopy(env["scene"]["cabinet"])
    with pytest.raises(NotImplementedError, match="2 articulations beside the robot"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    del env["scene"]["cabinet"]["joint_names"]
    with pytest.raises(ValueError, match="'cabinet' is an Articulation without 'joint_names' / 'body_names' tables"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["scene"]["ee_frame"]["target_frames"] = env["scene"]["ee_frame"]["target_frames"][:1]
    with pytest.raises(ValueError, match="reads the fingertip frames"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    del env["scene"]["cabinet_frame"]
    with pytest.raises(ValueError, match="'cabinet_frame' is not a FrameTransformer of the scene"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    # an op that reads the robot's tensors only does not take the second articulation's ids silently
    env = _env()
    env["rewards"]["joint_vel"]["params"] = {"asset_cfg": {"name": "cabinet", "joint_names": ["drawer_top_joint"]}}
    with pytest.raises(NotImplementedError, match="names the scene's second articulation 'cabinet'"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["observations"]["policy"]["cabinet_joint_pos"]["func"] = f"{cc.MDP}.observations:joint_pos"
    with pytest.raises(NotImplementedError, match="names the scene's second articulation 'cabinet'"):
        compile_plan(env, FRANKA_PANDA_CABINET)
    env = _env()
    env["rewards"]["open_drawer_bonus"]["params"]["asset_cfg"]["joint_names"] = ["no_such_joint"]
    with pytest.raises(ValueError, match="Not all regular expressions are matched"):
        compile_plan(env, FRANKA_PANDA_CABINET)


def test_every_existing_fixture_keeps_its_blob_free_of_the_new_ops():
    cfg_dir = os.path.join(os.path.dirname(planmod.__file__), "configs")
    tasks = sorted(f[:-5] for f in os.listdir(cfg_dir) if f.endswith(".json") and not f.endswith(".managers.json"))
    golden = ["Isaac-Lift-Cube-Franka-v0", "Isaac-Repose-Cube-Allegro-v0", "Isaac-Navigation-Flat-Anymal-C-v0"]
    assert len(tasks) >= 15 and cc.TASK not in tasks
    for task in tasks + [os.path.join(cc.GOLDEN_DIR, t + ".json") for t in golden]:
        fx = load_task_cfg(task)
        p = compile_plan(fx["env"], ROBOTS[fx["robot"]])
        assert p.frame_table_off == 0 and p.frame_tables == {} and not any(n.startswith("articulation_") for n in p.state_reads), task
        assert all(r[R["OP"]] <= O_OPS["GOAL_QUAT_DIFF"] for r in _recs(p.blob, "OBS_OFF", p.blob[H["NOBS"]])), task
        assert all(r[R["OP"]] <= W_OPS["TRACK_POS_L2"] for r in _recs(p.blob, "REW_OFF", p.blob[H["NREW"]])), task
    with pytest.raises(FileNotFoundError):
        load_task_cfg(cc.TASK)  # data derived from the reference lives under tests/golden only


def test_blob_validates_through_the_c_abi_and_the_library_has_the_kernels(libimx):
    from isaaclab_amd import _abi, _lib

    h = ctypes.c_void_p()

    def create(b):
        b = np.ascontiguousarray(b, np.int32)
        return libimx.imx_plan_create(b.ctypes.data, b.size, ctypes.byref(h))

    p = compile_plan(cc.load_fixture()["env"], FRANKA_PANDA_CABINET)
    assert create(p.blob) == 0, libimx.imx_last_error()
    assert libimx.imx_plan_obs_dim(h) == cc.D and libimx.imx_observations_kernel_name(h) == b"k_obs_cabinet<true>"
    assert libimx.imx_plan_bind_articulation_state(h, ctypes.byref(_lib.ImxArticulationState())) == 0
    assert libimx.imx_plan_bind_articulation_state(h, None) == 0
    # imx_plan_update: the same blob is taken; one whose frame table states other widths at the same offset is another shape
    same = np.ascontiguousarray(p.blob, np.int32)
    assert libimx.imx_plan_update(h, same.ctypes.data, same.size, None) == 0, libimx.imx_last_error()
    for word, value in ((0, 5), (1, 10)):  # J2, B2
        other = same.copy()
        other[p.frame_table_off + word] = value
        assert libimx.imx_plan_update(h, other.ctypes.data, other.size, None) != 0 and b"different shape" in libimx.imx_last_error(), word
    libimx.imx_plan_destroy(h)
    assert libimx.imx_plan_bind_articulation_state(None, None) != 0 and b"null plan" in libimx.imx_last_error()
    ft, rew = p.frame_table_off, p.blob[H["REW_OFF"]]
    bad = p.blob.copy(); bad[ft + 4 + 9 * 5] = 9  # the handle's body: one past the cabinet's nine
    assert create(bad) != 0 and b"frame 5 sits on body 9 outside [0,9)" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[ft + 4 + 9 * 1 + 1] = 2
    assert create(bad) != 0 and b"asset word 2" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[ft + 2] = 2  # two ee_frame targets: no right fingertip
    assert create(bad) != 0 and b"reads the two fingertip frames" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[rew + 5 * REC + R["AUX0"]] = ft + 1
    assert create(bad) != 0 and b"names the frame table at word" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[bad[rew + 5 * REC + R["IDS_OFF"]]] = 4  # the drawer joint: one past the cabinet's four
    assert create(bad) != 0 and b"second-articulation joint index 4" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[rew + R["OP"]] = W_OPS["TRACK_POS_L2"] + 1
    assert create(bad) != 0 and b"unknown reward op" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[rew + R["OP"]] = W_OPS["MULTI_STAGE_OPEN_DRAWER"] + 1
    assert create(bad) != 0 and b"unknown reward op" in libimx.imx_last_error()
    bad = p.blob.copy(); bad[bad[H["OBS_OFF"]] + R["OP"]] = O_OPS["ARTICULATION_JOINT_VEL_REL"] + 1
    assert create(bad) != 0 and b"unknown observation op" in libimx.imx_last_error()
    data = open(_lib.LIB_PATH, "rb").read()
    for sym in (b"_Z18k_term_rew_cabinet", b"_Z13k_obs_cabinetILb1EE", b"_Z13k_obs_cabinetILb0EE", b"_Z19k_frame_transformer"):
        assert sym in data, sym
    # the existing structs keep their sizes; the new tensors travel in a struct of their own
    assert ctypes.sizeof(_lib.ImxState) == 248 == int(libimx.imx_struct_size(0)) and int(libimx.imx_struct_size(1)) == 216
    assert int(libimx.imx_struct_size(5)) == 1944 and int(libimx.imx_struct_size(16)) == 32
    assert _lib.ARTICULATION_STATE_FIELDS == NEW_STATE and int(libimx.imx_struct_size(18)) == ctypes.sizeof(_lib.ImxArticulationState) == 32
    assert all(int(libimx.imx_struct_size(k)) == 0 for k in (9, 14, 17, 19))
    text = open(_abi.HEADER).read()
    assert '#include "imx_articulation_state.h"' in text and "imx_articulation_state_t" not in _abi.STRUCTS and len(_abi.STRUCTS) == 8
    res, args = _lib._SIGNATURES["imx_plan_bind_articulation_state"]
    assert res is ctypes.c_int and len(args) == 2 and args[1] is ctypes.POINTER(_lib.ImxArticulationState)
    # imx_frame_transformer's argument checks need no GPU: nothing is launched with what they name
    one = (ctypes.c_float * 8)()
    fr = np.zeros((2, 9), np.int32)
    ok = lambda *a: libimx.imx_frame_transformer(*a, None)  # noqa: E731
    assert ok(4, 1, 3, None, one, one, fr.ctypes.data, one, one, one, one, one, one) != 0 and b"body_pos_w missing" in libimx.imx_last_error()
    assert ok(4, 1, 3, one, None, one, fr.ctypes.data, one, one, one, one, one, one) != 0 and b"body_quat_w missing" in libimx.imx_last_error()
    assert ok(4, 0, 3, one, one, one, fr.ctypes.data, one, one, one, one, one, one) != 0 and b"0 target frames" in libimx.imx_last_error()
    fr[1, 0] = 3
    assert ok(4, 1, 3, one, one, one, fr.ctypes.data, one, one, one, one, one, one) != 0 and b"frame 1 sits on body 3 outside [0, 3)" in libimx.imx_last_error()


def test_the_new_struct_against_a_cxx_compiler(tmp_path):
    """Size and offsets of imx_articulation_state_t as a C++ compiler reads the header, by the recipe of tests/test_abi.py."""
    from isaaclab_amd import _lib

    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    cls = _lib.ImxArticulationState
    lines = ['#include <cstddef>', '#include "imx.h"', f'static_assert(sizeof(imx_articulation_state_t) == {ctypes.sizeof(cls)}, "size");']
    for field, _ in cls._fields_:
        f = getattr(cls, field)
        lines.append(f'static_assert(offsetof(imx_articulation_state_t, {field}) == {f.offset} && sizeof(imx_articulation_state_t::{field}) == {f.size}, "{field}");')
    lines += ['static_assert(IMX_W_APPROACH_EE_HANDLE == IMX_W_TRACK_POS_L2 + 2, "reserved op");',
              f'static_assert(IMX_FRAME_WORDS == {_lib.FRAME_WORDS} && IMX_FT_HEADER_WORDS == {_lib.FT_HEADER_WORDS}, "frame table");']
    src = tmp_path / "articulation_state_check.cpp"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the header can be included alone
    src.write_text('#include "imx_articulation_state.h"\nstatic_assert(sizeof(imx_articulation_state_t) == 4 * sizeof(void*), "size");\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_restatement_reproduces_the_step_fixture():
    """tests/_cabinet_oracle.py in fp32 on the fixture's inputs against what the real reference managers computed, and the fixture's
    branch counts: every branch taken, no env inside a margin."""
    g = cc.golden()
    scene = cc.scene_of(g.fixture)
    _, second, ee, cab, drawer, gripper = scene
    snaps = g.snapshots()
    for t in range(g.steps):
        s = {n: snaps[t + 1][n] for n in cc.NAMES}
        r = co.terms(s, ee, cab, drawer, gripper, cc.APPROACH_THRESHOLD, cc.GRASP_THRESHOLD, cc.OFFSET, cc.OPEN_JOINT_POS)
        sr, obs = g.t(f"step{t}/step_reward"), g.t(f"step{t}/obs")
        for i, name in enumerate(cc.REWARDS[:7]):
            assert_close(r[name].float() * cc.WEIGHTS[name], sr[:, i], FLOAT_TOL, f"step{t} {name}")
        assert torch.equal(r["align_grasp_around_handle"] * cc.WEIGHTS["align_grasp_around_handle"], sr[:, 3])
        for name in ("cabinet_joint_pos", "cabinet_joint_vel", "rel_ee_drawer_distance"):
            lo, hi = cc.COLS[name]
            assert_close(r[name], obs[:, lo:hi], FLOAT_TOL, f"step{t} {name}")
    c = cc.branch_counts([{n: sn[n] for n in cc.NAMES} for sn in snaps[1:]], scene)
    assert c == g.meta["branches"]
    assert cc.margins_hold(c) and all(v > 0 for k, v in c.items() if not k.startswith("min_")), c
    assert g.meta["processed_action_dim"] == cc.PA and g.meta["action_dim"] == cc.A and g.meta["obs_dim"] == cc.D
    assert g.meta["cabinet"] == {"joint_names": cc.CABINET_JOINTS, "body_names": cc.CABINET_BODIES}


@pytest.mark.parametrize("case", cc.FT_CASES)
def test_the_restatement_reproduces_the_frame_transformer_fixture(case):
    fg = cc.FrameGolden()
    bp, bq = fg.bodies(case)
    out, ref = co.frame_transformer(fg.sensor(case), bp, bq), fg.expected(case)
    for k in cc.FT_OUTPUTS:
        assert out[k].shape == ref[k].shape
        assert_close(out[k], ref[k], FLOAT_TOL, f"{case} {k}")
    out64 = co.frame_transformer(fg.sensor(case), bp.double(), bq.double())
    for k in cc.FT_OUTPUTS:  # (positions are a few tens of metres: fp32 rounds them at 4e-6)
        assert float((out64[k] - ref[k].double()).abs().max()) <= 2.0e-5, (case, k)
    assert len(fg.sensor(case)[1]) == (1 if case == "cabinet_frame" else 3)
    assert (fg.sensor(case)[0][1] != (0.0, 0.0, 0.0)) == (case == "ee_frame_source_offset")


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_host_program_reproduces_the_frame_transformer_fixture(tmp_path, sanitize):
    """tools/frame_transformer_host.cpp -- the kernels' per-lane function as host C++ -- on the fixture; also built with the address and
    undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
    if host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    try:
        exe = build_host_program("frame_transformer_host", str(tmp_path), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if sanitize else ())
    except subprocess.CalledProcessError:
        if sanitize:
            pytest.skip("this compiler has no sanitizer runtimes")
        raise
    fg = cc.FrameGolden()
    for case in cc.FT_CASES:
        inp, outp = str(tmp_path / f"{case}.in"), str(tmp_path / f"{case}.out")
        fg.host_file(inp, case)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out, ref = fg.read_host_output(outp, case), fg.expected(case)
        for k in cc.FT_OUTPUTS:
            assert_close(out[k], ref[k], FLOAT_TOL, f"{case} {k}")
    bad = str(tmp_path / "bad.in")
    fg.host_file(bad, "ee_frame")
    raw = bytearray(open(bad, "rb").read())
    raw[16:20] = np.asarray([99], np.int32).tobytes()  # the source frame's body id
    open(bad, "wb").write(bytes(raw))
    r = subprocess.run([exe, bad, str(tmp_path / "bad.out")], capture_output=True, text=True)
    assert r.returncode == 2 and "sits on body 99" in r.stderr


def test_the_generator_takes_every_branch_at_4096_envs():
    """The feed's own generator (no tweak): every branch of the cabinet terms occurs at the benchmark's env count; asking for the second
    articulation's state changes no other tensor."""
    from isaaclab_amd.state_feed import ARTICULATION_STATE, StateFeed

    scene = cc.scene_of()
    plan, second = scene[0], scene[1]
    feed = StateFeed(FRANKA_PANDA_CABINET, 4096, "cpu", seed=42, num_snapshots=1)
    before = {n: feed[n].clone() for n in feed.names()}
    feed.ensure_articulation_state(second, plan.frame_tables)
    assert all(torch.equal(feed[n], v) for n, v in before.items()) and all(n in feed.names() for n in ARTICULATION_STATE)
    assert feed["articulation_joint_pos"].shape == (4096, 4) and feed["articulation_body_quat_w"].shape == (4096, 9, 4)
    q = feed["articulation_joint_pos"][:, 3]
    assert float(q.min()) >= -0.05 and float(q.max()) <= 0.45
    c = cc.branch_counts([{n: feed[n] for n in cc.NAMES}], scene)
    assert all(v > 20 for k, v in c.items() if not k.startswith("min_")), c
