"""CPU: the Imu sensor below the GPU -- the torch oracle (tests/_imu_oracle.py) and the kernel's per-env device function compiled for the
host (tools/imu_host.cpp) against the fixture recorded from the REAL class (tests/golden/imu_sensor.json, tools/gen_golden_imu.py), the
plan of the fixture cfg (tests/golden/Isaac-Velocity-Flat-Anymal-C-v0-imu.json) and every refusal."""

import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _imu_oracle as io
from _task_space_cases import build_host_program, host_compiler
from isaaclab_amd import _abi, _lib
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import O_OPS, compile_plan
from isaaclab_amd.robots import ROBOTS, SceneEntityResolver

_OBS = "isaaclab.envs.mdp.observations:"


@pytest.fixture(scope="module")
def fx():
    return io.with_input_tensors(io.load_fixture(), lambda t: t)


@pytest.fixture(scope="module")
def oracle64_states(fx):
    """The fp64 oracle's state after every recorded call: {call index: {sensor: state}} -- the reference of every tolerance."""
    return {k: st for k, _, st in io.replay(fx, io.make_oracles(fx, torch.float64), lambda s: s.state())}


# ------------------------------------------------------------------------------------------------- fixture preconditions
def test_fixture_preconditions(fx):
    """On the fixture alone, so that no test on it can pass vacuously: imu_foot is read with some envs outdated and some not; an env is
    reset while it moves; dt changes in the middle; half of the envs have a centre of mass off the link origin; the first read raised."""
    N = fx["N"]
    reads = [c for c in fx["calls"] if c["op"] == "data"]
    assert any(0 < sum(c["outdated_before"]["imu_foot"]) < N for c in reads)
    # update_period 0: every env is outdated at every read but the one after the forced recompute, where only the reset env is
    assert sorted(sum(c["outdated_before"]["imu"]) for c in reads) == [1] + [N] * (len(reads) - 1)
    inputs, moving_reset = None, False
    for c in fx["calls"]:
        if c["op"] == "inputs":
            inputs = c
        if c["op"] == "reset":
            v = io.f32(inputs["lin_vel_w"])[c["env_ids"]]
            moving_reset |= bool((v.abs().max(dim=1).values > 0).all())
            prev = io.f32(c["state"]["imu"]["prev_lin_vel_w"])[c["env_ids"]]
            assert float(prev.abs().max()) > 0.0  # the previous velocity survives the reset
            assert float(io.f32(c["state"]["imu"]["quat_w"])[c["env_ids"]].abs().max()) == 0.0
    assert moving_reset
    assert len({c["dt"] for c in fx["calls"] if c["op"] == "update"}) == 2
    assert any(c.get("force_recompute") for c in fx["calls"] if c["op"] == "update")
    com = io.f32(fx["com_pos_b"])
    assert int((com.abs().sum(1) > 0).sum()) == N // 2
    assert fx["first_read_error"] == "The update function must be called before the data buffers are accessed the first time."
    assert fx["sensors"]["imu_foot"]["update_period"] == pytest.approx(2.5 * fx["physics_dt"]) and fx["sensors"]["imu"]["update_period"] == 0.0


# ------------------------------------------------------------------------------------------------- oracle and host build
def test_oracle_fp32_reproduces_the_fixture(fx, oracle64_states):
    states = {k: st for k, _, st in io.replay(fx, io.make_oracles(fx, torch.float32), lambda s: s.state())}
    io.check_against_fixture(fx, oracle64_states, states, "fp32 oracle")


def test_oracle_refuses_a_read_before_update(fx):
    with pytest.raises(RuntimeError, match="update function must be called before"):
        io.make_oracles(fx, torch.float32)["imu"].data


def test_oracle_quirks(fx):
    """The accelerations divide by the dt of the LAST update, not by the time since the last refresh; the gravity bias is added in the
    world frame; the reset keeps the previous velocity."""
    o = io.ImuOracle(1, dtype=torch.float64)
    p, q = torch.zeros(1, 3), torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    o.update(0.005, p, q, torch.tensor([[1.0, 0.0, 0.0]]), torch.zeros(1, 3))
    o.data
    o.update(0.005, p, q, torch.tensor([[1.5, 0.0, 0.0]]), torch.zeros(1, 3), substeps=4)  # 0.02 s pass
    assert o.data.lin_acc_b[0].tolist() == pytest.approx([0.5 / 0.005, 0.0, 9.81])
    o.reset([0])
    o.update(0.005, p, q, torch.tensor([[1.5, 0.0, 0.0]]), torch.zeros(1, 3))
    assert o.data.lin_acc_b[0].tolist() == pytest.approx([0.0, 0.0, 9.81])  # against the pre-reset 1.5, not against 0


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    if host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    return build_host_program("imu_host", str(tmp_path_factory.mktemp("imu_host")))


def run_host(exe, tmp, fx, name):
    N, cfg = fx["N"], fx["sensors"][name]
    f32b = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    calls, inputs, dt = [], None, 0.0
    for k, c in enumerate(fx["calls"]):
        if c["op"] == "inputs":
            inputs = c
            continue
        dt = c.get("dt", dt)  # Imu._dt
        mask = np.zeros(N, np.int32)
        mask[c.get("env_ids", [])] = 1
        op = {"update": 0, "reset": 1, "data": 2}[c["op"]]
        calls.append((k, np.array([op, int(bool(c.get("force_recompute")))], np.int32).tobytes() + np.float32(dt).tobytes()
                      + b"".join(f32b(inputs[n]) for n in ("pos_w", "quat_w", "lin_vel_w", "ang_vel_w")) + mask.tobytes()))
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([0x31554D49, N, len(calls), 0, 0, 0, 0, 0], np.int32).tobytes())
        f.write(f32b(cfg["offset_pos"]) + f32b(cfg["offset_rot"]) + f32b(cfg["gravity_bias"]) + f32b([cfg["update_period"]]) + f32b(fx["com_pos_b"]))
        for _, b in calls:
            f.write(b)
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    widths = [("pos_w", 3), ("quat_w", 4), ("lin_vel_b", 3), ("ang_vel_b", 3), ("lin_acc_b", 3), ("ang_acc_b", 3), ("prev_lin_vel_w", 3),
              ("prev_ang_vel_w", 3), ("timestamp", 1), ("timestamp_last_update", 1), ("is_outdated", 1)]
    per = N * sum(w for _, w in widths)
    raw = np.fromfile(tmp / "out.bin", np.float32)
    assert raw.size == per * len(calls)
    out = {}
    for (k, _), row in zip(calls, raw.reshape(len(calls), per)):
        st, o = {}, 0
        for n, w in widths:
            a = row[o:o + N * w]
            o += N * w
            st[n] = torch.from_numpy(a.view(np.int32) != 0) if n == "is_outdated" else torch.from_numpy(a.copy().reshape((N, w) if w > 1 else (N,)))
        out[k] = st
    return out


def test_host_build_reproduces_the_fixture(fx, oracle64_states, host_exe, tmp_path):
    per_sensor = {}
    for name in fx["sensors"]:
        d = tmp_path / name
        d.mkdir()
        per_sensor[name] = run_host(host_exe, d, fx, name)
    states = {k: {name: per_sensor[name][k] for name in fx["sensors"]} for k in next(iter(per_sensor.values()))}
    io.check_against_fixture(fx, oracle64_states, states, "host build of imu_env")


# ------------------------------------------------------------------------------------------------- ABI
def test_abi_side_header():
    assert "imx_imu_t" in _abi.IMU_STRUCTS and "imx_imu_t" not in _abi.STRUCTS  # imx.h only forward-declares it
    assert _abi.DEFINES["IMX_MAX_IMU"] == 4 == _lib.MAX_IMU
    assert {"imx_imu", "imx_plan_bind_imu"} <= set(_lib.EXPORTS)
    ops = _abi.ENUMS["imx_obs_op"]
    assert (ops["IMX_O_IMU_ORIENTATION"], ops["IMX_O_IMU_ANG_VEL"], ops["IMX_O_IMU_LIN_ACC"]) == (32, 33, 34)
    assert ops["IMX_O_ARTICULATION_JOINT_VEL_REL"] == 30  # appended: no older op moved, 31 stays unknown
    assert [n for n, _ in _lib.ImxImu._fields_][:5] == ["body_index", "num_bodies", "com_per_env", "substeps", "refresh"]


def test_library_struct_size(libimx):
    assert int(libimx.imx_struct_size(27)) == ctypes.sizeof(_lib.ImxImu) > 0 and int(libimx.imx_struct_size(26)) == 0


# ------------------------------------------------------------------------------------------------- plan
@pytest.fixture(scope="module")
def task():
    return load_task_cfg(io.TASK_JSON)


def test_plan_of_the_fixture_cfg(task):
    env = task["env"]
    assert {"imu", "imu_foot"} <= set(env["scene"]) and env["scene"]["imu_foot"]["class_type"].endswith(":Imu")
    plan = compile_plan(env, ROBOTS[task["robot"]])
    base = compile_plan(load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")["env"], ROBOTS[task["robot"]])
    assert [g.name for g in plan.obs_groups] == ["policy", "foot"]
    pol, foot = plan.obs_groups
    tail = pol.terms[-3:]
    assert [(t.name, t.op, t.external) for t in tail] == [("imu_orientation", O_OPS["IMU_ORIENTATION"], None), ("imu_ang_vel", O_OPS["IMU_ANG_VEL"], None),
                                                           ("imu_lin_acc", O_OPS["IMU_LIN_ACC"], None)]
    assert [tuple(d) for d in pol.term_dims[-3:]] == [(4,), (3,), (3,)]
    assert pol.dim == base.obs_dim + 10 and plan.obs_dim == pol.dim
    assert [(t.name, t.op) for t in foot.terms] == [("foot_lin_acc", O_OPS["IMU_LIN_ACC"])] and foot.dim == 3
    assert plan.n_ext_obs == 0 and all(t.op != O_OPS["EXTERNAL"] for g in plan.obs_groups for t in g.terms)
    assert plan.imu_sensors == ("imu", "imu_foot")
    assert set(plan.state_reads) == {"body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w"}
    assert base.imu_sensors == () and not set(base.state_reads) & set(plan.state_reads)
    # every record before the imu terms is word for word the base cfg's
    ent = SceneEntityResolver(ROBOTS[task["robot"]], env["scene"])
    assert ent.imu("imu") == (0, None) and ent.imu("imu_foot") == (ROBOTS[task["robot"]].body_names.index("LF_FOOT"), None)


def _with(task, edit):
    env = copy.deepcopy(task["env"])
    edit(env)
    return env


def _imu_term(name):
    return {"func": _OBS + "imu_lin_acc", "params": {"asset_cfg": {"name": name}}, "modifiers": None, "noise": None, "clip": None, "scale": None,
            "history_length": 0, "flatten_history_dim": True}


def test_body_com_table(task):
    robot = ROBOTS[task["robot"]]
    B = robot.num_bodies
    i = robot.body_names.index("LF_FOOT")
    table = [[0.001 * b, 0.0, -0.002 * b] for b in range(B)]
    env = _with(task, lambda e: e["scene"]["imu_foot"].update(body_com_pos_b=table))
    assert SceneEntityResolver(robot, env["scene"]).imu("imu_foot") == (i, table[i])
    env = _with(task, lambda e: e["scene"]["imu_foot"].update(body_com_pos_b=[0.01, 0.02, 0.03]))
    assert SceneEntityResolver(robot, env["scene"]).imu("imu_foot") == (i, [0.01, 0.02, 0.03])
    env = _with(task, lambda e: e["scene"]["imu_foot"].update(body_com_pos_b=[[0.0, 0.0, 0.0]] * (B + 1)))
    with pytest.raises(ValueError, match=r"Imu 'imu_foot': body_com_pos_b must be"):
        SceneEntityResolver(robot, env["scene"])


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_more_than_four_imus(task):
    def edit(e):
        for k in range(5):
            e["scene"][f"imu{k}"] = dict(e["scene"]["imu"])
            e["observations"]["policy"][f"acc{k}"] = _imu_term(f"imu{k}")

    with pytest.raises(NotImplementedError, match=r"already reads 4 Imu sensors .* at most 4"):
        compile_plan(_with(task, edit), ROBOTS[task["robot"]])


@pytest.mark.parametrize("body,exc,why", [
    ("no_such_link", ValueError, "neither a body of the robot"),
    ("drawer_top", NotImplementedError, "a body of a second articulation or of the rigid object"),
    ("Object", NotImplementedError, "a body of a second articulation or of the rigid object"),
])
def test_refused_prim_path(task, body, exc, why):
    def edit(e):
        e["scene"]["imu"]["prim_path"] = "{ENV_REGEX_NS}/Robot/" + body
        e["scene"]["cabinet"] = {"class_type": "isaaclab.assets.articulation.articulation:Articulation", "prim_path": "{ENV_REGEX_NS}/Cabinet",
                                 "init_state": {"pos": [0, 0, 0], "rot": [1, 0, 0, 0], "joint_pos": {".*": 0.0}, "joint_vel": {".*": 0.0}},
                                 "joint_names": ["drawer_top_joint"], "body_names": ["sektion", "drawer_top"]}
        e["scene"]["object"] = {"class_type": "isaaclab.assets.rigid_object.rigid_object:RigidObject", "prim_path": "{ENV_REGEX_NS}/Object"}

    with pytest.raises(exc, match=rf"Imu 'imu': its prim_path ends in '{body}'.*{why}"):
        compile_plan(_with(task, edit), ROBOTS[task["robot"]])


def test_refused_debug_vis(task):
    with pytest.raises(NotImplementedError, match=r"Imu 'imu_foot': debug_vis=True"):
        compile_plan(_with(task, lambda e: e["scene"]["imu_foot"].update(debug_vis=True)), ROBOTS[task["robot"]])


def test_refused_term_on_an_entity_that_is_no_imu(task):
    for name in ("robot", "contact_forces", "nothing"):
        with pytest.raises(ValueError, match=rf"observation term 'imu_lin_acc': asset_cfg names the scene entity '{name}', which is not an Imu"):
            compile_plan(_with(task, lambda e: e["observations"]["policy"]["imu_lin_acc"]["params"].update(asset_cfg={"name": name})), ROBOTS[task["robot"]])


def test_refused_in_a_low_level_policy_group():
    nav = load_task_cfg(os.path.join(io.ROOT, "tests", "golden", "Isaac-Navigation-Flat-Anymal-C-v0.json"))
    env = copy.deepcopy(nav["env"])
    act = next(a for a in env["actions"].values() if isinstance(a, dict) and str(a.get("class_type", "")).endswith("PreTrainedPolicyAction"))
    env["scene"]["imu"] = {"class_type": "isaaclab.sensors.imu.imu:Imu", "prim_path": "{ENV_REGEX_NS}/Robot/base"}
    act["low_level_observations"]["imu_acc"] = _imu_term("imu")
    with pytest.raises(NotImplementedError, match=r"low-level observation term 'imu_acc' .*reads an Imu sensor.*not between the low-level steps"):
        compile_plan(env, ROBOTS[nav["robot"]])
