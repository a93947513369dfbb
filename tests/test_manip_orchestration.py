"""CPU: the manipulation tasks' ``_reset_idx`` -- ``reset_scene_to_default``, ``reset_root_state_uniform`` on the rigid object and the
``modify_reward_weight`` curriculum.  The numpy restatement (tests/_manip_orch_oracle.py) against the two fixtures of the REAL reference,
what the fixtures must contain, the host program (tools/manip_orch_host.cpp) that runs the kernel's per-env functions, the ABI of the new
entry points, and every refusal that needs no GPU."""

import copy
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _manip_orch_oracle as mo
from _diff_ik_cases import ROOT, host_compiler
from _util import FLOAT_TOL, assert_close
from isaaclab_amd import _abi, _lib

WHICH = ["reach", "lift"]


# ------------------------------------------------------------------------------------------------ restatement vs. the real reference
@pytest.mark.parametrize("which", WHICH)
def test_restatement_reproduces_the_reference(which):
    """Reset ids, trigger state and the step of each weight change exactly; every ``write_*_to_sim`` buffer and the weights within 1e-5."""
    g = mo.ManipOrchGolden(which)
    changes, prev = {}, None
    for tag, ids, sw, trig, weights in mo.replay(g):
        if tag != "reset":
            assert np.array_equal(ids, g.a(f"{tag}/reset_env_ids")), tag
        assert np.array_equal(trig["last"], g.a(f"{tag}/reset_last_triggered_step")), tag
        assert np.array_equal(trig["once"], g.a(f"{tag}/reset_triggered_once")), tag
        for k in g.write_keys:
            assert_close(sw[k], g.a(f"{tag}/sim_writes/{k}"), FLOAT_TOL, f"{which} {tag} sim_writes[{k}]")
        ref = g.weights(tag)
        assert list(weights) == list(ref)
        assert_close(np.array(list(weights.values())), np.array(list(ref.values())), FLOAT_TOL, f"{which} {tag} weights")
        if prev is not None:
            changes.update({n: int(tag[4:]) for n in weights if weights[n] != prev[n]})
        prev = dict(weights)
    assert changes == g.meta["weight_change_steps"] and len(changes) == 2


@pytest.mark.parametrize("which", WHICH)
def test_fixture_holds_what_the_tests_rely_on(which):
    """A fixture cannot hide a failure: after each crossed threshold there is a step without resets on which the weight is still the old
    one; some reset takes a strict subset of the envs; the Lift fixture has an env that resets twice."""
    g = mo.ManipOrchGolden(which)
    w0 = g.weights("reset")
    counts = np.zeros(g.N, int)
    subset = False
    for t in range(g.steps):
        ids = g.reset_ids(t)
        counts[ids] += 1
        subset |= 0 < len(ids) < g.N
    assert subset
    for term_name, weight, num_steps in g.curriculum:
        assert w0[term_name] != weight
        quiet = [t for t in range(g.steps) if t + 1 > num_steps and len(g.reset_ids(t)) == 0 and g.weights(f"step{t}")[term_name] == w0[term_name]]
        assert len(quiet) >= 2 and quiet[0] == num_steps, (term_name, quiet)  # (step index t has common_step_counter t + 1)
        change = g.meta["weight_change_steps"][term_name]
        assert change > quiet[-1] and len(g.reset_ids(change)) > 0 and g.weights(f"step{change}")[term_name] == weight
        assert g.weights(f"step{g.steps - 1}")[term_name] == weight
    assert g.meta["curriculum_terms"] == list(g.meta["curriculum"])
    if which == "lift":
        assert counts.max() == 2 and g.object == "object"
        funcs = [t["func"].rsplit(":", 1)[-1] for t in g.events.values()]
        assert funcs == ["reset_scene_to_default", "reset_root_state_uniform"]
        # the second term overwrites the first one's object pose: the recorded pose is not the default one on a reset row
        ids = g.reset_ids(g.meta["weight_change_steps"]["action_rate"])
        d = g.a("static/default_object_root_state")[ids, :3] + g.a("static/env_origins")[ids]
        assert np.abs(g.a(f"step{g.meta['weight_change_steps']['action_rate']}/sim_writes/object_root_pose")[ids, :3] - d).max() > 1e-3
    else:
        assert [t["func"].rsplit(":", 1)[-1] for t in g.events.values()] == ["reset_joints_by_scale"]


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine: tools/manip_orch_host.cpp cannot be built")
    exe = str(tmp_path_factory.mktemp("manip_host") / "manip_orch_host")
    subprocess.check_call([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "manip_orch_host.cpp"), "-o", exe])
    return exe


def _run_host(exe, tmp_path, default13, origins, calls):
    N = default13.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([0x31504E4D, N, len(calls), 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(default13, np.float32).tobytes() + np.ascontiguousarray(origins, np.float32).tobytes())
        for op, ranges, mask, u in calls:
            f.write(np.int32(op).tobytes() + np.asarray(ranges, np.float32).tobytes() + mask.astype(np.int32).tobytes() + np.ascontiguousarray(u, np.float32).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin", np.float32).reshape(len(calls), N * 13)
    return [(o[:N * 7].reshape(N, 7), o[N * 7:].reshape(N, 6)) for o in out]


def test_host_program_reproduces_the_lift_fixture(host_program, tmp_path):
    """The kernel's per-env functions as host C++: the robot's and the object's root writes of every tag of the Lift fixture."""
    g = mo.ManipOrchGolden("lift")
    st = g.static()
    term = g.events["reset_object_position"]["params"]
    ranges = np.concatenate([mo.axis_ranges(term.get("pose_range")).ravel(), mo.axis_ranges(term.get("velocity_range")).ravel()])
    zero = np.zeros(24, np.float32)
    obj_calls, rob_calls, tags = [], [], []
    for k, tag in enumerate(g.tags):
        mask = np.zeros(g.N, bool)
        mask[np.arange(g.N) if tag == "reset" else g.reset_ids(k - 1)] = True
        u = g.draws(k)["reset_object_position"].numpy()
        obj_calls += [(0, zero, mask, np.zeros((g.N, 12))), (1, ranges, mask, u)]  # cfg order: reset_all, then reset_object_position
        rob_calls.append((0, zero, mask, np.zeros((g.N, 12))))
        tags.append(tag)
    (tmp_path / "o").mkdir(), (tmp_path / "r").mkdir()
    obj = _run_host(host_program, tmp_path / "o", st["default_object_root_state"], st["env_origins"], obj_calls)[1::2]
    rob = _run_host(host_program, tmp_path / "r", st["default_root_state"], st["env_origins"], rob_calls)
    for tag, (op, ov), (rp, rv) in zip(tags, obj, rob):
        assert_close(op, g.a(f"{tag}/sim_writes/object_root_pose"), FLOAT_TOL, f"{tag} object pose")
        assert_close(ov, g.a(f"{tag}/sim_writes/object_root_vel"), FLOAT_TOL, f"{tag} object vel")
        assert_close(rp, g.a(f"{tag}/sim_writes/root_pose"), FLOAT_TOL, f"{tag} root pose")
        assert_close(rv, g.a(f"{tag}/sim_writes/root_vel"), FLOAT_TOL, f"{tag} root vel")


def test_host_program_matches_restatement_on_rotated_defaults(host_program, tmp_path):
    """The shipped cube only moves in x and y: random default orientations, all six pose axes and all six velocity axes."""
    rng = np.random.default_rng(5)
    N = 37
    d = rng.normal(size=(N, 13)).astype(np.float32)
    d[:, 3:7] /= np.linalg.norm(d[:, 3:7], axis=1, keepdims=True)
    org = rng.normal(size=(N, 3)).astype(np.float32) * 3
    pr = {a: tuple(sorted(rng.uniform(-2, 2, 2))) for a in mo.AXES}
    vr = {a: tuple(sorted(rng.uniform(-1, 1, 2))) for a in mo.AXES}
    u = rng.random((N, 12), np.float32)
    mask = rng.random(N) < 0.6
    mask[-1] = True
    ranges = np.concatenate([mo.axis_ranges(pr).ravel(), mo.axis_ranges(vr).ravel()])
    (pose, vel), = _run_host(host_program, tmp_path, d, org, [(1, ranges, mask, u)])
    rp, rv = mo.root_state_uniform(d[mask], org[mask], u[mask], pr, vr)
    assert_close(pose[mask], rp, FLOAT_TOL, "pose")
    assert_close(vel[mask], rv, FLOAT_TOL, "vel")
    assert not pose[~mask].any() and not vel[~mask].any()


# ------------------------------------------------------------------------------------------------ ABI
def test_existing_structs_keep_their_size_and_the_new_one_is_bound():
    assert ctypes.sizeof(_lib.ImxOrch) == 1944 and ctypes.sizeof(_lib.ImxEventTerm) == 176
    assert [f for f, _ in _lib.ImxEventTerm._fields_][8] == "asset" and _lib.ImxEventTerm.asset.offset == 124  # the former `reserved`
    ops = _abi.ENUMS["imx_event_op"]
    assert list(ops)[-1] == "IMX_E_RESET_SCENE_TO_DEFAULT" and ops["IMX_E_RESET_SCENE_TO_DEFAULT"] == 7 and ops["IMX_E_RESET_ROOT_STATE_UNIFORM"] == 1
    assert _lib.ORCH_MAX_WEIGHT_TERMS >= 4
    L = _lib.lib()
    assert int(L.imx_struct_size(5)) == 1944 and int(L.imx_struct_size(6)) == 176 and int(L.imx_struct_size(9)) == 0
    assert int(L.imx_struct_size(10)) == ctypes.sizeof(_lib.ImxOrchManip) and int(L.imx_struct_size(11)) == ctypes.sizeof(_lib.ImxWeightTerm) == 32
    assert "imx_orch_manip_t" not in _abi.STRUCTS and list(_abi.MANIP_STRUCTS) == ["imx_weight_term_t", "imx_orch_manip_t"]
    for fn in ("imx_reset_orchestrate_manip", "imx_plan_reward_weight_ptr", "imx_plan_reward_weight_get"):
        assert fn in _lib.EXPORTS and hasattr(L, fn)
    # the old entry point keeps its signature
    assert len(_lib._SIGNATURES["imx_reset_orchestrate"][1]) == 2 and len(_lib._SIGNATURES["imx_reset_orchestrate_manip"][1]) == 3


def test_the_compiler_agrees_with_the_binding_of_imx_orch_manip_t(tmp_path):
    """imx_orch_manip_t lives in include/imx_orch_manip.h (imx.h includes it) and is bound from there by the same parser: size, every
    field's offset, size and kind, and the signatures of the new entry points, as a C++ compiler reads them in imx.h."""
    from test_abi import unit

    if host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    structs = {"imx_weight_term_t": _lib.ImxWeightTerm, "imx_orch_manip_t": _lib.ImxOrchManip}
    sigs = {n: _lib._SIGNATURES[n] for n in ("imx_reset_orchestrate", "imx_reset_orchestrate_manip", "imx_plan_reward_weight_ptr", "imx_plan_reward_weight_get")}
    text = unit(structs, sigs, {"imx_event_op": _abi.ENUMS["imx_event_op"]}, {"IMX_ORCH_MAX_WEIGHT_TERMS": _lib.ORCH_MAX_WEIGHT_TERMS})
    assert text.count("offset, size") == len(_lib.ImxWeightTerm._fields_) + len(_lib.ImxOrchManip._fields_) == 5 + 6
    src = tmp_path / "manip_abi.cpp"

    def compiles(t):
        src.write_text(t)
        r = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
        return "" if r.returncode == 0 else (r.stderr or f"exit status {r.returncode}")

    assert compiles(text) == ""
    fields = list(_lib.ImxWeightTerm._fields_)
    fields[3], fields[4] = fields[4], fields[3]  # weight <-> num_steps: the same size, only the kinds and offsets can tell
    err = compiles(unit({"imx_weight_term_t": type("ImxWeightTerm", (ctypes.Structure,), {"_fields_": fields})}, {}, {}, {}))
    assert "static" in err and "imx_weight_term_t" in err, err


# ------------------------------------------------------------------------------------------------ refusals (no GPU needed)
def _lift():
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import FRANKA_PANDA, SceneEntityResolver

    fx = mo.ManipOrchGolden("lift").fixture
    return fx, FRANKA_PANDA, SceneEntityResolver(FRANKA_PANDA, fx["env"]["scene"]), compile_plan(copy.deepcopy(fx["env"]), FRANKA_PANDA)


def test_event_terms_resolve_their_asset():
    from isaaclab_amd.events import EventManager, EventTermState

    fx, robot, ent, _ = _lift()
    ev, scene = fx["env"]["events"], fx["env"]["scene"]
    em = EventManager(ev, 8, robot, "cpu", entities=ent, scene=scene)
    assert [(t.name, t.func, t.asset) for t in em.terms] == [("reset_all", "reset_scene_to_default", 0), ("reset_object_position", "reset_root_state_uniform", 1)]
    assert em.needs_manip and em.active_terms == {"reset": ["reset_all", "reset_object_position"]}
    assert EventTermState("t", dict(ev["reset_object_position"], params={"pose_range": {}, "velocity_range": {}}), 8, robot, "cpu", ent).asset == 0
    robot_term = copy.deepcopy(ev["reset_object_position"])
    robot_term["params"]["asset_cfg"]["name"] = "robot"
    assert EventTermState("t", robot_term, 8, robot, "cpu", ent).asset == 0
    bad = copy.deepcopy(ev["reset_object_position"])
    bad["params"]["asset_cfg"]["name"] = "cube"
    with pytest.raises(ValueError, match=r"event term 'place'.*'cube'.*\['robot', 'object'\]"):
        EventTermState("place", bad, 8, robot, "cpu", ent)
    with pytest.raises(ValueError, match=r"event term 'place'.*'object'.*\['robot'\]"):  # a scene without the object
        EventTermState("place", ev["reset_object_position"], 8, robot, "cpu")
    with pytest.raises(NotImplementedError, match="reset_scene_to_default' as an interval event"):
        EventTermState("t", dict(ev["reset_all"], mode="interval", interval_range_s=(1.0, 2.0)), 8, robot, "cpu", ent)
    push = {"func": "isaaclab.envs.mdp.events:push_by_setting_velocity", "mode": "reset", "params": {"velocity_range": {}, "asset_cfg": {"name": "object"}}}
    with pytest.raises(NotImplementedError, match="'push'.*push_by_setting_velocity.*rigid object 'object'"):
        EventTermState("push", push, 8, robot, "cpu", ent)
    two = dict(scene, object2=scene["object"])
    from isaaclab_amd.robots import SceneEntityResolver
    with pytest.raises(NotImplementedError, match="'reset_all'.*2 rigid objects"):
        EventManager(ev, 8, robot, "cpu", entities=SceneEntityResolver(robot, two), scene=two)
    soft = dict(scene, cloth={"class_type": "isaaclab.assets.deformable_object.deformable_object:DeformableObject"})
    with pytest.raises(NotImplementedError, match=r"'reset_all'.*deformable objects \['cloth'\]"):
        EventManager(ev, 8, robot, "cpu", entities=ent, scene=soft)
    assert not EventManager(mo.ManipOrchGolden("reach").fixture["env"]["events"], 8, robot, "cpu").needs_manip


def test_curriculum_manager_refusals():
    from isaaclab_amd.events import CurriculumManager

    fx, _, _, plan = _lift()
    env = types.SimpleNamespace(plan=plan, terrain_importer=None)
    cur = fx["env"]["curriculum"]
    with pytest.raises(NotImplementedError, match="modify_reward_weight.*reward_curriculum=True"):  # without the keyword: as before, plus the hint
        CurriculumManager(cur, env)
    cm = CurriculumManager(cur, env, reward_curriculum=True)
    assert cm.active_terms == ["action_rate", "joint_vel"] and cm.terrain_terms == [] and cm.reset() == {}
    names = [t.name for t in plan.reward_terms]
    assert [(w["name"], w["term_name"], w["index"], w["weight"], w["num_steps"]) for w in cm.weight_terms] == [
        ("action_rate", "action_rate", names.index("action_rate"), -0.1, 12), ("joint_vel", "joint_vel", names.index("joint_vel"), -0.1, 25)]
    one = lambda **p: {"c": {"func": "isaaclab.envs.mdp.curriculums:modify_reward_weight", "params": p}}  # noqa: E731
    with pytest.raises(ValueError, match=r"^Reward term 'nope' not found\.$"):
        CurriculumManager(one(term_name="nope", weight=1.0, num_steps=3), env, reward_curriculum=True)
    for missing in ("term_name", "weight", "num_steps"):
        p = dict(term_name="joint_vel", weight=1.0, num_steps=3)
        p.pop(missing)
        with pytest.raises(ValueError, match=rf"curriculum term 'c'.*lacks \['{missing}'\]"):
            CurriculumManager(one(**p), env, reward_curriculum=True)
    many = {f"c{i}": one(term_name="joint_vel", weight=float(i), num_steps=i)["c"] for i in range(_lib.ORCH_MAX_WEIGHT_TERMS + 1)}
    with pytest.raises(NotImplementedError, match=rf"'c{_lib.ORCH_MAX_WEIGHT_TERMS}'.*more than {_lib.ORCH_MAX_WEIGHT_TERMS}"):
        CurriculumManager(many, env, reward_curriculum=True)
    # a target evaluated in Python reads its weight on the host
    ext = copy.deepcopy(plan)
    ext.reward_terms[names.index("joint_vel")].external = "some.module:function"
    with pytest.raises(NotImplementedError, match="'joint_vel'.*'joint_vel' is evaluated in Python"):
        CurriculumManager(cur, types.SimpleNamespace(plan=ext, terrain_importer=None), reward_curriculum=True)
    with pytest.raises(NotImplementedError, match="'x'.*'other_thing' has no kernel"):
        CurriculumManager({"x": {"func": "m:other_thing", "params": {}}}, env, reward_curriculum=True)
