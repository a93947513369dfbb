"""CPU: ``OperationalSpaceControllerAction`` on the fused path -- the torch restatement and the host build of the kernel's per-env
function against the fixtures of the REAL class (tools/gen_golden_osc.py), the term compiler on the Isaac-Reach-Franka-OSC-v0 fixture,
its errors and refusals, the state feed's dynamics tensors, and the C interface.  Tolerances: tests/_osc_cases.py."""

import copy
import ctypes
import hashlib
import os
import re

import pytest
import torch

import _osc_cases as oc
from isaaclab_amd import _lib
from isaaclab_amd.env import load_task_cfg
from isaaclab_amd.plan import A_JOINT_AFFINE, F_ACT_CLIP, compile_plan, resolve_osc_term
from isaaclab_amd.robots import FRANKA_PANDA, ROBOTS
from isaaclab_amd.state_feed import DYNAMICS, StateFeed

ROOT = oc.ROOT
OSC_CLASS = "isaaclab.envs.mdp.actions.task_space_actions:OperationalSpaceControllerAction"


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_restatement_matches_reference(variant):
    worst = oc.run_oracle(oc.OscGolden(variant))
    print(f"{variant}: largest rho {worst:.3g}, rho_ref {oc.META[variant]['rho_ref']:.3g}")


def test_fixture_covers_what_the_issue_asks():
    m = oc.META
    ctrl = {v: m[v]["cfg"]["controller_cfg"] for v in oc.VARIANTS}
    assert [ctrl[v]["target_types"] for v in oc.VARIANTS] == [["pose_abs"], ["pose_rel"], ["pose_abs"], ["pose_rel", "wrench_abs"], ["pose_abs"]]
    assert [ctrl[v]["impedance_mode"] for v in oc.VARIANTS] == ["variable_kp", "fixed", "variable", "fixed", "variable_kp"]
    assert [(ctrl[v]["inertial_dynamics_decoupling"], ctrl[v]["partial_inertial_dynamics_decoupling"]) for v in oc.VARIANTS] == \
        [(True, False), (True, False), (True, True), (False, False), (True, False)]
    assert [ctrl[v]["gravity_compensation"] for v in oc.VARIANTS] == [False, True, True, False, False]
    assert [ctrl[v]["nullspace_control"] for v in oc.VARIANTS] == ["position", "none", "none", "none", "none"]
    assert m["O1"]["cfg"]["nullspace_joint_pos_target"] == "center"
    assert [m[v]["action_dim"] for v in oc.VARIANTS] == [13, 6, 19, 12, 13]
    assert list(ctrl["O2"]["motion_control_axes_task"]) == [1, 1, 0, 1, 1, 1] == list(ctrl["O4"]["motion_control_axes_task"])
    assert list(ctrl["O4"]["contact_wrench_control_axes_task"]) == [0, 0, 1, 0, 0, 0] and m["O4"]["cfg"]["wrench_scale"] != 1.0
    assert ctrl["O4"]["contact_wrench_stiffness_task"] is None
    assert m["O2"]["cfg"]["body_offset"]["rot"][0] != 1.0 and isinstance(ctrl["O3"]["motion_stiffness_task"], list)
    assert {len(m[v]["joint_ids"]) for v in oc.VARIANTS} == {6, 7} and {m[v]["ND"] for v in oc.VARIANTS} == {9, 12}
    assert m["O5"]["jacobi_body_idx"] == m["O5"]["body_idx"] and m["O5"]["jacobi_joint_ids"] == [i + 6 for i in m["O5"]["joint_ids"]]
    assert m["O5"]["NM"] == 6 and m["O5"]["joint_ids"] == list(range(6))  # the mass matrix is indexed by joint_ids, not + 6
    assert m["O1"]["jacobi_body_idx"] == m["O1"]["body_idx"] - 1
    for v in ("O1", "O2", "O3", "O5"):  # the near-singular block: kappa = cond(M) cond(J M^-1 J^T) several decades above the easy block's
        assert m[v]["kappa_median_near_singular"] > 1.0e6 > 1.0e4 > m[v]["kappa_median_easy"] > 10.0, v
        assert 2.0 < m[v]["cond_M_median"] < 100.0, v
    assert m["O4"]["kappa_max"] == 1.0
    for v in oc.VARIANTS:
        assert (m[v]["N"], m[v]["steps"], m[v]["substeps"], m[v]["n_easy"]) == (256, 6, 2, 192)
        for suffix in ("", "_in", "_dyn"):
            assert os.path.getsize(os.path.join(oc.GOLDEN, f"osc_{v}{suffix}.npz")) <= 1 << 20


# ------------------------------------------------------------------------------------------------ the term compiler
def test_osc_task_fixture_compiles():
    fx = load_task_cfg(oc.task_path())
    rec = fx["managers"]  # what the generator recorded from the REAL managers
    p = compile_plan(fx["env"], ROBOTS[fx["robot"]])
    assert p.action_dim == rec["action_dim"] == 13 and p.processed_action_dim == rec["processed_action_dim"] == 13
    assert [t.name for t in p.action_terms] == rec["action_terms"] == ["arm_action"] and [t.dim for t in p.action_terms] == rec["action_term_dims"]
    assert p.obs_dim == rec["policy_obs_dim"]
    assert [t.name for t in p.obs_terms] == rec["policy_obs_terms"] and "joint_pos" not in rec["policy_obs_terms"] and "joint_vel" not in rec["policy_obs_terms"]
    assert [list(d) for d in p.obs_term_dims] == rec["policy_obs_term_dims"]
    assert p.ik_terms == [] and len(p.osc_terms) == 1
    o, r = p.osc_terms[0], rec["osc_term"]
    assert (o.name, o.body_name, o.body_idx, o.jacobi_body_idx) == (r["name"], r["body_name"], r["body_idx"], r["jacobi_body_idx"])
    assert o.body_name == "panda_hand" and o.jacobi_body_idx == o.body_idx - 1
    assert o.joint_ids == r["joint_ids"] == list(range(7)) and o.jacobi_joint_ids == r["jacobi_joint_ids"]
    assert o.width == r["action_dim"] == 13 and o.target_types == r["target_types"] == ["pose_abs"] and o.pose_type == "pose_abs"
    assert (o.pose_idx, o.wrench_idx, o.stiffness_idx, o.damping_ratio_idx) == (r["pose_abs_idx"], r["wrench_abs_idx"], r["stiffness_idx"], r["damping_ratio_idx"]) == (0, None, 7, None)
    assert r["pose_rel_idx"] is None
    assert o.impedance_mode == r["impedance_mode"] == "variable_kp" and o.decoupling == "full" and not o.gravity_compensation
    assert r["inertial_dynamics_decoupling"] and not r["partial_inertial_dynamics_decoupling"] and not r["gravity_compensation"]
    assert (o.nullspace_control, o.nullspace_joint_pos_target) == (r["nullspace_control"], r["nullspace_joint_pos_target"]) == ("position", "center")
    c = _lib.ImxOsc.from_term(o)
    assert c.nullspace_kp == r["nullspace_p_gain"] and c.nullspace_kd == r["nullspace_d_gain"]  # (fp32 tensors of the real controller)
    assert o.offset_pos is None and o.motion_stiffness_limits == tuple(r["motion_stiffness_limits_task"]) == (50.0, 200.0)
    assert o.scale == [1.0] * 7 + [r["stiffness_scale"]] * 6 and r["stiffness_scale"] == 100.0
    inf = float("inf")
    assert o.clip == [(-inf, inf)] * 7 + [(50.0, 200.0)] * 6
    assert rec["arm_actuators"] == {"panda_shoulder": {"stiffness": 0.0, "damping": 0.0}, "panda_forearm": {"stiffness": 0.0, "damping": 0.0}}
    assert fx["agent"]["experiment_name"] == "franka_reach"
    # the blob: one A_JOINT_AFFINE record with a scale table and a clip table
    from isaaclab_amd.plan import H as HEADER, R as REC_FIELDS, REC_WORDS

    w = p.blob
    rec0 = w[int(w[HEADER["ACT_OFF"]]): int(w[HEADER["ACT_OFF"]]) + REC_WORDS]
    assert int(rec0[REC_FIELDS["OP"]]) == A_JOINT_AFFINE and int(rec0[REC_FIELDS["FLAGS"]]) == F_ACT_CLIP and int(rec0[REC_FIELDS["DIM"]]) == 13


def test_variant_cfgs_resolve_as_the_real_term_did():
    for v in oc.VARIANTS:
        o, m = oc.OscGolden(v, 1).osc, oc.META[v]
        assert (o.body_idx, o.jacobi_body_idx, o.joint_ids, o.jacobi_joint_ids, o.width) == \
            (m["body_idx"], m["jacobi_body_idx"], m["joint_ids"], m["jacobi_joint_ids"], m["action_dim"]), v
        pose = m["pose_abs_idx"] if m["pose_abs_idx"] is not None else m["pose_rel_idx"]
        assert (o.pose_idx, o.wrench_idx, o.stiffness_idx, o.damping_ratio_idx) == (pose, m["wrench_abs_idx"], m["stiffness_idx"], m["damping_ratio_idx"]), v
    g = oc.OscGolden("O1", 4)
    assert torch.allclose(g.target[0], torch.tensor(oc.META["O1"]["nullspace_target_row0"]))
    o4 = oc.OscGolden("O4", 1).osc
    assert o4.scale == [0.5] * 6 + [2.5] * 6 and o4.decoupling == "none" and o4.wrench_idx == 6
    o3 = oc.OscGolden("O3", 1).osc
    assert o3.clip[7:13] == [(10.0, 300.0)] * 6 and o3.clip[13:19] == [(0.1, 2.0)] * 6 and o3.scale[13:] == [1.5] * 6 and o3.decoupling == "partial"


# sha256 of the blob words (little-endian int32) the commit before this term compiled these fixtures to
PARENT_BLOBS = {
    "Isaac-Reach-Franka-v0": "3c7746b4b2cdbca6b8857cd4c8b5580f96c92681dc62ed7978ba5ab520b9072d",
    "Isaac-Reach-UR10-v0": "651dc1fc562d5dc604489a1626ed78728b0010f4233da806cdbeabbece41c4ec",
    "golden/Isaac-Lift-Cube-Franka-v0.json": "0493d97a2fccc4cdc4d9372bece973eaee7c59141b8c5ef1798a39aaa74c6876",
    "golden/Isaac-Reach-Franka-IK-Abs-v0.json": "dec881e4548296658524c4215f036dbd3dcbcc6f5555dc886edf2cf5181367a8",
    "golden/Isaac-Reach-Franka-IK-Rel-v0.json": "1f8aece61aee726e7b721f1b2227d80468cac327a67c4b416400f00f3548dac9",
    "golden/Isaac-Lift-Cube-Franka-IK-Abs-v0.json": "0dfd7743daf5a430bf410996feb28b895d68c3b0fddff103000fa35d5469beb4",
    "golden/Isaac-Lift-Cube-Franka-IK-Rel-v0.json": "2edfa4cea341ce704a4e04080f5b252c733726c26b971ade0234adc9af5a4e9c",
    # (the term's own task, as compiled before diff-IK and OSC came to share their resolver code)
    "golden/Isaac-Reach-Franka-OSC-v0.json": "e6838b6a3c1f8134ce3ca6cf3ccf16e907c75a6c01c5d072bd8fb40dc952a901",
}
# sha256 of bytes(ImxOsc.from_term(...)) of the variants' cfgs, from the same commit (little-endian ints and floats: platform-independent)
OSC_STRUCTS = {
    "O1": "090c39dd5493aa88dd3226e02aa5ea6079f3f5745d92d487340cc1ba2b310bac",
    "O2": "2f39d0f41d57aaf4e0354fa101343d3e9f208a9910ced962087698aae90db9d4",
    "O3": "d122e7b3c0be0d981d7e11976d83d7e86124d822f5166786a4f6441bf65ebfae",
    "O4": "920d3790d7d2a44b11bacdc250a04799364106b86af972f043b0049b905770f7",
    "O5": "119201c85db5506b5f25795a2ee1d6bfc0db498e1df9cf9e4b06c9aeed0bb9b9",
}


@pytest.mark.parametrize("task", list(PARENT_BLOBS))
def test_existing_fixtures_compile_to_the_same_blob(task):
    fx = load_task_cfg(os.path.join(oc.HERE, task) if task.startswith("golden/") else task)
    p = compile_plan(fx["env"], ROBOTS[fx["robot"]])
    assert hashlib.sha256(p.blob.astype("<i4").tobytes()).hexdigest() == PARENT_BLOBS[task]
    assert len(p.osc_terms) == (1 if "-OSC-" in task else 0) and len(p.ik_terms) == (1 if "-IK-" in task else 0)


@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_variant_cfgs_fill_the_same_struct(variant):
    assert hashlib.sha256(bytes(_lib.ImxOsc.from_term(oc.OscGolden(variant, 1).osc))).hexdigest() == OSC_STRUCTS[variant]


# ------------------------------------------------------------------------------------------------ errors and refusals
def _osc_env():
    return copy.deepcopy(load_task_cfg(oc.task_path())["env"])


def _arm(env):
    return env["actions"]["arm_action"]


def _raises(exc, match, edit):
    env = _osc_env()
    edit(env)
    with pytest.raises(exc, match=match):
        compile_plan(env, FRANKA_PANDA)


def test_reference_value_errors():
    _raises(ValueError, r"Invalid control command: pose_delta\.", lambda e: _arm(e)["controller_cfg"].update(target_types=["pose_delta"]))
    _raises(ValueError, r"Invalid impedance mode: soft\.", lambda e: _arm(e)["controller_cfg"].update(impedance_mode="soft"))
    _raises(ValueError, r"Nullspace joint targets can only be set when null space control is set to 'position'\.",
            lambda e: _arm(e)["controller_cfg"].update(nullspace_control="none"))
    _raises(ValueError, r"Nullspace joint targets must be set when null space control is set to 'position'\.",
            lambda e: _arm(e).update(nullspace_joint_pos_target="none"))
    _raises(ValueError, r"Invalid value for nullspace joint pos targets\.", lambda e: _arm(e).update(nullspace_joint_pos_target="middle"))
    _raises(ValueError, r"Null-space control is only applicable for redundant manipulators\.", lambda e: _arm(e).update(joint_names=["panda_joint[1-6]"]))
    _raises(ValueError, r"Expected one match for the ee body name: panda_\.\*finger\. Found 2: \['panda_leftfinger', 'panda_rightfinger'\]\.",
            lambda e: _arm(e).update(body_name="panda_.*finger"))


def test_refusals_name_the_term_and_the_reason():
    ni = NotImplementedError
    _raises(ni, r"arm_action.*task_frame_rel_path 'task_frame'.*FrameTransformer", lambda e: _arm(e).update(task_frame_rel_path="task_frame"))
    _raises(ni, r"arm_action.*closed-loop wrench control.*contact sensor",
            lambda e: _arm(e)["controller_cfg"].update(target_types=["pose_abs", "wrench_abs"], contact_wrench_stiffness_task=0.1))
    _raises(ni, r"arm_action.*nullspace_control 'position' without full inertial decoupling.*SVD",
            lambda e: _arm(e)["controller_cfg"].update(partial_inertial_dynamics_decoupling=True))
    _raises(ni, r"arm_action.*nullspace_control 'position' without full inertial decoupling.*SVD",
            lambda e: _arm(e)["controller_cfg"].update(inertial_dynamics_decoupling=False))
    _raises(ni, r"arm_action.*9 controlled joints.*at most 8", lambda e: _arm(e).update(joint_names=["panda_.*"]))
    _raises(ni, r"second_arm.*second OperationalSpaceControllerAction.*arm_action",
            lambda e: e["actions"].update(second_arm=copy.deepcopy(_arm(e))))
    _raises(ni, r"arm_action.*two motion targets or two wrench targets", lambda e: _arm(e)["controller_cfg"].update(target_types=["pose_abs", "pose_rel"]))
    _raises(ni, r"arm_action.*two motion targets or two wrench targets",
            lambda e: _arm(e)["controller_cfg"].update(target_types=["pose_abs", "wrench_abs", "wrench_abs"]))
    _raises(ni, r"arm_action.*an OperationalSpaceControllerAction cfg without \['controller_cfg'\] is not on the fused path",
            lambda e: _arm(e).pop("controller_cfg"))
    ik = load_task_cfg(os.path.join(oc.GOLDEN, "Isaac-Reach-Franka-IK-Rel-v0.json"))["env"]["actions"]["arm_action"]
    _raises(ni, r"ik_arm.*DifferentialInverseKinematicsAction beside the OperationalSpaceControllerAction 'arm_action'",
            lambda e: e["actions"].update(ik_arm=copy.deepcopy(ik)))

    def ik_first(e):
        e["actions"] = {"ik_arm": copy.deepcopy(ik), "arm_action": _arm(e)}

    _raises(ni, r"arm_action.*OperationalSpaceControllerAction beside the DifferentialInverseKinematicsAction 'ik_arm'", ik_first)


def test_wrench_and_impedance_variants_are_supported():
    """Everything the issue lists as supported resolves: both pose types with and without the open-loop wrench, the three impedance
    modes, the three decouplings, gravity compensation, no null space, an offset, one to eight joints."""
    base = _arm(_osc_env())
    for targets, width in ((["pose_abs"], 7), (["pose_rel"], 6), (["pose_abs", "wrench_abs"], 13), (["wrench_abs", "pose_rel"], 12)):
        for mode, extra in (("fixed", 0), ("variable_kp", 6), ("variable", 12)):
            for dec, part in ((False, False), (True, False), (True, True)):
                t = copy.deepcopy(base)
                t["controller_cfg"].update(target_types=targets, impedance_mode=mode, inertial_dynamics_decoupling=dec,
                                           partial_inertial_dynamics_decoupling=part, gravity_compensation=True, nullspace_control="none")
                t.update(nullspace_joint_pos_target="none", body_offset={"pos": (0.0, 0.0, 0.1), "rot": (1.0, 0.0, 0.0, 0.0)})
                o = resolve_osc_term("arm_action", t, FRANKA_PANDA)
                assert o.width == width + extra and len(o.scale) == len(o.clip) == o.width
                c = _lib.ImxOsc.from_term(o)
                assert c.has_wrench == ("wrench_abs" in targets) and c.has_offset == 1
    t = copy.deepcopy(base)
    t["controller_cfg"].update(nullspace_control="none")
    t.update(nullspace_joint_pos_target="none", joint_names=["panda_joint1"])
    assert resolve_osc_term("arm_action", t, FRANKA_PANDA).joint_ids == [0]
    o = resolve_osc_term("arm_action", copy.deepcopy(base), FRANKA_PANDA)  # wrench_abs before the pose: the columns follow cfg order
    w = copy.deepcopy(base)
    w["controller_cfg"].update(target_types=["wrench_abs", "pose_abs"])
    ow = resolve_osc_term("arm_action", w, FRANKA_PANDA)
    assert (o.pose_idx, ow.wrench_idx, ow.pose_idx, ow.stiffness_idx) == (0, 0, 6, 13)


# ------------------------------------------------------------------------------------------------ the state feed
def test_ensure_dynamics_changes_no_other_tensor():
    a, b = StateFeed(FRANKA_PANDA, 16, seed=7, num_snapshots=2), StateFeed(FRANKA_PANDA, 16, seed=7, num_snapshots=2)
    b.ensure_jacobians()
    before = {n: b._stack[n].clone() for n in b._stack}
    assert not any(n in a._stack for n in DYNAMICS)
    b.ensure_dynamics()
    assert set(b._stack) == set(before) | set(DYNAMICS)
    for n, t in before.items():
        assert torch.equal(b._stack[n], t), n
    for n in a._stack:
        assert torch.equal(a._stack[n], b._stack[n]), n
    J, B = FRANKA_PANDA.num_joints, FRANKA_PANDA.num_bodies
    M = b._stack["mass_matrices"]
    assert M.shape == (2, 16, J, J) and b["gravity_compensation_forces"].shape == (16, J) and b["body_ang_vel_w"].shape == (16, B, 3)
    assert torch.equal(M, M.transpose(-1, -2)) and (torch.linalg.eigvalsh(M.double()) > 0.04).all()
    assert (torch.linalg.cond(M.double()) < 1.0e3).all()
    again = StateFeed(FRANKA_PANDA, 16, seed=7, num_snapshots=2)
    again.ensure_dynamics()  # (without the Jacobians first: its own generator)
    for n in DYNAMICS:
        assert torch.equal(again._stack[n], b._stack[n]), n
    rec = StateFeed.from_tensors(FRANKA_PANDA, [a.snapshot(0)])
    with pytest.raises(KeyError, match="mass_matrices"):
        rec.ensure_dynamics()
    StateFeed.from_tensors(FRANKA_PANDA, [b.snapshot(0)]).ensure_dynamics()


# ------------------------------------------------------------------------------------------------ the C interface
def _header():
    with open(os.path.join(ROOT, "include", "imx.h")) as f:
        return f.read()


def test_entry_point_is_declared_with_its_citations():
    h = _header()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int imx_osc\(([^;]*)\);", h, re.S)
    assert m, "imx_osc is not declared in include/imx.h"
    comment, args = " ".join(m.group(1).replace("\n * ", " ").split()), m.group(2)
    for cite in ("task_space_actions.py:416-438", ":440-462", ":464-474", "operational_space.py:173-343", ":345-548", ":664-700", ":597-615", ":403-410",
                 ":576-595", ":617-634", ":568-574", ":645-649"):
        assert cite in comment, cite
    s = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define IMX_OSC_CMD_WIDTH", h, re.S)
    struct_comment = " ".join(s.group(1).replace("\n * ", " ").split())
    for cite in ("task_space_actions.py:248-378", ":504-537", ":539-566", "operational_space.py:34-140", ":146-160", "operational_space_cfg.py"):
        assert cite in struct_comment, cite
    nargs = len([a for a in args.split(",") if a.strip()])
    res, argtypes = _lib._SIGNATURES["imx_osc"]
    assert nargs == len(argtypes) == 29 and res is ctypes.c_int
    assert "imx_osc" in _lib.EXPORTS and "typedef struct imx_osc imx_osc_t;" in h and '#include "imx_osc_struct.h"' in h
    with open(os.path.join(ROOT, "include", "imx_osc_struct.h")) as f:
        assert "typedef struct imx_osc {" in f.read()


def test_structs_keep_their_size_and_imx_osc_t_is_bound():
    assert ctypes.sizeof(_lib.ImxState) == 248 and ctypes.sizeof(_lib.ImxBuffers) == 216 and ctypes.sizeof(_lib.ImxOrch) == 1944
    assert ctypes.sizeof(_lib.ImxDiffIk) == 4 * (4 + 2 + 3 + 4 + 3 + 8 + 8 + 1)
    assert ctypes.sizeof(_lib.ImxOsc) == 4 * (11 + 24 + 2 + 2 + 2 + 3 + 4 + 3 + 8 + 8)
    L = _lib.lib()
    assert int(L.imx_struct_size(8)) == ctypes.sizeof(_lib.ImxOsc) and int(L.imx_struct_size(7)) == ctypes.sizeof(_lib.ImxDiffIk)
    assert int(L.imx_struct_size(9)) == 0


def test_the_compiler_agrees_with_the_binding_of_imx_osc_t(tmp_path):
    """imx_osc_t is defined in include/imx_osc_struct.h (imx.h includes it) and bound from there by the same parser: a C++ compiler that reads
    imx.h must see the size, every field's offset, size and kind, and the entry point's signature as the binding has them."""
    import subprocess

    from test_abi import unit

    if oc.host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    from isaaclab_amd import _abi

    assert list(_abi.OSC_STRUCTS) == ["imx_osc_t"] and "imx_osc_t" not in _abi.STRUCTS
    assert [f for f, _ in _lib.ImxOsc._fields_] == [f for f, _ in _abi.OSC_STRUCTS["imx_osc_t"]]
    text = unit({"imx_osc_t": _lib.ImxOsc}, {"imx_osc": _lib._SIGNATURES["imx_osc"]}, {}, {})
    assert text.count("offset, size") == len(_lib.ImxOsc._fields_) == 26
    src = tmp_path / "osc_abi.cpp"

    def compiles(t):
        src.write_text(t)
        r = subprocess.run([oc.host_compiler(), "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
        return "" if r.returncode == 0 else (r.stderr or f"exit status {r.returncode}")

    assert compiles(text) == ""
    fields = list(_lib.ImxOsc._fields_)
    i = [n for n, _ in fields].index("nullspace_kp")
    fields[i], fields[i + 1] = fields[i + 1], fields[i]  # the same size, two floats swapped: only the offsets can tell
    err = compiles(unit({"imx_osc_t": type("ImxOsc", (ctypes.Structure,), {"_fields_": fields})}, {}, {}, {}))
    assert "static" in err and "imx_osc_t.nullspace_kp offset, size" in err, err


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if oc.host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine: tools/osc_host.cpp cannot be built")
    return oc.build_host_program(str(tmp_path_factory.mktemp("osc_host")))


@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_host_program_matches_reference(host_program, variant, tmp_path):
    """tools/osc_host.cpp runs the kernel's own per-env function (csrc/imx_osc.h) as plain host C++."""
    worst = oc.run_host_program(host_program, oc.OscGolden(variant), str(tmp_path))
    print(f"{variant}: largest rho {worst:.3g}, bound {oc.FACTOR * oc.META[variant]['rho_ref']:.3g}")


def test_host_program_reads_only_its_rows_and_columns(host_program, tmp_path):
    """NaN in every unselected body, Jacobian row / column, joint and mass-matrix row / column (and the strict upper triangle of the
    mass matrix): the outputs do not change by a bit."""
    import numpy as np

    class Filled(oc.OscGolden):
        def state(self, t, s, fill=0.0):
            return super().state(t, s, float("nan"))

    for v in ("O1", "O2", "O5"):
        a, b = oc.OscGolden(v, 8), Filled(v, 8)
        da, db = tmp_path / f"{v}a", tmp_path / f"{v}b"
        da.mkdir(), db.mkdir()
        for x, y in zip(oc.host_outputs(host_program, a, str(da)), oc.host_outputs(host_program, b, str(db))):
            assert np.isfinite(y[4]).all() and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4]), (v, x[:3])


@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_host_program_mode3_equals_mode1_then_mode2(host_program, variant, tmp_path):
    import numpy as np

    g = oc.OscGolden(variant, 9)
    split = oc.host_outputs(host_program, g, str(tmp_path))
    merged = oc.host_outputs(host_program, g, str(tmp_path), merged_first=True)
    for t in range(g.steps):  # split: (1, 2, 2) per step; merged: (3, 2) per step
        for a, b in ((split[3 * t + 1], merged[2 * t]), (split[3 * t + 2], merged[2 * t + 1])):
            assert a[:2] == b[:2] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), (variant, t)


def test_argument_checks_run_before_any_launch():
    """The host-side checks of ``imx_osc`` need no GPU: every bad argument comes back as an error string (the pointers are never
    dereferenced on the host; the GPU file repeats this with real tensors and checks that nothing was written)."""
    L = _lib.lib()
    cfg = _lib.ImxOsc.from_term(oc.OscGolden("O1", 8).osc)
    fake = 0x1000

    def call(cfg=cfg, N=8, mode=3, PA=13, B=11, NB=10, ND=9, NM=9, J=9, ld_cmd=25, ld_eff=7, p=fake, out=fake, mass=fake, target=fake, cmd=fake):
        return L.imx_osc(ctypes.byref(cfg), N, mode, p, PA, fake, fake, fake, fake, fake, fake, fake, fake, B, fake, NB, ND, mass, fake, NM,
                         fake, fake, J, target, cmd, ld_cmd, out, ld_eff, None)

    for kw, why in ((dict(mode=0), "mode must be 1, 2 or 3"), (dict(mode=4), "mode"), (dict(N=0), "num_envs"), (dict(PA=12), "processed columns"),
                    (dict(B=8), "body_idx"), (dict(NB=7), "jacobi_body_idx"), (dict(ND=6), "Jacobian column"), (dict(J=6), "joint id"),
                    (dict(NM=6), "mass-matrix row"), (dict(ld_cmd=24), "ld_cmd"), (dict(ld_eff=6), "ld_eff"), (dict(p=None), "null processed action"),
                    (dict(out=None), "null argument"), (dict(cmd=None), "null argument"), (dict(mass=None), "null mass matrices"),
                    (dict(target=None), "null joint state or null-space target")):
        assert call(**kw) != 0, kw
        msg = L.imx_last_error().decode()
        assert msg.startswith("imx_osc: ") and why in msg, (kw, msg)
    for field, value, why in (("num_joints", 9, "num_joints outside [1, 8]"), ("num_joints", 6, "six joints or fewer"), ("decoupling", 2, "without full decoupling"),
                              ("decoupling", 3, "unknown decoupling"), ("pose_type", 2, "unknown pose type"), ("impedance_mode", 3, "unknown impedance mode"),
                              ("stiffness_col", 8, "processed columns")):
        bad = _lib.ImxOsc.from_buffer_copy(bytes(cfg))
        setattr(bad, field, value)
        assert call(cfg=bad) != 0 and why in L.imx_last_error().decode(), (field, L.imx_last_error().decode())
