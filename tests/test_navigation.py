"""CPU: Isaac-Navigation-Flat-Anymal-C-v0 and its ``PreTrainedPolicyAction`` -- the fixture compiles, what is not built is refused with its
reason, the policy loader takes and refuses what it should, the torch restatement (tests/_navigation_oracle.py) reproduces the
recordings P1-P3 of the REAL class, the new struct's binding is what a C++ compiler reads, and ``imx_pretrained_policy`` refuses bad
arguments before any launch."""

import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _navigation_cases as nc
from _util import FLOAT_TOL, assert_close
from isaaclab_amd import _abi, _lib
from isaaclab_amd.plan import A_JOINT_AFFINE, W_OPS, O_OPS, R, REC_WORDS, H, command_width, compile_plan
from isaaclab_amd.policy_loader import PolicyError, load_policy, resolve_policy_path
from isaaclab_amd.robots import ANYMAL_C_NAV, ROBOTS
from isaaclab_amd.state_feed import StateFeed

_POSE_2D = "isaaclab.envs.mdp.commands.pose_2d_command:"


def _plan(fx=None):
    fx = fx or nc.fixture()
    return fx, compile_plan(fx["env"], ROBOTS[fx["robot"]])


def _records(plan, table: str, n: int):
    off = int(plan.blob[H[table]])
    return [plan.blob[off + k * REC_WORDS: off + (k + 1) * REC_WORDS] for k in range(n)]


# ------------------------------------------------------------------------------------------------ the term compiler
def test_navigation_fixture_compiles():
    fx, p = _plan()
    m = fx["managers"]  # what the REAL managers reported over the fake scene
    assert fx["robot"] == "anymal_c_nav" and p.cmd_dim == 4 and int(p.blob[H["CMD_DIM"]]) == 4
    assert p.obs_dim == m["policy_obs_dim"] == 10 and p.action_dim == m["action_dim"] == 3 and p.processed_action_dim == 3
    assert [t.name for t in p.obs_terms] == m["policy_obs_terms"] == ["base_lin_vel", "projected_gravity", "pose_command"]
    assert [t.dim for t in p.obs_terms] == [3, 3, 4]
    assert [t.name for t in p.action_terms] == m["action_terms"] == [nc.TERM] and [t.dim for t in p.action_terms] == m["action_term_dims"] == [3]
    assert [t.name for t in p.reward_terms] == m["reward_terms"] and [t.name for t in p.termination_terms] == m["termination_terms"]
    # the two new reward ops, with their std in P0 and the cfg's weights
    recs = _records(p, "REW_OFF", 4)
    assert [int(r[R["OP"]]) for r in recs] == [W_OPS["IS_TERMINATED"], W_OPS["NAV_POSITION_COMMAND_ERROR_TANH"],
                                                W_OPS["NAV_POSITION_COMMAND_ERROR_TANH"], W_OPS["NAV_HEADING_COMMAND_ERROR_ABS"]]
    f = lambda w: float(np.asarray([w], np.int32).view(np.float32)[0])  # noqa: E731
    assert [f(r[R["WEIGHT"]]) for r in recs] == [-400.0, 0.5, 0.5, np.float32(-0.2)]
    assert f(recs[1][R["P0"]]) == 2.0 and f(recs[2][R["P0"]]) == np.float32(0.2)
    # raw -> processed is the affine record with scale 1 and no flag
    (a,) = _records(p, "ACT_OFF", 1)
    assert int(a[R["OP"]]) == A_JOINT_AFFINE and int(a[R["DIM"]]) == 3 and f(a[R["P0"]]) == 1.0 and f(a[R["P1"]]) == 0.0 and int(a[R["FLAGS"]]) == 0
    # the low-level plan
    (pt,) = p.policy_terms
    ll = pt.low_level_plan
    assert pt.low_level_decimation == m["low_level"]["low_level_decimation"] == 4 and fx["env"]["decimation"] == 40
    assert ll.obs_dim == m["low_level"]["obs_dim"] == 48 and ll.action_dim == m["low_level"]["action_dim"] == 12 and ll.cmd_dim == 3
    assert [t.name for t in ll.obs_terms] == m["low_level"]["obs_terms"]
    assert [[t.dim] for t in ll.obs_terms] == m["low_level"]["obs_term_dims"] and ll.enable_corruption
    assert [t.op for t in ll.obs_terms] == [O_OPS[k] for k in ("BASE_LIN_VEL", "BASE_ANG_VEL", "PROJECTED_GRAVITY", "GENERATED_COMMANDS", "JOINT_POS_REL",
                                                                "JOINT_VEL_REL", "LAST_ACTION")]
    assert len(ll.obs_groups) == 1 and ll.mod_state_dim == 0 and ll.num_rays == 0 and not ll.reward_terms and not ll.termination_terms
    assert os.path.isabs(pt.policy_path) and os.path.basename(pt.policy_path) == "navigation_low_level_policy.pt"
    # the library takes both blobs
    L = _lib.lib()
    for plan in (p, ll):
        blob, h = np.ascontiguousarray(plan.blob, np.int32), ctypes.c_void_p()
        assert L.imx_plan_create(blob.ctypes.data, blob.size, ctypes.byref(h)) == 0, L.imx_last_error().decode()
        L.imx_plan_destroy(h)


def test_variant_cfgs_compile_to_the_recorded_widths():
    for v in nc.VARIANTS:
        g = nc.NavGolden(v)
        fx, p = _plan(g.env_cfg())
        ll = p.policy_terms[0].low_level_plan
        assert ll.obs_dim == g.meta["obs_dim"] and [t.name for t in ll.obs_terms] == g.meta["ll_terms"] and [t.dim for t in ll.obs_terms] == g.meta["ll_term_dims"]
        assert p.policy_terms[0].low_level_decimation == g.meta["low_level_decimation"] and ll.enable_corruption == (v != "P3")


def test_command_width_and_feed():
    assert command_width({"class_type": _POSE_2D + "UniformPose2dCommand"}) == 4 == command_width({"class_type": _POSE_2D + "TerrainBasedPose2dCommand"})
    assert command_width({"class_type": "isaaclab.envs.mdp.commands.velocity_command:UniformVelocityCommand"}) == 3 and command_width(None) == 3
    feed = StateFeed(ANYMAL_C_NAV, 512, "cpu", seed=3, num_snapshots=2)
    c = feed["command"]
    assert c.shape == (512, 4) and c[:, :2].abs().max() <= 3.0 and c[:, :2].abs().max() > 2.5 and c[:, 2].abs().max() <= 0.05
    assert c[:, 3].abs().max() <= math.pi and c[:, 3].min() < -2.5 and c[:, 3].max() > 2.5
    base = StateFeed(ROBOTS["anymal_c"], 512, "cpu", seed=3, num_snapshots=2)  # every other tensor keeps its draws
    assert torch.equal(base["joint_pos"], feed["joint_pos"]) and torch.equal(base["root_quat_w"], feed["root_quat_w"])


def _edit(fn):
    fx = copy.deepcopy(nc.fixture())
    fn(fx["env"], fx["env"]["actions"][nc.TERM])
    return fx


def _scan_term(env, t):
    t["low_level_observations"]["height_scan"] = {"func": "isaaclab.envs.mdp.observations:height_scan", "params": {"sensor_cfg": {"name": "height_scanner"}}}
    env["scene"]["height_scanner"] = {"pattern_cfg": {"func": "isaaclab.sensors.ray_caster.patterns.patterns:grid_pattern", "resolution": 0.1, "size": [1.6, 1.0]},
                                      "offset": {"pos": [0.0, 0.0, 20.0]}, "attach_yaw_only": True}


_IK = {"class_type": "isaaclab.envs.mdp.actions.task_space_actions:DifferentialInverseKinematicsAction", "joint_names": [".*HAA"], "body_name": "base",
       "controller": {"command_type": "position", "ik_method": "dls"}}
REFUSALS = {
    "group history": (lambda e, t: t["low_level_observations"].update(history_length=3), r"low-level observation group with history \(history_length 3\)"),
    "term history": (lambda e, t: t["low_level_observations"]["joint_pos"].update(history_length=2), r"term 'joint_pos' has history"),
    "modifiers": (lambda e, t: t["low_level_observations"]["joint_vel"].update(modifiers=[{"func": "isaaclab.utils.modifiers.modifier:scale", "params": {"multiplier": 2.0}}]),
                  r"term 'joint_vel' has modifiers"),
    "height scan": (_scan_term, r"term 'height_scan' is a height scan"),
    "python term": (lambda e, t: t["low_level_observations"].update(mine={"func": "my_pkg.obs:something", "_dim": 2}), r"term 'mine' \(my_pkg.obs:something\) would be evaluated in Python"),
    "dict of terms": (lambda e, t: t["low_level_observations"].update(concatenate_terms=False), r"concatenate_terms=False feeds no policy"),
    "low-level class": (lambda e, t: t["low_level_actions"].update(class_type="isaaclab.envs.mdp.actions.binary_joint_actions:BinaryJointPositionAction"),
                        r"low-level action class .*BinaryJointPositionAction is not on the fused path"),
    "second term": (lambda e, t: e["actions"].update(second=copy.deepcopy(t)), r"'second': a second PreTrainedPolicyAction \(after 'pre_trained_policy_action'\)"),
    "beside IK": (lambda e, t: e["actions"].update(arm=_IK), r"'arm': a DifferentialInverseKinematicsAction beside the PreTrainedPolicyAction"),
    "beside a joint term": (lambda e, t: e["actions"].update(legs=copy.deepcopy(t["low_level_actions"])), r"beside other action terms \(\['legs'\]\)"),
    "no cfg": (lambda e, t: t.update(low_level_observations=None), r"without low_level_actions / low_level_observations"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_name_the_term_and_the_reason(case):
    edit, why = REFUSALS[case]
    fx = _edit(edit)
    with pytest.raises(NotImplementedError, match=why) as e:
        compile_plan(fx["env"], ROBOTS[fx["robot"]])
    assert "action term" in str(e.value)


def test_ik_before_the_policy_term_and_missing_remapped_terms():
    fx = copy.deepcopy(nc.fixture())
    fx["env"]["actions"] = {"arm": _IK, **fx["env"]["actions"]}
    with pytest.raises(NotImplementedError, match="a PreTrainedPolicyAction beside the task-space term 'arm'"):
        compile_plan(fx["env"], ROBOTS[fx["robot"]])
    fx = _edit(lambda e, t: t["low_level_observations"].pop("velocity_commands"))
    with pytest.raises(ValueError, match="no term 'velocity_commands'"):
        compile_plan(fx["env"], ROBOTS[fx["robot"]])
    # the nav rewards read a 4-wide command: on a velocity-command cfg they are refused with the reason
    fx = copy.deepcopy(nc.fixture())
    fx["env"]["commands"]["pose_command"]["class_type"] = "isaaclab.envs.mdp.commands.velocity_command:UniformVelocityCommand"
    with pytest.raises(ValueError, match=r"position_command_error_tanh reads a UniformPose2dCommand \(N, 4\); command 'pose_command' is 3 wide"):
        compile_plan(fx["env"], ROBOTS[fx["robot"]])


# ------------------------------------------------------------------------------------------------ the policy loader
def _seq(dims, act=torch.nn.ELU):
    torch.manual_seed(5)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(act())
    return torch.nn.Sequential(*mods)


class _Exported(torch.nn.Module):
    def __init__(self, actor, normalizer=None):
        super().__init__()
        self.actor, self.normalizer = actor, normalizer or torch.nn.Identity()

    def forward(self, x):
        return self.actor(self.normalizer(x))


class _Normalizer(torch.nn.Module):  # what rsl_rl's EmpiricalNormalization does at inference
    def __init__(self, d):
        super().__init__()
        self.register_buffer("_mean", torch.full((1, d), 0.1))
        self.register_buffer("_std", torch.full((1, d), 2.0))

    def forward(self, x):
        return (x - self._mean) / (self._std + 1e-2)


def test_loader_takes_the_archive_a_sequential_a_module_and_a_list(tmp_path):
    p = load_policy(nc.ARCHIVE)
    assert p.dims == [48, 128, 128, 128, 12] and p.elu_alpha == 1.0 and os.path.getsize(nc.ARCHIVE) < 200 * 1024
    x = torch.randn(5, 48, generator=torch.Generator().manual_seed(1))
    assert torch.equal(p.forward(x), torch.jit.load(nc.ARCHIVE)(x)) or (p.forward(x) - torch.jit.load(nc.ARCHIVE)(x)).abs().max() <= 1e-6
    seq = _seq([7, 33, 5])
    for src in (seq, torch.jit.script(seq), _Exported(seq), torch.jit.script(_Exported(seq))):
        q = load_policy(src)
        assert q.dims == [7, 33, 5] and torch.equal(q.layers[0][0], seq[0].weight.detach()) and torch.equal(q.layers[1][1], seq[2].bias.detach())
    path = str(tmp_path / "bare.pt")
    torch.jit.script(seq).save(path)
    assert load_policy(path).dims == [7, 33, 5]
    q = load_policy([(seq[0].weight, seq[0].bias), (seq[2].weight, seq[2].bias)])
    y = torch.randn(3, 7)
    assert q.dims == [7, 33, 5] and (q.forward(y) - seq(y)).abs().max() <= 1e-6
    alpha = torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.ELU(alpha=0.5), torch.nn.Linear(6, 2))
    assert load_policy(alpha).elu_alpha == 0.5 and (load_policy(alpha).forward(y[:, :4]) - alpha(y[:, :4])).abs().max() <= 1e-6


def test_loader_refusals(tmp_path):
    for src, why in ((_seq([4, 8, 8, 8, 8, 2]), "5 Linear layers; the fused path takes at most 4"),
                     (_seq([4, 513, 2]), "layer width 513; the fused path takes widths up to 512"),
                     (_seq([4, 8, 2], torch.nn.Tanh), "holds a Tanh"),
                     (_Exported(_seq([4, 8, 2]), _Normalizer(4)), "the normalizer is a _Normalizer; only the exporter's Identity"),
                     (torch.jit.script(_Exported(_seq([4, 8, 2]), _Normalizer(4))), "the normalizer is a _Normalizer"),
                     (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ELU(0.5), torch.nn.Linear(8, 8), torch.nn.ELU(1.0), torch.nn.Linear(8, 2)), "ELU alphas"),
                     (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Linear(8, 2)), r"not Linear \(ELU Linear\)\*"),
                     (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ELU()), "must end with a Linear"),
                     (torch.nn.LSTM(4, 8), "a LSTM with children"),
                     ([(torch.zeros(8, 4), torch.zeros(8)), (torch.zeros(2, 9), torch.zeros(2))], "layer 1 takes 9 inputs, layer 0 gives 8")):
        with pytest.raises(PolicyError, match=why):
            load_policy(src)
    with pytest.raises(TypeError, match="a path, an nn.Module or a list"):
        load_policy(3.5)
    # a path that is no local file: the reference's error, the keyword named, nothing fetched
    for path in ("omniverse://nucleus/Policies/ANYmal-C/Blind/policy.pt", str(tmp_path / "missing.pt"), None):
        with pytest.raises(FileNotFoundError, match=r"Policy file '.*' does not exist\..*low_level_policy=") as e:
            resolve_policy_path(path)
        assert not isinstance(e.value, PolicyError)
    junk = tmp_path / "junk.pt"
    junk.write_bytes(b"not an archive")
    with pytest.raises(PolicyError, match="is no TorchScript archive"):
        load_policy(str(junk))


def test_policy_path_is_resolved_beside_the_fixture(tmp_path):
    import json
    import shutil

    for name in (nc.TASK + ".json", nc.TASK + ".managers.json", "navigation_low_level_policy.pt"):
        shutil.copy(os.path.join(nc.GOLDEN, name), tmp_path / name)
    from isaaclab_amd.env import load_task_cfg

    fx = load_task_cfg(str(tmp_path / (nc.TASK + ".json")))
    assert fx["env"]["actions"][nc.TERM]["policy_path"] == str(tmp_path / "navigation_low_level_policy.pt")
    with open(nc.task_path()) as f:
        assert json.load(f)["env"]["actions"][nc.TERM]["policy_path"] == "navigation_low_level_policy.pt"  # the committed file stays relative


# ------------------------------------------------------------------------------------------------ the recordings and the restatement
@pytest.mark.parametrize("variant", nc.VARIANTS)
def test_fixture_covers_what_the_issue_asks(variant):
    g = nc.NavGolden(variant)
    m = g.meta
    assert m["N"] == 64 and m["steps"] == 3
    want = {"P1": (40, 4, 48, [48, 128, 128, 128, 12]), "P2": (6, 2, 45, [45, 96, 40, 12]), "P3": (40, 4, 48, [48, 128, 128, 128, 12])}[variant]
    assert (m["decimation"], m["low_level_decimation"], m["obs_dim"], m["policy_dims"]) == want
    assert m["launches"] == [m["decimation"] // m["low_level_decimation"]] * 3 and len(g.low_level_steps()) == sum(m["launches"])
    # all envs start at episode_length_buf 0, step 1 runs on (next to) none -- a base contact may have reset an env --, step 2 on the envs a
    # time-out reset
    ep = [g.t(f"step{t}/episode_length_buf") for t in range(3)]
    assert (ep[0] == 0).all() and int((ep[1] > 0).sum()) >= 60 and 16 <= int((ep[2] == 0).sum()) < 64
    assert g.t("step1/time_outs")[::4].all() and not g.t("step0/time_outs").any()
    # the zeroed block shows: the recorded `actions` columns of step 2's first low-level step are 0 exactly on the reset envs (P3: no noise)
    if variant == "P3":
        a0 = g.t("step2/ll0/obs")[:, -12:]
        assert (a0[ep[2] == 0] == 0).all() and (a0[ep[2] != 0] != 0).any(dim=1).all()
        assert not g.has("step0/ll0/noise_u") and g.term["low_level_actions"]["clip"] and isinstance(g.term["low_level_actions"]["scale"], dict)
        lo_hi = g.t("step1/ll3/joint_pos_target")
        assert lo_hi[:, :4].abs().max() <= 0.3 + 1e-7  # the clipped HAA joints
    else:
        assert g.has("step2/ll0/noise_u") and g.t("step2/ll0/noise_u").shape == (64, m["obs_dim"])
    # the term's raw action is the action, untouched by the reset; low_level_actions stay too (the term has no reset)
    assert torch.equal(g.t("step1/raw_after_reset"), g.t("step1/raw"))
    last = m["launches"][1] - 1
    assert torch.equal(g.t("step1/low_level_actions_after_reset"), g.t(f"step1/ll{last}/low_level_actions"))


@pytest.mark.parametrize("variant", nc.VARIANTS)
def test_restatement_reproduces_the_reference_in_fp32(variant):
    """Every env, every low-level step: the fp32 restatement, carrying its own low_level_actions from step to step, against the
    recording of the real class under assert_close; the recording lies within the same rule of the fp64 one (the generator's
    own assertion, here with the restatement's own low_level_actions carried along)."""
    g = nc.NavGolden(variant)
    r32, r64 = nc.restate(g, torch.float32), nc.restated(variant)
    assert list(r32) == g.low_level_steps() and len(r32) == sum(g.meta["launches"])
    count = 0
    for (t, k), got in r32.items():
        for name, x, y in zip(nc.LL_OUTPUTS, got, r64[(t, k)]):
            ref = g.t(f"step{t}/ll{k}/{name}")
            assert x.shape == ref.shape == (64, ref.shape[1])
            assert_close(x, ref, FLOAT_TOL, f"{variant} step {t} ll {k} {name}")
            assert_close(ref, y, FLOAT_TOL, f"{variant} step {t} ll {k} {name}: the recording against the fp64 restatement")
            count += x.shape[0]
    assert count == 64 * 3 * sum(g.meta["launches"])
    for name in nc.LL_OUTPUTS:  # the reference's own fp32 error, the floor of the GPU tests' bound: rounding, nothing more
        assert 0.0 < nc.e_ref(variant, name) < 1.0e-6, (variant, name, nc.e_ref(variant, name))


def test_env_step_terms_of_the_restatement():
    import _navigation_oracle as no

    g = nc.NavGolden("P1")
    fx = nc.fixture()
    base = ROBOTS[fx["robot"]].body_names.index("base")
    for t in range(3):
        st = g.state(t + 1) if t + 1 < 3 else None
        if st is None:
            break
        ep = g.t(f"step{t}/episode_length_buf") + 1
        to, contact = no.terminations(st, ep, g.meta["max_episode_length"], [base], 1.0)
        assert torch.equal(to, g.t(f"step{t}/time_outs")) and torch.equal(contact, g.t(f"step{t}/terminated"))
        rew, terms = no.rewards(g.meta["rewards"], st, contact, g.meta["step_dt"])
        assert_close(rew, g.t(f"step{t}/reward"), FLOAT_TOL, f"step {t} reward")
        assert_close(terms, g.t(f"step{t}/step_reward"), FLOAT_TOL, f"step {t} step_reward")
        assert_close(no.policy_observation(st, g.meta["gravity_dir"]), g.t(f"step{t}/policy_obs"), FLOAT_TOL, f"step {t} obs")


# ------------------------------------------------------------------------------------------------ the ABI
def test_entry_point_and_struct_are_declared_and_bound():
    with open(os.path.join(nc.ROOT, "include", "imx.h")) as f:
        h = f.read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct imx_pretrained_policy imx_pretrained_policy_t;\s*#include \"imx_pretrained_policy_struct.h\"\s*"
                  r"int imx_pretrained_policy\(([^;]*)\);", h, re.S)
    assert m, "imx_pretrained_policy is not declared in include/imx.h"
    comment = " ".join(m.group(1).replace("\n * ", " ").split())
    for cite in ("pre_trained_policy_action.py:93-100", ":53-57", "ONE launch", "bit for bit", "Refused without a launch"):
        assert cite in comment, cite
    res, args = _lib._SIGNATURES["imx_pretrained_policy"]
    assert res is ctypes.c_int and len(args) == 14 and args[4] is ctypes.POINTER(_lib.ImxPretrainedPolicy)
    assert list(_abi.POLICY_STRUCTS) == ["imx_pretrained_policy_t"] and "imx_pretrained_policy_t" not in _abi.STRUCTS and len(_abi.STRUCTS) == 8
    assert _abi.DEFINES["IMX_PP_MAX_LAYERS"] == 4 == _lib.PP_MAX_LAYERS
    assert ctypes.sizeof(_lib.ImxPretrainedPolicy) == 4 * (1 + 5 + 4 + 1 + 1) + 8 * 12
    L = _lib.lib()
    assert int(L.imx_struct_size(12)) == ctypes.sizeof(_lib.ImxPretrainedPolicy) and int(L.imx_struct_size(9)) == 0
    assert "pretrained_policy.hip" in __import__("isaaclab_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_compiler_agrees_with_the_binding_of_imx_pretrained_policy_t(tmp_path):
    """The struct is defined in include/imx_pretrained_policy_struct.h (imx.h includes it) and bound from there by the same parser: a C++
    compiler that reads imx.h must see the size, every field's offset, size and kind, and the entry points' signatures as the binding has
    them."""
    import subprocess

    from _task_space_cases import host_compiler
    from test_abi import unit

    if host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    cls = _lib.ImxPretrainedPolicy
    assert [f for f, _ in cls._fields_] == [f for f, _ in _abi.POLICY_STRUCTS["imx_pretrained_policy_t"]]
    sigs = {n: _lib._SIGNATURES[n] for n in ("imx_pretrained_policy", "imx_pretrained_policy_check", "imx_pretrained_policy_tile_rows")}
    text = unit({"imx_pretrained_policy_t": cls}, sigs, {"imx_rew_op": {k: v for k, v in _abi.ENUMS["imx_rew_op"].items() if "_NAV_" in k}},
                {"IMX_PP_MAX_LAYERS": 4})
    assert text.count("offset, size") == len(cls._fields_) == 8 and text.count("enum member") == 2
    src = tmp_path / "pp_abi.cpp"

    def compiles(t):
        src.write_text(t)
        r = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-I", f"{nc.ROOT}/include", str(src)], capture_output=True, text=True)
        return "" if r.returncode == 0 else (r.stderr or f"exit status {r.returncode}")

    assert compiles(text) == ""
    fields = list(cls._fields_)
    i = [n for n, _ in fields].index("weights_d")
    fields[i], fields[i + 1] = fields[i + 1], fields[i]  # two pointer arrays swapped: only the offsets can tell
    err = compiles(unit({"imx_pretrained_policy_t": type("ImxPretrainedPolicy", (ctypes.Structure,), {"_fields_": fields})}, {}, {}, {}))
    assert "static" in err and "imx_pretrained_policy_t.weights_d offset, size" in err, err


def test_argument_checks_run_before_any_launch():
    """The refusals of ``imx_pretrained_policy`` need no GPU (``imx_pretrained_policy_check`` is the entry point's own check function;
    the pointers are never dereferenced on the host).  The GPU file repeats a few through the entry point itself."""
    L = _lib.lib()
    fx, p = _plan()
    ll = p.policy_terms[0].low_level_plan
    blob, h = np.ascontiguousarray(ll.blob, np.int32), ctypes.c_void_p()
    assert L.imx_plan_create(blob.ctypes.data, blob.size, ctypes.byref(h)) == 0
    main_blob, hm = np.ascontiguousarray(p.blob, np.int32), ctypes.c_void_p()
    assert L.imx_plan_create(main_blob.ctypes.data, main_blob.size, ctypes.byref(hm)) == 0
    fake = 0x1000
    state = {n: fake for n in ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w", "joint_pos", "joint_vel", "default_joint_pos",
                               "default_joint_vel", "command")}
    bufs = dict(episode_length_buf=fake, action=fake, prev_action=fake, processed_action=fake)

    def policy(**kw):
        c = _lib.ImxPretrainedPolicy(nlayers=4, elu_alpha=1.0)
        for i, d in enumerate((48, 128, 128, 128, 12)):
            c.dims[i] = d
        for i, pitch in enumerate((64, 128, 128, 128)):
            c.weight_pitch[i] = pitch
            c.weights_d[i] = c.biases_d[i] = fake
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def call(plan=h, N=8, st=None, bf=None, pol=None, rows=0, null=()):
        s = _lib.ImxState(**{**state, **(st or {})})
        b = _lib.ImxBuffers(**{**bufs, **(bf or {})})
        c = pol or policy()
        args = dict(plan=plan, st=ctypes.byref(s), bf=ctypes.byref(b), pol=ctypes.byref(c))
        for n in null:
            args[n] = None
        return L.imx_pretrained_policy_check(args["plan"], N, args["st"], args["bf"], args["pol"], rows)

    assert call() == 0 and call(rows=16) == 0 and call(rows=32) == 0 and call(N=1) == 0
    cases = (
        (dict(null=("plan",)), "null plan"), (dict(null=("st",)), "null plan / state"), (dict(null=("bf",)), "buffers"), (dict(null=("pol",)), "policy"),
        (dict(N=0), "num_envs out of range: 0"), (dict(N=-3), "num_envs"), (dict(rows=8), "tile_rows 8"), (dict(rows=64), "tile_rows 64"),
        (dict(plan=hm), "the policy takes 48 inputs, the low-level observation group has 10"),
        (dict(pol=policy(nlayers=0)), "0 layers"), (dict(pol=policy(nlayers=5)), "5 layers"),
        (dict(pol=policy(dims=(1, 513))), "layer width 513"), (dict(pol=policy(dims=(2, 0))), "layer width 0"),
        (dict(pol=policy(dims=(0, 45))), "the policy takes 45 inputs"), (dict(pol=policy(dims=(4, 11))), "the policy has 11 outputs, the low-level action term 12"),
        (dict(pol=policy(weights_d=(2, None))), "null weight / bias (layer 2)"), (dict(pol=policy(biases_d=(0, None))), "null weight / bias (layer 0)"),
        (dict(pol=policy(weights_d=(1, fake + 4))), "weights of layer 1 need a 16-byte aligned"),
        (dict(pol=policy(weight_pitch=(0, 48))), "pitch 48, in-features 48"), (dict(pol=policy(weight_pitch=(1, 96))), "pitch 96, in-features 128"),
        (dict(pol=policy(packed_weights_d=(0, fake))), "packed weights must be given for every layer or for none"),
        (dict(st=dict(root_quat_w=None)), "root state missing"), (dict(st=dict(joint_pos=None)), "'joint_pos/default_joint_pos' is required"),
        (dict(st=dict(default_joint_vel=None)), "'joint_vel/default_joint_vel' is required"), (dict(st=dict(command=None)), "'command' is required"),
        (dict(bf=dict(action=None)), "'action' is required"), (dict(bf=dict(episode_length_buf=None)), "null episode_length_buf"),
        (dict(bf=dict(processed_action=None)), "null action buffer"), (dict(bf=dict(prev_action=None)), "null action buffer"),
    )
    for kw, why in cases:
        assert call(**kw) != 0, kw
        msg = L.imx_last_error().decode()
        assert (msg.startswith("imx_pretrained_policy: ") or "imx_pretrained_policy" in msg) and why in msg, (kw, msg)
    # the entry point itself runs the same checks first (no device is touched for a refused call)
    s, b, c = _lib.ImxState(**state), _lib.ImxBuffers(**bufs), policy()
    assert L.imx_pretrained_policy(h, 0, ctypes.byref(s), ctypes.byref(b), ctypes.byref(c), None, 0, None, 1, 0, 1, 0, None, None) != 0
    assert "num_envs" in L.imx_last_error().decode()
    assert L.imx_pretrained_policy(h, 8, ctypes.byref(s), ctypes.byref(b), None, None, 0, None, 1, 0, 1, 0, None, None) != 0
    L.imx_plan_destroy(h)
    L.imx_plan_destroy(hm)
