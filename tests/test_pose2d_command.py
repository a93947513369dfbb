"""The env's own ``UniformPose2dCommand`` / ``TerrainBasedPose2dCommand`` without a GPU: the CPU restatement (tests/_pose2d_oracle.py) and
the per-env device function run as host C++ (tools/pose2d_host.cpp) against the fixtures of the REAL classes
(tests/golden/pose2d_command.npz, tools/gen_golden_pose2d_command.py), the C interface and its ctypes mirror, the producers' constructors."""

import ctypes
import os
import subprocess

import pytest
import torch

from _pose2d_cases import OUT_KEYS, VARIANTS, NavOrchGolden, Pose2dGolden, assert_outputs_close, term_outputs, wrap_to_pi
from _util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAV_CFG = {"resampling_time_range": (8.0, 8.0), "simple_heading": False,
           "ranges": {"pos_x": (-3.0, 3.0), "pos_y": (-3.0, 3.0), "heading": (-3.14, 3.14)}}


# An angle of the host-C++ run against torch's: the two atan2f behind it (the target direction, the robot's heading) each differ by up to
# an ulp at pi (2^-22), and that difference can move each of the four roundings on the way (+ pi, the remainder - pi, - heading, + pi
# again: intermediates below 2 pi, ulp 2^-21) by one ulp
ANGLE_BOUND = 2 * 2.0 ** -22 + 4 * 2.0 ** -21


def test_fixture_margins_and_shapes():
    """What the generator promises: N = 300, 12 steps, the three variants, and no decision within an ulp of flipping."""
    for v in VARIANTS:
        g = Pose2dGolden(v)
        assert (g.N, g.steps, g.kind) == (300, 12, int(v == "T1")) and g.cfg["simple_heading"] == (v != "U0")
        assert g.meta["min_wrap_margin"] >= 1e-4 and g.meta["min_time_left_margin"] >= g.step_dt / 100
        assert (g.meta["min_tie_margin"] is None) if v == "U0" else g.meta["min_tie_margin"] >= 1e-4
        assert g.meta["metrics_before_first_compute"] == ["error_pos", "error_heading"]
        assert g.meta["metrics"] == ["error_pos", "error_heading", "error_pos_2d"]
        assert float(g.constants()["env_origins"].abs().min()) > 0.0
        assert all(float(g.t(f"step{k}/error_pos").abs().max()) == 0.0 for k in range(g.steps))  # the reference never writes it
    assert tuple(Pose2dGolden("T1").constants()["valid_targets"].shape) == (3, 4, 5, 3)


@pytest.mark.parametrize("variant", VARIANTS)
def test_pose2d_oracle_matches_reference(variant):
    """Counters and reset masks bit for bit, floats within 1e-6 (the figure of tests/test_pose_command.py), heading_command_w on the
    circle.  The metrics' keys appear as in the reference: error_pos_2d only after the first compute."""
    g = Pose2dGolden(variant)
    orc = g.oracle()
    assert list(orc.metrics) == ["error_pos", "error_heading"]
    timer_resampled = flipped = 0
    for k in range(g.steps):
        d = g.inputs(k)
        before = orc.command_counter.clone()
        orc.reset_and_compute(g.step_dt, d["root_pos_w"], d["root_quat_w"], d["reset_mask"], d["uniforms"], d["patch_ids"])
        timer_resampled += int(((orc.command_counter > before) & ~d["reset_mask"]).sum())
        assert list(orc.metrics) == g.meta["metrics"]
        assert_outputs_close(term_outputs(orc), g.expected(k), 1e-6, f"{variant} step {k}")
        assert torch.equal(orc.command_counter[d["reset_mask"]] >= 1, torch.ones(int(d["reset_mask"].sum()), dtype=torch.bool))
        if variant != "U0":  # both candidates of the simple heading are taken
            tv = orc.pos_command_w - d["root_pos_w"]
            flipped += int(((torch.atan2(tv[:, 1], tv[:, 0]) - orc.heading_command_w).abs() > 1.0).sum())
    assert timer_resampled > 100  # the (2, 5) x step_dt range makes the timer path run, not only the reset path
    assert variant == "U0" or flipped > 100


def test_pose2d_oracle_matches_the_orchestration_fixture():
    """The restatement over ``reset`` and the 40 recorded steps of tests/golden/navigation_orchestration*.npz (the REAL ``_reset_idx`` +
    ``CommandManager.compute`` of ``NavigationEnvCfg``): the recorded root poses, draws and reset ids in; command, pos_command_w,
    heading_command_w (on the circle), timer and metrics within 1e-6, the counter and the metrics' keys exact, and the
    ``Metrics/pose_command/*`` entries of the recorded log within 1e-6 at every recorded point.  The fixture's stored margins hold."""
    from _pose2d_oracle import Pose2dOracle

    g = NavOrchGolden()
    m = g.meta
    assert (g.N, g.steps, m["command_term"]) == (64, 40, "pose_command") and m["event_terms"] == {"reset": ["reset_base"]}
    assert m["min_wrap_margin"] >= 1e-4 and m["min_time_left_margin"] >= m["step_dt"] / 100 and m["min_tie_margin"] is None
    assert m["metrics"] == ["error_pos", "error_heading", "error_pos_2d"] and 60 <= m["n_resets"] <= 200 and m["n_timer_resamplings"] > 100
    ccfg = g.fixture["env"]["commands"]["pose_command"]
    assert ccfg["simple_heading"] is False and tuple(ccfg["resampling_time_range"]) == (0.4, 1.2)
    assert float(g.t("static/env_origins")[:, :2].abs().max()) > 0.0
    orc = Pose2dOracle(ccfg, g.N, g.t("static/env_origins"), g.t("static/default_root_state")[:, 2])
    log, resets, timer = {}, 0, 0
    for slot, tag in enumerate(["reset"] + [f"step{k}" for k in range(g.steps)]):
        mask = g.reset_mask(tag)
        before = orc.command_counter.clone()
        new = orc.reset_and_compute(m["step_dt"], g.t(f"{tag}/in/root_pos_w"), g.t(f"{tag}/in/root_quat_w"), mask, g.t("draws/command")[slot],
                                    do_compute=tag != "reset")
        if bool(mask.any()):  # (a step without resets leaves the log as it was, as the reference's extras["log"])
            log = {f"Metrics/pose_command/{k}": v for k, v in new.items()}
        resets += int(mask.sum()) if tag != "reset" else 0
        timer += int(((orc.command_counter > before) & ~mask).sum())
        assert [k for k in g.z.files if k.startswith(f"{tag}/metric_")] == [f"{tag}/metric_{k}" for k in orc.metrics], tag
        got = {"command": orc.command, "pos_command_w": orc.pos_command_w, "heading_command_w": orc.heading_command_w,
               "time_left": orc.time_left, "command_counter": orc.command_counter, **orc.metrics}
        ref = {"command": g.t(f"{tag}/command"), "pos_command_w": g.t(f"{tag}/pos_command_w"), "heading_command_w": g.t(f"{tag}/heading_command_w"),
               "time_left": g.t(f"{tag}/command_time_left"), "command_counter": g.t(f"{tag}/command_counter"),
               **{k: g.t(f"{tag}/metric_{k}") for k in orc.metrics}}
        assert_outputs_close(got, ref, 1e-6, tag, names=tuple(ref))
        want = {k: v for k, v in g.log(tag).items() if k.startswith("Metrics/")}
        assert list(want) == list(log), (tag, list(want), list(log))
        for k, v in want.items():
            assert abs(log[k] - v) <= 1e-6 * max(1.0, abs(v)), (tag, k, log[k], v)
    assert resets == m["n_resets"] and timer == m["n_timer_resamplings"]
    assert float(orc.metrics["error_pos"].abs().max()) == 0.0


def test_pose2d_oracle_fp64_agrees_with_fp32():
    """The fp64 run of the restatement takes the same decisions (the margins) and lands within 1e-5 of the fp32 reference."""
    for v in VARIANTS:
        g = Pose2dGolden(v)
        orc = g.oracle(dtype=torch.float64)
        for k in range(g.steps):
            d = g.inputs(k)
            orc.reset_and_compute(g.step_dt, d["root_pos_w"], d["root_quat_w"], d["reset_mask"], d["uniforms"], d["patch_ids"])
            assert_outputs_close(term_outputs(orc), g.expected(k), 1e-5, f"{v} fp64 step {k}")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    import _task_space_cases as tsc

    if tsc.host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    return tsc.build_host_program("pose2d_host", str(tmp_path_factory.mktemp("pose2d_host")))


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_function_as_host_code_matches_reference(host_program, tmp_path, variant):
    """pose2d_command_env (csrc/imx_pose2d.h), compiled as plain C++, over all 12 steps.  Counters, the timer and what is copied
    (kind 1: pos_command_w) bit for bit; floats within 1e-6, and the base-frame position within 1e-6 + 2^-21 ||target||: the C library's
    atan2f / sinf / cosf and torch's each round to about an ulp, so the yaw angle of yaw_quat may differ by ~4 ulp of 1 rad (2^-21) and
    the rotated vector by that angle times its length -- which shows in a component much smaller than the vector.  The angles (both
    headings, error_heading) within ANGLE_BOUND on the circle."""
    g = Pose2dGolden(variant)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    g.host_file(fin)
    subprocess.check_call([host_program, fin, fout])
    for k, got in enumerate(g.read_host_output(fout)):
        ref = g.expected(k)
        assert torch.equal(got["time_left"], ref["time_left"]) and torch.equal(got["command_counter"], ref["command_counter"])
        if g.kind == 1:
            assert torch.equal(got["pos_command_w"], ref["pos_command_w"])
        pos_err = (got["command"][:, :3] - ref["command"][:, :3]).abs()
        bound = 1e-6 * ref["command"][:, :3].abs().clamp(min=1.0) + 2.0 ** -21 * ref["command"][:, :3].norm(dim=-1, keepdim=True)
        assert bool((pos_err <= bound).all()), (variant, k, float(pos_err.max()))
        for name, a, b in (("heading_command_b", got["command"][:, 3], ref["command"][:, 3]), ("error_heading", got["error_heading"], ref["error_heading"]),
                           ("heading_command_w", got["heading_command_w"], ref["heading_command_w"])):
            err = wrap_to_pi(a.double() - b.double()).abs()
            assert float(err.max()) <= ANGLE_BOUND, (variant, k, name, float(err.max()))
        # (command, error_heading and heading_command_w are held to their own bounds above, not to 1e-6)
        assert_outputs_close(got, ref, 1e-6, f"{variant} host step {k}", names=("pos_command_w", "time_left", "error_pos_2d", "command_counter"))


def test_host_program_refuses_bad_files(host_program, tmp_path):
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 64)
    assert subprocess.run([host_program, str(bad), str(tmp_path / "o")], capture_output=True).returncode == 2
    g = Pose2dGolden("T1")
    fin = tmp_path / "in.bin"
    g.host_file(str(fin))
    fin.write_bytes(fin.read_bytes()[:-100])  # the last step is truncated
    r = subprocess.run([host_program, str(fin), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 2 and "truncated" in r.stderr


def test_c_interface_and_binding(libimx):
    """The two symbols, the struct of its own header at index 13, and the pinned sizes that must not move."""
    from isaaclab_amd import _abi, _lib

    h = open(os.path.join(ROOT, "include", "imx.h")).read()
    assert '#include "imx_pose2d_struct.h"' in h and "typedef struct imx_pose2d_command imx_pose2d_command_t;" in h
    assert "pose_2d_command.py:26-143" in h and ":146-203" in h and "command_manager.py:120-187" in h
    for fn in ("imx_pose2d_command", "imx_reset_orchestrate_pose2d"):
        assert fn in _lib.EXPORTS and hasattr(libimx, fn)
    res, args = _lib._SIGNATURES["imx_pose2d_command"]
    assert res is ctypes.c_int and len(args) == 10 and args[1] is ctypes.POINTER(_lib.ImxPose2dCommand)
    res, args = _lib._SIGNATURES["imx_reset_orchestrate_pose2d"]
    assert res is ctypes.c_int and args[:2] == [ctypes.POINTER(_lib.ImxOrch), ctypes.POINTER(_lib.ImxPose2dCommand)]
    assert int(libimx.imx_struct_size(13)) == ctypes.sizeof(_lib.ImxPose2dCommand) > 0
    assert int(libimx.imx_struct_size(5)) == 1944 == ctypes.sizeof(_lib.ImxOrch) and int(libimx.imx_struct_size(9)) == 0
    assert int(libimx.imx_struct_size(14)) == 0
    assert list(_abi.POSE2D_STRUCTS) == ["imx_pose2d_command_t"] and "imx_pose2d_command_t" not in _abi.STRUCTS and len(_abi.STRUCTS) == 8
    assert [f for f, _ in _lib.ImxPose2dCommand._fields_] == [f for f, _ in _abi.POSE2D_STRUCTS["imx_pose2d_command_t"]]
    assert _lib.ImxPose2dCommand.cfg.size == 32 and _lib.ImxPose2dCommand.env_origins_d.offset == 40


def test_the_compiler_agrees_with_the_struct():
    """sizeof / offsetof of every field of imx_pose2d_command_t as a C++ compiler lays it out (the recipe of tests/test_abi.py)."""
    import _task_space_cases as tsc
    from isaaclab_amd import _lib

    cxx = tsc.host_compiler()
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    cls = _lib.ImxPose2dCommand
    lines = ['#include <cstddef>', '#include "imx.h"', f'static_assert(sizeof(imx_pose2d_command_t) == {ctypes.sizeof(cls)}, "size");']
    for field, _ in cls._fields_:
        f = getattr(cls, field)
        lines.append(f'static_assert(offsetof(imx_pose2d_command_t, {field}) == {f.offset} && sizeof(imx_pose2d_command_t::{field}) == {f.size}, "{field}");')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", "-x", "c++", "-"], input="\n".join(lines) + "\n",
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_producer_metrics_follow_the_reference_quirk():
    """The constructor creates error_pos and error_heading; error_pos_2d exists only after the first compute (``mark_computed`` is what a
    launch with do_compute calls); error_pos is never written."""
    from isaaclab_amd import producers

    term = producers.UniformPose2dCommand(NAV_CFG, 8, 0.2, "cpu", env_origins=torch.ones(8, 3), default_root_z=0.6)
    assert list(term.metrics) == ["error_pos", "error_heading"]
    assert tuple(term.command.shape) == (8, 4) and term.command.is_contiguous()
    assert term.pos_command_b.data_ptr() == term.command.data_ptr() and term.heading_command_b.data_ptr() == term.command[:, 3].data_ptr()
    assert tuple(term.pos_command_w.shape) == (8, 3) and tuple(term.heading_command_w.shape) == (8,)
    assert term.time_left.shape == (8,) and term.command_counter.dtype == torch.long and not term.simple_heading and term.kind == 0
    assert torch.equal(term.default_root_z, torch.full((8,), 0.6)) and torch.equal(term.env_origins, torch.ones(8, 3))
    term.mark_computed()
    assert list(term.metrics) == ["error_pos", "error_heading", "error_pos_2d"]
    assert float(term.metrics["error_pos"].abs().max()) == 0.0
    c = term.struct()
    assert (c.kind, c.simple_heading) == (0, 0) and [round(v, 2) for v in c.cfg] == [8.0, 8.0, -3.0, 3.0, -3.0, 3.0, -3.14, 3.14]
    assert c.metric_error_pos_2d_d == term.metrics["error_pos_2d"].data_ptr() and c.command_d == term.command.data_ptr()
    assert c.valid_targets_d is None and c.uniforms_d is None


def test_producer_constructor_refusals():
    from isaaclab_amd import producers

    with pytest.raises(ValueError, match="resampling_time_range"):
        producers.UniformPose2dCommand(dict(NAV_CFG, resampling_time_range=(0.0, 0.0)), 8, 0.2, "cpu")
    with pytest.raises(ValueError, match="ranges.heading"):
        producers.UniformPose2dCommand(dict(NAV_CFG, ranges={"pos_x": (-1, 1), "pos_y": (-1, 1), "heading": None}), 8, 0.2, "cpu")
    with pytest.raises(ValueError, match="env_origins"):
        producers.UniformPose2dCommand(NAV_CFG, 8, 0.2, "cpu", env_origins=torch.zeros(7, 3))
    with pytest.raises(ValueError, match="root_pos_w"):
        producers.UniformPose2dCommand(NAV_CFG, 8, 0.2, "cpu").compute(0.2)
    vt, lv, ty = torch.zeros(3, 4, 5, 3), torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long)
    T = producers.TerrainBasedPose2dCommand
    with pytest.raises(ValueError, match="valid_targets="):
        T(NAV_CFG, 8, 0.2, "cpu")
    with pytest.raises(ValueError, match=r"\(L, T, P, 3\)"):
        T(NAV_CFG, 8, 0.2, "cpu", valid_targets=torch.zeros(3, 4, 5), terrain_levels=lv, terrain_types=ty)
    with pytest.raises(ValueError, match=r"terrain_levels has entries outside \[0, 3\)"):
        T(NAV_CFG, 8, 0.2, "cpu", valid_targets=vt, terrain_levels=lv + 3, terrain_types=ty)
    with pytest.raises(ValueError, match=r"terrain_types has entries outside \[0, 4\)"):
        T(NAV_CFG, 8, 0.2, "cpu", valid_targets=vt, terrain_levels=lv, terrain_types=ty - 1)
    with pytest.raises(ValueError, match="int64"):
        T(NAV_CFG, 8, 0.2, "cpu", valid_targets=vt, terrain_levels=lv.int(), terrain_types=ty)
    term = T(dict(NAV_CFG, simple_heading=True), 8, 0.2, "cpu", valid_targets=vt, terrain_levels=lv, terrain_types=ty)
    c = term.struct()
    assert (c.kind, c.simple_heading, c.num_levels, c.num_types, c.num_patches) == (1, 1, 3, 4, 5) and c.valid_targets_d == term.valid_targets.data_ptr()
    assert isinstance(term, producers.UniformPose2dCommand) and OUT_KEYS[0] == "command"
    assert_close(term.command, torch.zeros(8, 4), 1e-6, "the command starts at zero")
