"""The env's own ``UniformPoseCommand`` without a GPU: the CPU restatement against the fixtures of the REAL class
(tests/golden/pose_command.npz, tools/gen_golden_pose_command.py), the C interface and its ctypes mirror, the producer's constructor."""

import ctypes
import os
import re

import pytest
import torch

from _pose_command_cases import OUT_KEYS, PoseGolden, term_outputs
from _util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", ["A", "B"])
def test_pose_command_oracle_matches_reference(variant):
    """A: the Franka task's ranges (roll 0, pitch pi, no quat_unique: w ~ -4e-8 cos(yaw / 2)); B: every angle in (-3.14, 3.14) with
    quat_unique.  Ints and the timer bit for bit, floats within 1e-6 (the figure of the velocity restatement, test_producers.py)."""
    from _pose_command_oracle import PoseCommandOracle

    g = PoseGolden(variant)
    assert g.N == 300 and g.steps == 12 and g.body_idx == 8
    orc = PoseCommandOracle(g.cfg, g.N, g.step_dt, g.body_idx)
    assert float(orc.pose_command_b[:, 3].min()) == 1.0
    timer_resampled = 0
    for k in range(g.steps):
        d = g.inputs(k)
        before = orc.command_counter.clone()
        orc.reset_and_compute(g.step_dt, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"], d["reset_mask"], d["uniforms"])
        timer_resampled += int(((orc.command_counter > before) & ~d["reset_mask"]).sum())
        got, ref = term_outputs(orc), g.expected(k)
        for name in OUT_KEYS:
            if name in ("command_counter", "time_left"):
                assert torch.equal(got[name], ref[name]), (k, name)
            else:
                assert_close(got[name], ref[name], 1e-6, f"{variant} step {k} {name}")
    assert timer_resampled > 100  # the (2, 5) x step_dt range makes the timer path run, not only the reset path
    if variant == "A":  # w = cos(pi / 2 in fp32) cos(yaw / 2) ~ -4.4e-8 cos(yaw / 2): tiny and negative, kept (no quat_unique)
        w = torch.cat([g.expected(k)["pose_command_b"][:, 3] for k in range(g.steps)])
        assert float(w.abs().max()) < 1e-6 and bool((w < 0).all())
    else:
        assert all(float(g.expected(k)["pose_command_b"][:, 3].min()) >= 0.0 for k in range(g.steps))


def test_c_interface_and_binding_grew_only_at_the_tail():
    """include/imx.h declares imx_pose_command, _lib.py carries its signature, and imx_orch_t / ImxOrch grew at the END: the offsets of
    has_command and ev_part_d are the parent's (1648, 1896; the parent struct was 1904 bytes)."""
    from isaaclab_amd import _lib

    h = open(os.path.join(ROOT, "include", "imx.h")).read()
    m = re.search(r"int imx_pose_command\(([^;]*)\);", h)
    assert m, "imx_pose_command is not declared in include/imx.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert "pose_command.py:25-127" in h and "command_manager.py:120-187" in h
    res, args = _lib._SIGNATURES["imx_pose_command"]
    assert res is ctypes.c_int and len(args) == nargs == 22
    assert "imx_pose_command" in _lib.EXPORTS
    O = _lib.ImxOrch
    assert O.has_command.offset == 1648 and O.ev_part_d.offset == 1896
    tail = [n for n, _ in O._fields_][[n for n, _ in O._fields_].index("ev_part_d") + 1:]
    assert tail == ["pose_command_b_d", "pose_command_w_d", "body_pos_w_d", "body_quat_w_d", "pose_body_idx", "make_quat_unique"]
    assert O.pose_command_b_d.offset == 1904 and ctypes.sizeof(O) == 1904 + 4 * 8 + 2 * 4
    # the struct in the header lists the same tail after ev_part_d
    body = h[h.index("typedef struct imx_orch {"):h.index("} imx_orch_t;")]
    after = body[body.index("float* ev_part_d;"):]
    pos = [after.index(n) for n in tail]
    assert pos == sorted(pos)


def test_producer_resolves_the_body_name_and_starts_at_identity():
    from isaaclab_amd import producers
    from isaaclab_amd.robots import FRANKA_PANDA

    cfg = PoseGolden("A").cfg
    term = producers.UniformPoseCommand(cfg, 8, 1.0 / 30.0, "cpu", robot=FRANKA_PANDA)
    assert cfg["body_name"] == "panda_hand" and term.body_idx == 8 and term.num_bodies == FRANKA_PANDA.num_bodies
    assert term.command is term.pose_command_b and tuple(term.command.shape) == (8, 7)
    assert torch.equal(term.pose_command_b, torch.tensor([0.0, 0, 0, 1, 0, 0, 0]).repeat(8, 1))
    assert torch.equal(term.pose_command_w, torch.zeros(8, 7))
    assert list(term.metrics) == ["position_error", "orientation_error"]
    assert term.time_left.shape == (8,) and term.command_counter.dtype == torch.long and not term.make_quat_unique
    assert producers.UniformPoseCommand(dict(cfg, make_quat_unique=True), 8, 1.0 / 30.0, "cpu", robot=FRANKA_PANDA).make_quat_unique
    with pytest.raises(ValueError, match="no_such_body"):
        producers.UniformPoseCommand(dict(cfg, body_name="no_such_body"), 8, 1.0 / 30.0, "cpu", robot=FRANKA_PANDA)
    with pytest.raises(ValueError, match="robot="):
        producers.UniformPoseCommand(cfg, 8, 1.0 / 30.0, "cpu")
