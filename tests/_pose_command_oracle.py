"""TEST INFRASTRUCTURE -- CPU restatement (fp32 torch) of ``CommandTerm.reset / compute`` + ``UniformPoseCommand``
(isaaclab/managers/command_manager.py:120-187; isaaclab/envs/mdp/commands/pose_command.py:25-127), pinned by
tests/golden/pose_command.npz (tools/gen_golden_pose_command.py: the REAL class).  Same call shape as
``oracle.producers_oracle.VelocityCommandOracle``: ``reset_and_compute`` runs the reset of the flagged envs, then ``compute(dt)``.

``U`` is the (2, N, 7) table of samples in [0, 1): columns {time_left, pos_x, pos_y, pos_z, roll, pitch, yaw}, row 0 / 1 = the first /
second resampling of an env within one call (reset, timer).
"""

from __future__ import annotations

import torch


def quat_mul(a, b):  # utils/math.py:464-499: the eight-product form, with its association
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                        qq - zz + (z1 + y1) * (w2 - x2)], dim=-1)


def quat_conjugate(q):  # :224-235
    return torch.cat([q[..., :1], -q[..., 1:]], dim=-1)


def quat_apply(q, v):  # :545-564
    xyz = q[..., 1:]
    t = torch.cross(xyz, v, dim=-1) * 2
    return v + q[..., :1] * t + torch.cross(xyz, t, dim=-1)


def quat_from_euler_xyz(roll, pitch, yaw):  # :252-278
    cy, sy = torch.cos(yaw * 0.5), torch.sin(yaw * 0.5)
    cr, sr = torch.cos(roll * 0.5), torch.sin(roll * 0.5)
    cp, sp = torch.cos(pitch * 0.5), torch.sin(pitch * 0.5)
    return torch.stack([cy * cr * cp + sy * sr * sp, cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp,
                        sy * cr * cp - cy * sr * sp], dim=-1)


def axis_angle_from_quat(q, eps=1.0e-6):  # :646-674
    q = q * (1.0 - 2.0 * (q[..., 0:1] < 0.0))
    mag = torch.linalg.norm(q[..., 1:], dim=-1)
    half = torch.atan2(mag, q[..., 0])
    angle = 2.0 * half
    s = torch.where(angle.abs() > eps, torch.sin(half) / angle, 0.5 - angle * angle / 48)
    return q[..., 1:4] / s.unsqueeze(-1)


def pose_error_norms(t01, q01, t02, q02):
    """``torch.norm`` of both results of ``compute_pose_error(..., rot_error_type="axis_angle")`` (:820-867): the source quaternion's
    norm is ``quat_mul(q, conj q)[:, 0]`` and the conjugate is divided by it."""
    conj = quat_conjugate(q01)
    inv = conj / quat_mul(q01, conj)[..., 0:1]
    return torch.norm(t02 - t01, dim=-1), torch.norm(axis_angle_from_quat(quat_mul(q02, inv)), dim=-1)


class PoseCommandOracle:
    def __init__(self, cfg: dict, num_envs: int, step_dt: float, body_idx: int):
        self.cfg, self.N, self.step_dt, self.body_idx = cfg, num_envs, step_dt, int(body_idx)
        self.pose_command_b = torch.zeros(num_envs, 7)
        self.pose_command_b[:, 3] = 1.0
        self.pose_command_w = torch.zeros(num_envs, 7)
        self.time_left = torch.zeros(num_envs)
        self.command_counter = torch.zeros(num_envs, dtype=torch.long)
        self.metrics = {"position_error": torch.zeros(num_envs), "orientation_error": torch.zeros(num_envs)}
        self._draw = torch.zeros(num_envs, dtype=torch.long)

    @property
    def command(self):
        return self.pose_command_b

    def _u(self, U, ids, col, lo, hi):  # Tensor.uniform_(lo, hi) = u * (hi - lo) + lo in fp32
        return U[self._draw[ids], ids, col] * (hi - lo) + lo

    def _resample(self, ids, U):
        if len(ids) == 0:
            return
        c, r = self.cfg, self.cfg["ranges"]
        self.time_left[ids] = self._u(U, ids, 0, *c["resampling_time_range"])
        self.command_counter[ids] += 1
        for k, name in enumerate(("pos_x", "pos_y", "pos_z")):
            self.pose_command_b[ids, k] = self._u(U, ids, 1 + k, *r[name])
        q = quat_from_euler_xyz(self._u(U, ids, 4, *r["roll"]), self._u(U, ids, 5, *r["pitch"]), self._u(U, ids, 6, *r["yaw"]))
        if c.get("make_quat_unique", False):
            q = torch.where(q[..., 0:1] < 0, -q, q)  # quat_unique (:448-460)
        self.pose_command_b[ids, 3:] = q
        self._draw[ids] += 1

    def reset_and_compute(self, dt, root_pos_w, root_quat_w, body_pos_w, body_quat_w, reset_mask, U, do_compute=True):
        self._draw[:] = 0
        ids = reset_mask.nonzero().flatten()
        if len(ids):  # CommandTerm.reset
            for m in self.metrics.values():
                m[ids] = 0.0
            self.command_counter[ids] = 0
            self._resample(ids, U)
        if not do_compute:
            return
        # CommandTerm.compute: _update_metrics (assigned, not accumulated), the timer, the resampling; _update_command is empty
        b = self.pose_command_b
        self.pose_command_w[:, :3] = root_pos_w + quat_apply(root_quat_w, b[:, :3])
        self.pose_command_w[:, 3:] = quat_mul(root_quat_w, b[:, 3:])
        pe, re = pose_error_norms(self.pose_command_w[:, :3], self.pose_command_w[:, 3:], body_pos_w[:, self.body_idx],
                                  body_quat_w[:, self.body_idx])
        self.metrics["position_error"], self.metrics["orientation_error"] = pe, re
        self.time_left -= dt
        self._resample((self.time_left <= 0.0).nonzero().flatten(), U)
