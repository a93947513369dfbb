"""CPU restatement, in fp32 torch, of the five manipulation/inhand/mdp terms the Repose-Cube task uses and of its command term
(``CommandTerm.reset`` / ``compute`` with ``InHandReOrientationCommand``), written from the reference's formulas: what
tests/test_inhand_oracle.py holds against the fixtures recorded from the real classes, and what the GPU tests hold the kernels against at
sizes the fixtures do not have."""

from __future__ import annotations

import math

import torch

F = torch.float32


def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The Hamilton product, quaternions w, x, y, z."""
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def quat_conj(q: torch.Tensor) -> torch.Tensor:
    return torch.cat([q[..., :1], -q[..., 1:]], dim=-1)


def quat_unique(q: torch.Tensor) -> torch.Tensor:
    return torch.where(q[..., 0:1] < 0, -q, q)


def quat_error_magnitude(q1: torch.Tensor, q2: torch.Tensor) -> torch.Tensor:
    """The norm of the axis-angle vector of q1 * conj(q2): the quaternion flipped to w >= 0, angle = 2 atan2(||xyz||, w), the vector
    xyz / (sin(angle / 2) / angle) with the small-angle series 1/2 - angle^2 / 48 below 1e-6."""
    d = quat_mul(q1, quat_conj(q2))
    d = d * (1.0 - 2.0 * (d[..., 0:1] < 0.0).to(d.dtype))
    mag = d[..., 1:].norm(dim=-1)
    half = torch.atan2(mag, d[..., 0])
    angle = 2.0 * half
    k = torch.where(angle.abs() > 1.0e-6, torch.sin(half) / angle, 0.5 - angle * angle / 48.0)
    return (d[..., 1:] / k.unsqueeze(-1)).norm(dim=-1)


def terms(s: dict, threshold: float, rot_eps: float, num_success: float, reach: float) -> dict:
    """The task's two in-hand rewards (raw values), its two in-hand terminations, and its object / goal observation terms (before
    noise and scale) from the fp32 feed tensors ``s``."""
    oq, goal = s["object_root_quat_w"].to(F), s["command"][:, 3:7].to(F)
    dth = quat_error_magnitude(oq, goal)
    return {"dtheta": dth, "track_orientation_inv_l2": 1.0 / (dth + rot_eps), "success_bonus": (dth <= threshold).to(F),
            "track_pos_l2": (s["command"][:, :3] - (s["object_root_pos_w"] - s["env_origins"])).norm(dim=-1),
            "max_consecutive_success": s["command_consecutive_success"] >= num_success,
            "object_out_of_reach": (s["root_pos_w"] - s["object_root_pos_w"]).norm(dim=-1) > reach,
            "object_pos": s["object_root_pos_w"] - s["env_origins"], "object_quat": oq, "object_lin_vel": s["object_root_lin_vel_w"],
            "object_ang_vel": s["object_root_ang_vel_w"], "goal_pose": s["command"], "goal_quat_diff": quat_mul(oq, quat_conj(goal))}


def quat_about(angle: torch.Tensor, axis: int) -> torch.Tensor:
    """quat_from_angle_axis about unit axis X (0) or Y (1): (cos, axis sin) of the half angle, normalised."""
    h = angle / 2.0
    q = torch.zeros(angle.shape[0], 4, dtype=angle.dtype)
    q[:, 0], q[:, 1 + axis] = torch.cos(h), torch.sin(h)
    return q / q.norm(dim=-1, keepdim=True).clamp(min=1.0e-9)


class CommandOracle:
    """``InHandReOrientationCommand`` under ``CommandTerm.reset`` / ``compute``; every draw comes from ``U`` (3, N, 3): [which resampling
    of the env within the call, env, {time_left, rand 0, rand 1}]."""

    def __init__(self, cfg: dict, N: int, pos_command_e: torch.Tensor, pos_command_w: torch.Tensor):
        self.N, self.cfg = N, cfg
        self.pos_command_e, self.pos_command_w = pos_command_e.to(F).clone(), pos_command_w.to(F).clone()
        self.quat_command_w = torch.zeros(N, 4)
        self.quat_command_w[:, 0] = 1.0
        self.time_left = torch.zeros(N)
        self.command_counter = torch.zeros(N, dtype=torch.long)
        self.metrics = {k: torch.zeros(N) for k in ("orientation_error", "position_error", "consecutive_success")}
        self.draw = torch.zeros(N, dtype=torch.long)

    @property
    def command(self) -> torch.Tensor:
        return torch.cat([self.pos_command_e, self.quat_command_w], dim=-1)

    def _resample(self, ids: torch.Tensor, U: torch.Tensor) -> None:
        if len(ids) == 0:
            return
        u = U[self.draw[ids], ids]
        lo, hi = self.cfg["resampling_time_range"]
        self.time_left[ids] = u[:, 0] * (hi - lo) + lo
        self.command_counter[ids] += 1
        r = 2.0 * u[:, 1:3] - 1.0
        q = quat_mul(quat_about(r[:, 0] * math.pi, 0), quat_about(r[:, 1] * math.pi, 1))
        self.quat_command_w[ids] = quat_unique(q) if self.cfg["make_quat_unique"] else q
        self.draw[ids] += 1

    def call(self, dt: float, do_compute: bool, reset_mask: torch.Tensor, U: torch.Tensor, obj_pos=None, obj_quat=None) -> dict:
        """One launch's worth: reset on the mask, then (``do_compute``) compute(dt).  Returns the means CommandTerm.reset logs."""
        self.draw[:] = 0
        ids = reset_mask.nonzero().flatten()
        log = {}
        if len(ids):
            for k, v in self.metrics.items():
                log[k] = float(v[ids].mean())
                v[ids] = 0.0
            self.command_counter[ids] = 0
            self._resample(ids, U)
        if do_compute:
            err = quat_error_magnitude(obj_quat.to(F), self.quat_command_w)
            self.metrics["orientation_error"] = err
            self.metrics["position_error"] = (obj_pos - self.pos_command_w).norm(dim=-1)
            reached = err < self.cfg["orientation_success_threshold"]
            self.metrics["consecutive_success"] = self.metrics["consecutive_success"] + reached.to(F)
            self.time_left = self.time_left - dt
            self._resample((self.time_left <= 0.0).nonzero().flatten(), U)
            if self.cfg["update_goal_on_success"]:
                self._resample(reached.nonzero().flatten(), U)
        return log
