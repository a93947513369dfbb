"""TEST INFRASTRUCTURE -- a plain torch restatement of ``CommandTerm.reset`` / ``compute`` + ``UniformPose2dCommand`` /
``TerrainBasedPose2dCommand`` (isaaclab/managers/command_manager.py:120-187, isaaclab/envs/mdp/commands/pose_2d_command.py), fp32 or, on
request, fp64.  Draws come from a (2, N, 4) table {time_left, pos_x, pos_y, heading} and, for the terrain-based class, a (2, N) table of
patch ids: row 0 = the env's first resampling of a call, row 1 = its second (reset, then timer)."""

from __future__ import annotations

import math

import torch


def wrap_to_pi(a: torch.Tensor) -> torch.Tensor:
    """utils/math.py:95-117"""
    w = (a + math.pi) % (2 * math.pi)
    return torch.where((w == 0) & (a > 0), torch.full_like(a, math.pi), w - math.pi)


def quat_apply(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """utils/math.py:545-564"""
    xyz = q[:, 1:]
    t = torch.cross(xyz, v, dim=-1) * 2
    return v + q[:, 0:1] * t + torch.cross(xyz, t, dim=-1)


def heading_w(q: torch.Tensor) -> torch.Tensor:
    """ArticulationData.heading_w (articulation_data.py:518-526)"""
    f = quat_apply(q, torch.tensor([1.0, 0.0, 0.0], dtype=q.dtype).repeat(q.shape[0], 1))
    return torch.atan2(f[:, 1], f[:, 0])


def yaw_quat(q: torch.Tensor) -> torch.Tensor:
    """utils/math.py:521-542"""
    w, x, y, z = q.unbind(-1)
    yaw = torch.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    out = torch.zeros_like(q)
    out[:, 0], out[:, 3] = torch.cos(yaw / 2), torch.sin(yaw / 2)
    return out / out.norm(dim=-1, keepdim=True).clamp(min=1e-9)


def quat_rotate_inverse(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """utils/math.py:605-625"""
    w, vec = q[:, 0:1], q[:, 1:]
    a = v * (2.0 * w**2 - 1.0)
    b = torch.cross(vec, v, dim=-1) * w * 2.0
    c = vec * (vec * v).sum(-1, keepdim=True) * 2.0
    return a - b + c


class Pose2dOracle:
    """``cfg``: dict with ``resampling_time_range``, ``simple_heading``, ``ranges`` {pos_x, pos_y, heading}; ``kind`` 1 = terrain based
    (``valid_targets`` (L, T, P, 3), ``terrain_levels`` / ``terrain_types`` (N))."""

    def __init__(self, cfg: dict, N: int, env_origins, default_root_z, kind: int = 0, valid_targets=None, terrain_levels=None,
                 terrain_types=None, dtype=torch.float32):
        self.cfg, self.N, self.kind, self.dtype = cfg, N, kind, dtype
        c = lambda x: None if x is None else torch.as_tensor(x).to(dtype)  # noqa: E731
        self.env_origins, self.default_root_z, self.valid_targets = c(env_origins), c(default_root_z), c(valid_targets)
        self.terrain_levels, self.terrain_types = terrain_levels, terrain_types
        self.pos_command_w, self.heading_command_w = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype)
        self.pos_command_b, self.heading_command_b = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype)
        self.time_left, self.command_counter = torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=torch.long)
        self.metrics = {"error_pos": torch.zeros(N, dtype=dtype), "error_heading": torch.zeros(N, dtype=dtype)}
        self._draw = torch.zeros(N, dtype=torch.long)

    @property
    def command(self):
        return torch.cat([self.pos_command_b, self.heading_command_b.unsqueeze(1)], dim=1)

    def _u(self, ids, col, rng):
        return self._U[self._draw[ids], ids, col] * (rng[1] - rng[0]) + rng[0]

    def _resample(self, ids):
        if len(ids) == 0:
            return
        r = self.cfg["ranges"]
        self.time_left[ids] = self._u(ids, 0, self.cfg["resampling_time_range"])
        if self.kind == 1:
            pid = self._patch_ids[self._draw[ids], ids]
            self.pos_command_w[ids] = self.valid_targets[self.terrain_levels[ids], self.terrain_types[ids], pid]
            self.pos_command_w[ids, 2] += self.default_root_z[ids]
        else:
            self.pos_command_w[ids] = self.env_origins[ids]
            self.pos_command_w[ids, 0] += self._u(ids, 1, r["pos_x"])
            self.pos_command_w[ids, 1] += self._u(ids, 2, r["pos_y"])
            self.pos_command_w[ids, 2] += self.default_root_z[ids]
        if self.cfg["simple_heading"]:
            tv = self.pos_command_w[ids] - self._root_pos[ids]
            td = torch.atan2(tv[:, 1], tv[:, 0])
            flipped = wrap_to_pi(td + math.pi)
            to_t, to_f = wrap_to_pi(td - self._heading[ids]).abs(), wrap_to_pi(flipped - self._heading[ids]).abs()
            self.heading_command_w[ids] = torch.where(to_t < to_f, td, flipped)
        else:
            self.heading_command_w[ids] = self._u(ids, 3, r["heading"])
        self.command_counter[ids] += 1
        self._draw[ids] += 1

    def reset_and_compute(self, dt: float, root_pos_w, root_quat_w, reset_mask, uniforms, patch_ids=None, do_compute: bool = True):
        """``reset(ids of reset_mask)`` returns what CommandTerm.reset logs (the means of the metrics over the reset envs) or {}."""
        self._root_pos, self._root_quat = root_pos_w.to(self.dtype), root_quat_w.to(self.dtype)
        self._heading = heading_w(self._root_quat)
        self._U, self._patch_ids = uniforms.to(self.dtype), patch_ids
        self._draw[:] = 0
        log = {}
        ids = reset_mask.nonzero().flatten()
        if len(ids):
            for k, v in self.metrics.items():
                log[k] = float(v[ids].mean())
                v[ids] = 0.0
            self.command_counter[ids] = 0
            self._resample(ids)
        if do_compute:
            self.metrics["error_pos_2d"] = torch.norm(self.pos_command_w[:, :2] - self._root_pos[:, :2], dim=1)
            self.metrics["error_heading"] = torch.abs(wrap_to_pi(self.heading_command_w - self._heading))
            self.time_left -= dt
            self._resample((self.time_left <= 0.0).nonzero().flatten())
            self.pos_command_b[:] = quat_rotate_inverse(yaw_quat(self._root_quat), self.pos_command_w - self._root_pos)
            self.heading_command_b[:] = wrap_to_pi(self.heading_command_w - self._heading)
        return log
