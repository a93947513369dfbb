"""Shared by tests/test_ray_caster.py (CPU) and tests/test_ray_caster_gpu.py: the sensor cfgs, the pose sets and the fp64 / torch
restatements of what the RayCaster does around the cast (reference isaaclab/sensors/ray_caster/ray_caster.py:201-260,
sensors/sensor_base.py:182-205,287-296)."""

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATTERNS_NPZ = os.path.join(GOLDEN, "ray_caster_patterns.npz")
SENSOR_NPZ = os.path.join(GOLDEN, "ray_caster_sensor.npz")
_PAT = "isaaclab.sensors.ray_caster.patterns.patterns:"

# the four pattern cfgs of fixture (a), dict form
PATTERN_CFGS = {
    "bpearl_default": {"func": _PAT + "bpearl_pattern", "horizontal_fov": 360.0, "horizontal_res": 10.0,
                       "vertical_ray_angles": [89.5, 86.6875, 83.875, 81.0625, 78.25, 75.4375, 72.625, 69.8125, 67.0, 64.1875, 61.375, 58.5625,
                                               55.75, 52.9375, 50.125, 47.3125, 44.5, 41.6875, 38.875, 36.0625, 33.25, 30.4375, 27.625, 24.8125,
                                               22, 19.1875, 16.375, 13.5625, 10.75, 7.9375, 5.125, 2.3125]},
    # lidarfly_cfg.py:397-408: torch.linspace(0, 20, 5).tolist() and 360 / 72
    "bpearl_fork": {"func": _PAT + "bpearl_pattern", "horizontal_fov": 360.0, "horizontal_res": 360 / 72,
                    "vertical_ray_angles": torch.linspace(0.0, 20.0, 5).tolist()},
    "lidar_full": {"func": _PAT + "lidar_pattern", "channels": 4, "vertical_fov_range": (-15.0, 15.0), "horizontal_fov_range": (-180.0, 180.0),
                   "horizontal_res": 15.0},
    # 120 / 17.2 = 6.98: seven azimuths, the span no multiple of the resolution
    "lidar_partial": {"func": _PAT + "lidar_pattern", "channels": 1, "vertical_fov_range": (-10.0, -10.0), "horizontal_fov_range": (-60.0, 60.0),
                      "horizontal_res": 17.2},
}


def fork_cfg(max_distance=1.0e6, attach_yaw_only=False, **kw):
    """The lidar of the reference fork's quadcopter (lidarfly_cfg.py:397-408): 5 x 72 Bpearl rays, full orientation, 0.1 m above the base."""
    return {"pattern_cfg": PATTERN_CFGS["bpearl_fork"], "offset": {"pos": (0.0, 0.0, 0.1), "rot": (1.0, 0.0, 0.0, 0.0)},
            "attach_yaw_only": attach_yaw_only, "max_distance": max_distance, "update_period": 0.1, "drift_range": (0.0, 0.0),
            "mesh_prim_paths": ["/World/ground"], **kw}


def lidar7_cfg(max_distance=1.0e6, attach_yaw_only=False, **kw):
    return {"pattern_cfg": PATTERN_CFGS["lidar_partial"], "offset": {"pos": (0.05, 0.0, 0.2), "rot": (0.9238795, 0.0, 0.3826834, 0.0)},
            "attach_yaw_only": attach_yaw_only, "max_distance": max_distance, "update_period": 0.0, "drift_range": (0.0, 0.0), **kw}


def make_poses(N, verts, seed):
    """(N, 3) positions and (N, 4) uniformly random unit quaternions (upside-down included): x, y up to 3 m outside the mesh's extent on
    every side, z in [0.3, 3.0], the first eight envs below the surface at z in [-0.95, -0.55].  No origin on a round height."""
    rng = np.random.default_rng(seed)
    lo, hi = verts.min(0), verts.max(0)
    pos = np.stack([rng.uniform(lo[0] - 3.0, hi[0] + 3.0, N), rng.uniform(lo[1] - 3.0, hi[1] + 3.0, N), rng.uniform(0.3, 3.0, N)], 1)
    k = min(8, N)
    pos[:k, 2] = rng.uniform(-0.95, -0.55, k)
    pos[:k, :2] = np.stack([rng.uniform(lo[0] + 0.5, hi[0] - 0.5, k), rng.uniform(lo[1] + 0.5, hi[1] - 0.5, k)], 1)  # under the mesh itself
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return pos.astype(np.float32), q.astype(np.float32)


def quat_apply64(q, v):
    """quat_apply (utils/math.py:545-564) in fp64; q (..., 4), v (..., 3) broadcast."""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    xyz = np.broadcast_to(q[..., 1:], v.shape)
    t = np.cross(xyz, v) * 2
    return v + q[..., 0:1] * t + np.cross(xyz, t)


def yaw_quat64(q):
    q = np.asarray(q, np.float64)
    yaw = np.arctan2(2 * (q[..., 0] * q[..., 3] + q[..., 1] * q[..., 2]), 1 - 2 * (q[..., 2] ** 2 + q[..., 3] ** 2))
    out = np.zeros_like(q)
    out[..., 0], out[..., 3] = np.cos(yaw / 2), np.sin(yaw / 2)
    return out


def world_rays64(pos_w, quat_w, starts, dirs, yaw_only):
    """fp64 world rays (N, R, 3) x 2 of ``_update_buffers_impl`` (ray_caster.py:243-252) from the sensor pose and the local rays (R, 3)."""
    pos_w, quat_w = np.asarray(pos_w, np.float64), np.asarray(quat_w, np.float64)
    N, R = len(pos_w), len(starts)
    s = np.broadcast_to(np.asarray(starts, np.float64)[None], (N, R, 3))
    d = np.broadcast_to(np.asarray(dirs, np.float64)[None], (N, R, 3))
    if yaw_only:
        return quat_apply64(yaw_quat64(quat_w)[:, None, :], s) + pos_w[:, None, :], d.copy()
    return quat_apply64(quat_w[:, None, :], s) + pos_w[:, None, :], quat_apply64(quat_w[:, None, :], d)


# ---- the torch restatement of the sensor around the cast (fp32, the reference's ops) ------------------------------------------------
def t_quat_apply(quat, vec):
    shape = vec.shape
    quat, vec = quat.reshape(-1, 4), vec.reshape(-1, 3)
    xyz = quat[:, 1:]
    t = xyz.cross(vec, dim=-1) * 2
    return (vec + quat[:, 0:1] * t + xyz.cross(t, dim=-1)).view(shape)


def t_yaw_quat(quat):
    q = quat.clone().view(-1, 4)
    yaw = torch.atan2(2 * (q[:, 0] * q[:, 3] + q[:, 1] * q[:, 2]), 1 - 2 * (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
    out = torch.zeros_like(q)
    out[:, 3], out[:, 0] = torch.sin(yaw / 2), torch.cos(yaw / 2)
    return out / out.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)


class SensorRestatement:
    """SensorBase.reset / update / _update_outdated_buffers and RayCaster.reset / _update_buffers_impl up to the cast, in torch on the
    CPU: what the kernel's thread 0 and its ray lanes do."""

    def __init__(self, N, starts, dirs, yaw_only, update_period, drift_range):
        self.N, self.yaw_only, self.period, self.drift_range = N, yaw_only, update_period, drift_range
        self.starts, self.dirs = torch.as_tensor(starts), torch.as_tensor(dirs)  # (R, 3), offset applied
        self.timestamp, self.last = torch.zeros(N), torch.zeros(N)
        self.outdated = torch.ones(N, dtype=torch.bool)
        self.drift = torch.zeros(N, 3)
        self.pos_w, self.quat_w = torch.zeros(N, 3), torch.zeros(N, 4)
        R = len(self.starts)
        self.starts_w, self.dirs_w = torch.zeros(N, R, 3), torch.zeros(N, R, 3)

    def reset(self, ids, uniforms):
        self.timestamp[ids] = 0.0
        self.last[ids] = 0.0
        self.outdated[ids] = True
        lo, hi = self.drift_range
        self.drift[ids] = uniforms[ids] * (hi - lo) + lo

    def update(self, dt):
        self.timestamp += dt
        self.outdated |= self.timestamp - self.last + 1e-6 >= self.period

    def refresh(self, pos, quat):
        ids = self.outdated.nonzero().squeeze(-1)
        if len(ids) == 0:
            return ids
        R = len(self.starts)
        p = pos[ids].clone() + self.drift[ids]
        q = quat[ids].clone()
        self.pos_w[ids], self.quat_w[ids] = p, q
        s, d = self.starts.repeat(len(ids), 1, 1), self.dirs.repeat(len(ids), 1, 1)
        if self.yaw_only:
            sw = t_quat_apply(t_yaw_quat(q.repeat(1, R)), s)
            dw = d
        else:
            sw = t_quat_apply(q.repeat(1, R), s)
            dw = t_quat_apply(q.repeat(1, R), d)
        sw = sw + p.unsqueeze(1)
        self.starts_w[ids], self.dirs_w[ids] = sw, dw
        self.last[ids] = self.timestamp[ids]
        self.outdated[ids] = False
        return ids
