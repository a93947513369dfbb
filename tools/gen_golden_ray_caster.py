"""TEST INFRASTRUCTURE (build container only): the fixtures of the RayCaster sensor, from the REAL reference.

    python tools/gen_golden_ray_caster.py

Writes
  * ``tests/golden/ray_caster_patterns.npz``: the reference's ``bpearl_pattern`` / ``lidar_pattern`` for the four cfgs of
    ``tests/_ray_caster_cases.py:PATTERN_CFGS`` (Bpearl defaults, the fork's 5 angles at ``horizontal_res = 5``, a lidar with a full 360
    degree range, a lidar whose span is no multiple of its resolution): ``<name>/starts``, ``<name>/dirs``.
  * ``tests/golden/ray_caster_sensor.npz``: the real ``RayCaster._update_buffers_impl``, ``RayCaster.reset`` and ``SensorBase.update`` on
    an instance made without ``__init__``.  The module's ``XFormPrim`` is replaced by a small class that returns recorded poses (the
    stubbed name is a mock and fails ``isinstance``), ``raycast_mesh`` by a recorder of the world rays, ``Tensor.uniform_`` by a table of
    recorded draws.  N = 8 poses, both attach modes, a rotated offset and non-zero drift: ``full/...`` and ``yaw/...``; the flags and
    clocks over 12 updates of dt = 0.02 at update_period = 0.1 with ``data`` asked after each and a partial reset after the seventh:
    ``clock/...``.
Deterministic: a second run reproduces the files bit for bit."""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden as gg  # noqa: E402,F401  (installs oracle.ref_import)

import importlib  # noqa: E402

rc_mod = importlib.import_module("isaaclab.sensors.ray_caster.ray_caster")  # (the package re-exports names that shadow its modules)
ref_patterns = importlib.import_module("isaaclab.sensors.ray_caster.patterns.patterns")
from isaaclab.sensors.sensor_base import SensorBase  # noqa: E402

from _ray_caster_cases import PATTERN_CFGS, PATTERNS_NPZ, SENSOR_NPZ  # noqa: E402

N = 8
OFFSET_POS = (0.05, -0.02, 0.1)
OFFSET_ROT = (0.9238795, 0.0, 0.3826834, 0.0)  # 45 degrees about y
DRIFT_RANGE = (-0.05, 0.15)


def pattern_fixture():
    out = {}
    for name, cfg in PATTERN_CFGS.items():
        c = types.SimpleNamespace(**{k: v for k, v in cfg.items() if k != "func"})
        fn = getattr(ref_patterns, cfg["func"].rsplit(":", 1)[1])
        starts, dirs = fn(c, "cpu")
        out[f"{name}/starts"], out[f"{name}/dirs"] = starts.numpy(), dirs.numpy()
        print(name, tuple(dirs.shape))
    np.savez(PATTERNS_NPZ, **out)


class RecordedPoses:
    """Stands in for ``XFormPrim``: ``get_world_poses(env_ids)`` of recorded poses."""

    def __init__(self, pos, quat):
        self.pos, self.quat, self.count = pos, quat, len(pos)

    def get_world_poses(self, env_ids):
        return self.pos[env_ids], self.quat[env_ids]


def make_sensor(pos, quat, yaw_only, update_period, pattern):
    s = rc_mod.RayCaster.__new__(rc_mod.RayCaster)
    pc = types.SimpleNamespace(**{k: v for k, v in PATTERN_CFGS[pattern].items() if k != "func"})
    pc.func = getattr(ref_patterns, PATTERN_CFGS[pattern]["func"].rsplit(":", 1)[1])
    s.cfg = types.SimpleNamespace(pattern_cfg=pc, offset=types.SimpleNamespace(pos=OFFSET_POS, rot=OFFSET_ROT), attach_yaw_only=yaw_only,
                                  max_distance=1.0e6, drift_range=DRIFT_RANGE, update_period=update_period, mesh_prim_paths=["/World/ground"],
                                  history_length=0)
    s._device, s._is_visualizing = "cpu", False
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # (SensorBase.__del__ reads them)
    s._view = RecordedPoses(pos, quat)
    s._data = types.SimpleNamespace()
    s.meshes = {"/World/ground": None}
    n = len(pos)
    s._num_envs = n
    s._is_outdated = torch.ones(n, dtype=torch.bool)  # SensorBase._initialize_impl (sensor_base.py:226-231)
    s._timestamp = torch.zeros(n)
    s._timestamp_last_update = torch.zeros(n)
    s._initialize_rays_impl()
    return s


def sensor_fixture():
    g = torch.Generator().manual_seed(20)
    pos = torch.stack([torch.rand(N, generator=g) * 8 - 4, torch.rand(N, generator=g) * 10 - 5, torch.rand(N, generator=g) * 2.5 + 0.4], 1)
    quat = torch.randn(N, 4, generator=g)
    quat = quat / quat.norm(dim=1, keepdim=True)
    uniforms0 = torch.rand(N, 3, generator=g)
    out = {"pos": pos.numpy(), "quat": quat.numpy(), "uniforms0": uniforms0.numpy(), "offset_pos": np.asarray(OFFSET_POS, np.float32),
           "offset_rot": np.asarray(OFFSET_ROT, np.float32), "drift_range": np.asarray(DRIFT_RANGE, np.float32)}
    recorded = {}

    def fake_raycast_mesh(ray_starts, ray_directions, max_dist=1e6, mesh=None, **kw):
        recorded["starts"], recorded["dirs"] = ray_starts.clone(), ray_directions.clone()
        return (torch.zeros_like(ray_starts),)

    table = {}

    def fake_uniform(self, lo=0.0, hi=1.0):
        self.copy_(table["u"] * (hi - lo) + lo)
        return self

    real = (rc_mod.XFormPrim, rc_mod.raycast_mesh, torch.Tensor.uniform_)
    rc_mod.XFormPrim, rc_mod.raycast_mesh, torch.Tensor.uniform_ = RecordedPoses, fake_raycast_mesh, fake_uniform
    try:
        for mode, yaw_only in (("full", False), ("yaw", True)):
            s = make_sensor(pos, quat, yaw_only, 0.1, "bpearl_fork")
            table["u"] = uniforms0
            s.reset()  # the real RayCaster.reset -> SensorBase.reset, drift.uniform_(*drift_range)
            SensorBase.update(s, 0.02, force_recompute=True)
            assert tuple(recorded["starts"].shape) == (N, 360, 3) and float(s.drift.abs().min()) > 0.0
            out[f"{mode}/ray_starts_w"], out[f"{mode}/ray_directions_w"] = recorded["starts"].numpy(), recorded["dirs"].numpy()
            out[f"{mode}/pos_w"], out[f"{mode}/drift"] = s._data.pos_w.numpy().copy(), s.drift.numpy().copy()
        # the clocks
        s = make_sensor(pos, quat, False, 0.1, "bpearl_fork")
        reset_ids = [1, 2, 5]
        before, ts, last = [], [], []
        for k in range(12):
            SensorBase.update(s, 0.02)
            before.append(s._is_outdated.numpy().copy())
            s.data  # RayCaster.data -> _update_outdated_buffers
            ts.append(s._timestamp.numpy().copy())
            last.append(s._timestamp_last_update.numpy().copy())
            assert not bool(s._is_outdated.any())
            if k == 6:
                table["u"] = torch.zeros(len(reset_ids), 3)
                s.reset(reset_ids)
                out["clock/outdated_after_reset"] = s._is_outdated.numpy().copy()
        out["clock/outdated_before"], out["clock/timestamp"], out["clock/last_update"] = np.stack(before), np.stack(ts), np.stack(last)
        out["clock/reset_ids"] = np.asarray(reset_ids, np.int64)
        print("refreshes per update:", [int(b.sum()) for b in before])
    finally:
        rc_mod.XFormPrim, rc_mod.raycast_mesh, torch.Tensor.uniform_ = real
    np.savez(SENSOR_NPZ, **out)


if __name__ == "__main__":
    pattern_fixture()
    sensor_fixture()
    for p in (PATTERNS_NPZ, SENSOR_NPZ):
        print(p, os.path.getsize(p), "bytes")
