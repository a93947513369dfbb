"""The RayCaster sensor without a GPU: the Bpearl / lidar patterns against the reference's (tests/golden/ray_caster_patterns.npz), the torch
restatement of the pose composition and the clock logic against the REAL ``RayCaster`` / ``SensorBase`` (tests/golden/ray_caster_sensor.npz,
both from tools/gen_golden_ray_caster.py), the cfg forms, the refusals, the C interface and its ctypes mirror."""

import ctypes
import subprocess
import types

import numpy as np
import pytest
import torch

from _diff_ik_cases import ROOT, host_compiler
from _ray_caster_cases import PATTERN_CFGS, PATTERNS_NPZ, SENSOR_NPZ, SensorRestatement, fork_cfg
from isaaclab_amd import _abi, _lib, plan, producers

ULP2 = 2.4e-7  # 2 ulp of fp32 at 1: the components of a unit vector


def as_object(cfg: dict):
    return types.SimpleNamespace(**{k: (as_object(v) if isinstance(v, dict) and k in ("pattern_cfg", "offset") else v) for k, v in cfg.items()})


@pytest.mark.parametrize("name", list(PATTERN_CFGS))
def test_patterns_match_the_reference(name):
    z = np.load(PATTERNS_NPZ)
    starts, dirs = plan.ray_pattern(PATTERN_CFGS[name])
    want = z[f"{name}/dirs"]
    assert dirs.dtype == np.float32 and dirs.shape == want.shape == {"bpearl_default": (32 * 36, 3), "bpearl_fork": (360, 3), "lidar_full": (4 * 23, 3),
                                                                      "lidar_partial": (7, 3)}[name]
    assert np.abs(dirs - want).max() <= ULP2  # count and order exact (same shape, every ray within 2 ulp of its own)
    assert np.array_equal(starts, z[f"{name}/starts"]) and not starts.any()
    assert np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_pattern_order_keeps_neighbouring_rays_together():
    _, d = plan.ray_pattern(PATTERN_CFGS["bpearl_fork"])
    az = np.degrees(np.arctan2(d[:, 1].astype(np.float64), d[:, 0]))
    assert np.allclose(az[:5], az[0], atol=1e-4) and abs(((az[5] - az[0] + 180) % 360 - 180) - 5.0) < 1e-3  # the 5 rings of one azimuth, then the next azimuth
    assert (d[:, 2] >= -1e-7).all()  # the fork's rings 0..20 degrees point level or up in the sensor frame
    _, d = plan.ray_pattern(PATTERN_CFGS["lidar_full"])
    assert len(d) == 4 * (24 - 1)  # ceil(360 / 15) = 24 azimuths, the last one (= the first) dropped
    assert np.allclose(d[:23, 2], d[0, 2])  # one channel's azimuths are consecutive


def test_dict_and_object_forms_give_the_same_pattern():
    for name, cfg in PATTERN_CFGS.items():
        a, b = plan.ray_pattern(cfg), plan.ray_pattern(as_object(cfg))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
    def bpearl_pattern(cfg, device):  # a callable `func`, as a cfg object carries it
        raise AssertionError("never called: the pattern is restated")

    bpearl_pattern.__module__ = "isaaclab.sensors.ray_caster.patterns.patterns"
    obj = as_object(dict(PATTERN_CFGS["bpearl_fork"], func=bpearl_pattern))
    assert np.array_equal(plan.ray_pattern(obj)[1], plan.ray_pattern(PATTERN_CFGS["bpearl_fork"])[1])
    # the sensor cfg, too: same rays with the offset applied
    a = producers.RayCaster(fork_cfg(), 4, "cpu", mesh=object())
    b = producers.RayCaster(as_object(fork_cfg()), 4, "cpu", mesh=object())
    assert a.num_rays == b.num_rays == 360 and torch.equal(a.ray_starts, b.ray_starts) and torch.equal(a.ray_directions, b.ray_directions)
    assert torch.equal(a.ray_starts, torch.tensor([0.0, 0.0, 0.1]).repeat(360, 1)) and a.cfg.update_period == 0.1 and not a.cfg.attach_yaw_only
    assert bool(a._is_outdated.all()) and tuple(a._data.ray_hits_w.shape) == (4, 360, 3)


def test_refusals():
    pin = {"func": "isaaclab.sensors.ray_caster.patterns.patterns:pinhole_camera_pattern", "width": 4, "height": 4}
    with pytest.raises(NotImplementedError, match="pinhole_camera_pattern.*camera sensors.*out of scope"):
        plan.ray_pattern(pin)
    with pytest.raises(NotImplementedError, match="pinhole_camera_pattern"):
        producers.RayCaster(dict(fork_cfg(), pattern_cfg=pin), 4, "cpu", mesh=object())
    with pytest.raises(NotImplementedError, match="only supports one mesh prim. Received: 2"):
        producers.RayCaster(fork_cfg(mesh_prim_paths=["/World/ground", "/World/walls"]), 4, "cpu", mesh=object())
    with pytest.raises(NotImplementedError, match="no mesh .a plane."):
        producers.RayCaster(fork_cfg(), 4, "cpu", mesh=None)
    with pytest.raises(NotImplementedError, match="'spiral_pattern' is not known"):
        plan.ray_pattern({"func": "somewhere:spiral_pattern"})
    with pytest.raises(ValueError, match="'channels' is missing"):
        plan.ray_pattern({"func": "p:lidar_pattern", "vertical_fov_range": (0, 1), "horizontal_fov_range": (0, 90), "horizontal_res": 1.0})
    with pytest.raises(RuntimeError, match="no body pose yet"):
        producers.RayCaster(fork_cfg(), 4, "cpu", mesh=object()).data
    # the height-scan path keeps its grid_pattern-only refusal
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.robots import ROBOTS
    import copy

    fx = copy.deepcopy(load_task_cfg("Isaac-Velocity-Rough-Anymal-C-v0"))
    fx["env"]["scene"]["height_scanner"]["pattern_cfg"] = PATTERN_CFGS["bpearl_fork"]
    with pytest.raises(NotImplementedError, match="only grid_pattern ray patterns are on the fused path"):
        plan.compile_plan(fx["env"], ROBOTS[fx["robot"]])


@pytest.mark.parametrize("mode,yaw_only", [("full", False), ("yaw", True)])
def test_restated_pose_composition_matches_the_real_sensor(mode, yaw_only):
    z = np.load(SENSOR_NPZ)
    cfg = fork_cfg(1.0e6, yaw_only, offset={"pos": tuple(z["offset_pos"]), "rot": tuple(z["offset_rot"])}, drift_range=tuple(z["drift_range"]))
    prod = producers.RayCaster(cfg, len(z["pos"]), "cpu", mesh=object())  # the host side of the producer: pattern + offset
    r = SensorRestatement(len(z["pos"]), prod.ray_starts, prod.ray_directions, yaw_only, 0.1, tuple(float(x) for x in z["drift_range"]))
    r.reset(slice(None), torch.from_numpy(z["uniforms0"]))
    r.update(0.02)
    ids = r.refresh(torch.from_numpy(z["pos"]), torch.from_numpy(z["quat"]))
    assert len(ids) == len(z["pos"])
    assert np.array_equal(r.drift.numpy(), z[f"{mode}/drift"]) and np.array_equal(r.pos_w.numpy(), z[f"{mode}/pos_w"])
    assert np.abs(r.starts_w.numpy() - z[f"{mode}/ray_starts_w"]).max() <= 1e-6
    assert np.abs(r.dirs_w.numpy() - z[f"{mode}/ray_directions_w"]).max() <= 1e-6
    if yaw_only:  # the directions are the offset-rotated pattern itself
        assert np.array_equal(z["yaw/ray_directions_w"][3], prod.ray_directions.numpy())


def test_restated_clock_logic_matches_the_real_sensor_bit_for_bit():
    z = np.load(SENSOR_NPZ)
    N = len(z["pos"])
    prod = producers.RayCaster(fork_cfg(), N, "cpu", mesh=object())
    r = SensorRestatement(N, prod.ray_starts, prod.ray_directions, False, 0.1, (0.0, 0.0))
    pos, quat = torch.from_numpy(z["pos"]), torch.from_numpy(z["quat"])
    refreshes = []
    for k in range(12):
        r.update(0.02)
        assert np.array_equal(r.outdated.numpy(), z["clock/outdated_before"][k]), k
        refreshes.append(len(r.refresh(pos, quat)))
        assert np.array_equal(r.timestamp.numpy().view(np.uint32), z["clock/timestamp"][k].view(np.uint32)), k
        assert np.array_equal(r.last.numpy().view(np.uint32), z["clock/last_update"][k].view(np.uint32)), k
        if k == 6:
            r.reset(torch.from_numpy(z["clock/reset_ids"]), torch.zeros(N, 3))
            assert np.array_equal(r.outdated.numpy(), z["clock/outdated_after_reset"])
    assert refreshes == [N, 0, 0, 0, 0, N, 0, 3, 0, 0, N - 3, 0]


def test_c_interface_and_its_mirror(libimx):
    h = open(f"{ROOT}/include/imx.h").read()
    assert '#include "imx_ray_caster_struct.h"' in h and "typedef struct imx_ray_caster imx_ray_caster_t;" in h
    for fn in ("imx_ray_caster", "imx_mesh_build_ray_bounds"):
        assert fn in _lib.EXPORTS and hasattr(libimx, fn)
    res, args = _lib._SIGNATURES["imx_ray_caster"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.ImxRayCaster), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert int(libimx.imx_struct_size(25)) == ctypes.sizeof(_lib.ImxRayCaster) > 0
    assert all(int(libimx.imx_struct_size(k)) == 0 for k in (9, 14, 17, 19, 21, 24, 26))
    # imx.h's own struct count stays: the struct lives in its own header
    assert list(_abi.RAY_CASTER_STRUCTS) == ["imx_ray_caster_t"] and "imx_ray_caster_t" not in _abi.STRUCTS and len(_abi.STRUCTS) == 8
    assert [f for f, _ in _lib.ImxRayCaster._fields_] == [f for f, _ in _abi.RAY_CASTER_STRUCTS["imx_ray_caster_t"]]
    assert _lib.ImxRayCaster.seed.offset == 40 and _lib.ImxRayCaster.ray_starts_d.offset == 48
    # refused before any launch, by name (no GPU is needed for that)
    c = _lib.ImxRayCaster(num_rays=0)
    assert libimx.imx_ray_caster(ctypes.byref(c), 4, ctypes.c_void_p(1), None) != 0 and b"num_rays" in libimx.imx_last_error()
    assert libimx.imx_ray_caster(None, 4, None, None) != 0 and b"null argument" in libimx.imx_last_error()


def test_struct_layout_against_a_compiler(tmp_path):
    """sizeof / offsetof of every field of imx_ray_caster_t as a C++ compiler lays it out (the recipe of tests/test_abi.py)."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    cls = _lib.ImxRayCaster
    lines = ['#include <cstddef>', '#include "imx.h"', f'static_assert(sizeof(imx_ray_caster_t) == {ctypes.sizeof(cls)}, "size");']
    for field, _ in cls._fields_:
        f = getattr(cls, field)
        lines.append(f'static_assert(offsetof(imx_ray_caster_t, {field}) == {f.offset} && sizeof(imx_ray_caster_t::{field}) == {f.size}, "{field}");')
    src = tmp_path / "rc_abi.cpp"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # ... and the check bites: a shifted field must not compile
    src.write_text("\n".join(lines).replace(f"offsetof(imx_ray_caster_t, seed) == {cls.seed.offset}", f"offsetof(imx_ray_caster_t, seed) == {cls.seed.offset + 4}") + "\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", f"{ROOT}/include", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "seed" in r.stderr
