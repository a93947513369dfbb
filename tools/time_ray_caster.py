"""Time the lidar of the reference fork's quadcopter two ways, on the bench terrain at 4096 envs.

    python tools/time_ray_caster.py [--envs 4096] [--launches 200] [--rounds 5] [--out profiles/ray_caster_timing.txt]

  (a) the way the tree had before the sensor existed: the world rays composed in torch (quat_apply on (N, R, 3) starts and directions,
      plus pos_w) and ``TerrainMesh.raycast`` -- the 2-D walk without pruning in z;
  (b) the one launch of ``producers.RayCaster`` (``imx_ray_caster``: pose, world rays, the z-pruned walk).
Poses 0.5 - 3 m above the terrain's base plane with roll / pitch ~ N(0, 0.3 rad) and uniform yaw, all envs outdated at every launch, the
fork's 5 x 72 Bpearl pattern, ``max_distance`` 1e6 and 10.  The outputs are compared bit for bit first.  HIP events around ``launches``
back-to-back launches after a warm-up, ``rounds`` alternated rounds; per setting both series, their spread, the ratio of medians, and the
bounds' build time and bytes."""

from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaaclab_amd.env import TerrainMesh  # noqa: E402
from isaaclab_amd.producers import RayCaster  # noqa: E402
from isaaclab_amd.terrain import make_rough_terrain  # noqa: E402

PATTERN = {"func": "isaaclab.sensors.ray_caster.patterns.patterns:bpearl_pattern", "horizontal_fov": 360.0, "horizontal_res": 5.0,
           "vertical_ray_angles": [0.0, 5.0, 10.0, 15.0, 20.0]}


def quat_apply(quat, vec):  # isaaclab/utils/math.py:545-564
    shape = vec.shape
    quat, vec = quat.reshape(-1, 4), vec.reshape(-1, 3)
    xyz = quat[:, 1:]
    t = xyz.cross(vec, dim=-1) * 2
    return (vec + quat[:, 0:1] * t + xyz.cross(t, dim=-1)).view(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, dev = a.envs, torch.device("cuda:0")
    v, t, ext = make_rough_terrain()
    mesh = TerrainMesh(v, t, 0.0)
    g = torch.Generator().manual_seed(1)
    pos = torch.stack([(torch.rand(N, generator=g) * 2 - 1) * (ext[0] - 2.0), (torch.rand(N, generator=g) * 2 - 1) * (ext[1] - 2.0),
                       torch.rand(N, generator=g) * 2.5 + 0.5], 1)
    roll, pitch, yaw = torch.randn(N, generator=g) * 0.3, torch.randn(N, generator=g) * 0.3, (torch.rand(N, generator=g) * 2 - 1) * math.pi
    cr, sr, cp, sp, cy, sy = (f(x * 0.5) for x in (roll, pitch, yaw) for f in (torch.cos, torch.sin))
    quat = torch.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
    pos, quat = pos.to(dev).contiguous(), quat.to(dev).contiguous()
    lines = [f"mesh: {len(t)} triangles, grid {mesh.nx} x {mesh.ny} cells of {mesh.cell_size:.4f} m; {N} envs x 360 rays; "
             f"{a.launches} launches per sample, {a.rounds} alternated rounds; device {torch.cuda.get_device_name(0)}"]
    first_info = None
    for max_distance in (1.0e6, 10.0):
        cfg = {"pattern_cfg": PATTERN, "offset": {"pos": (0.0, 0.0, 0.1)}, "attach_yaw_only": False, "max_distance": max_distance, "update_period": 0.0}
        s = RayCaster(cfg, N, dev, mesh)
        first_info = first_info or s.bounds_info
        R = s.num_rays
        starts, dirs = s.ray_starts.repeat(N, 1, 1), s.ray_directions.repeat(N, 1, 1)

        def old():
            sw = quat_apply(quat.repeat(1, R), starts)
            sw += pos.unsqueeze(1)
            dw = quat_apply(quat.repeat(1, R), dirs)
            return mesh.raycast(sw, dw, max_distance)[0]

        def new():
            s.update(0.02, pos, quat, force_recompute=True)  # update_period 0: every env is outdated at every update
            return s._data.ray_hits_w

        # first: same outputs.  The walk on the launch's own world rays against TerrainMesh.raycast on those rays (must be bit-identical),
        # then (a) against (b) end to end (they differ where torch's composition rounds a ray differently from the kernel's)
        chk = RayCaster(cfg, N, dev, mesh, keep_world_rays=True)
        chk.update(0.02, pos, quat, force_recompute=True)
        hk = chk._data.ray_hits_w
        hr = mesh.raycast(chk.ray_starts_w, chk.ray_directions_w, max_distance)[0]
        ha, hb = old(), new().clone()
        sw = quat_apply(quat.repeat(1, R), starts) + pos.unsqueeze(1)
        dw = quat_apply(quat.repeat(1, R), dirs)
        torch.cuda.synchronize()
        walk_same = torch.equal(hk.view(torch.int32), hr.view(torch.int32)) and torch.equal(hk.view(torch.int32), hb.view(torch.int32))
        rays_same = torch.equal(sw, chk.ray_starts_w) and torch.equal(dw, chk.ray_directions_w)
        same = torch.equal(ha.view(torch.int32), hb.view(torch.int32))
        hit = float(torch.isfinite(hb[..., 0]).float().mean())
        lines.append(f"max_distance {max_distance:g}: walk bit-identical to TerrainMesh.raycast on the launch's own rays: {walk_same}; torch-composed rays "
                     f"bit-identical to the launch's: {rays_same} (max |diff| starts {float((sw - chk.ray_starts_w).abs().max()):.2e}, dirs "
                     f"{float((dw - chk.ray_directions_w).abs().max()):.2e}); outputs (a) == (b) bit for bit: {same} "
                     f"({int((ha.view(torch.int32) != hb.view(torch.int32)).any(-1).sum())} of {N * R} rays differ); hit fraction {hit:.3f}")
        if not walk_same:
            bad = (hk.view(torch.int32) != hr.view(torch.int32)).any(-1).nonzero()[:8]
            for e, j in bad.tolist():
                lines.append(f"  ray ({e}, {j}): start {chk.ray_starts_w[e, j].tolist()} dir {chk.ray_directions_w[e, j].tolist()} launch {hk[e, j].tolist()} "
                             f"raycast {hr[e, j].tolist()}")
            raise SystemExit("\n".join(lines + ["the walk differs from TerrainMesh.raycast: not timed"]))
        del chk, hk, hr, sw, dw
        series, count = {"a": [], "b": []}, {}
        for key, fn in (("a", old), ("b", new)):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            # a way that takes more than 50 ms per call is sampled with a tenth of the launches (at least 20): 200 x 5 of them would
            # be ten minutes of one kernel, and its run-to-run spread is a fraction of a percent
            count[key] = a.launches if e0.elapsed_time(e1) < 50.0 else max(min(a.launches, 20), a.launches // 10)
            for _ in range(7 if count[key] == a.launches else 0):
                fn()
        for _ in range(a.rounds):
            for key, fn in (("a", old), ("b", new)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(count[key]):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                series[key].append(e0.elapsed_time(e1) * 1000.0 / count[key])
        for key, what in (("a", "(a) torch composition + TerrainMesh.raycast"), ("b", "(b) imx_ray_caster")):
            x = series[key]
            lines.append(f"  {what} ({count[key]} launches per sample): us per call {[round(u, 1) for u in x]}  min {min(x):.1f} median {statistics.median(x):.1f} max {max(x):.1f}")
        ma, mb = statistics.median(series["a"]), statistics.median(series["b"])
        lines.append(f"  ratio of medians (a) / (b): {ma / mb:.2f}; (b) median below (a) minimum: {mb < min(series['a'])}")
    bi = first_info
    s2 = RayCaster(cfg, 8, dev, TerrainMesh(v, t, 0.0))  # a fresh mesh: what the build takes
    lines.append(f"z-bounds: {bi['bytes']} bytes ({bi['cells']} cells, {bi['tiles']} tiles); build {s2.bounds_info['build_ns'] / 1e3:.0f} us "
                 f"(the first build of the process, code object load included: {bi['build_ns'] / 1e3:.0f} us)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
