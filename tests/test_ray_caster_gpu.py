"""GPU: the RayCaster sensor (producers.RayCaster -> imx_ray_caster, csrc/ray_caster.hip) and its z-pruned grid walk (csrc/imx_ray_walk.h).

The binding criterion is exactness: on the kernel's OWN world rays the walk's closest hit is bit for bit the brute-force search over all
triangles in the same fp32 Woop arithmetic (oracle.raycast.raycast_woop_f32) and bit for bit ``TerrainMesh.raycast``; no ray is excluded."""

import functools

import numpy as np
import pytest
import torch

from _ray_caster_cases import SENSOR_NPZ, fork_cfg, lidar7_cfg, make_poses, world_rays64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def terrain(which):
    if which == "rough":
        from isaaclab_amd.terrain import make_rough_terrain

        v, t, _ = make_rough_terrain(2, 3, tile=4.0, border=2.0, seed=21)
        assert len(t) == 4648
        return v, t
    from _scan_cases import zoo

    c = zoo()["C_overlap_coplanar_slab"]  # vertical walls, overlapping boxes, a floating slab over a box and the ground
    return c.verts, c.tris


@functools.lru_cache(maxsize=None)
def mesh_of(which, cell):
    from isaaclab_amd.env import TerrainMesh

    v, t = terrain(which)
    return TerrainMesh(v, t, cell)


def make_sensor(cfg, N, mesh, seed=0, **kw):
    from isaaclab_amd.producers import RayCaster

    return RayCaster(cfg, N, "cuda", mesh, seed=seed, keep_world_rays=True, **kw)


def cast(cfg, N, which, cell, pose_seed):
    v, _ = terrain(which)
    pos, quat = make_poses(N, v, pose_seed)
    s = make_sensor(cfg, N, mesh_of(which, cell))
    s.update(0.02, torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda(), force_recompute=True)
    return s, pos, quat


CASES = [  # N, pattern, cell, max_distance, mesh, yaw only
    (129, "fork", 0.1, 1.0e6, "rough", False), (129, "fork", 0.0, 10.0, "rough", False), (129, "fork", 0.37, 1.0e6, "rough", True),
    (1, "fork", 0.1, 1.0e6, "rough", False), (63, "lidar7", 0.0, 1.0e6, "rough", False), (64, "fork", 0.37, 10.0, "rough", False),
    (65, "lidar7", 0.37, 10.0, "rough", True), (257, "lidar7", 0.1, 10.0, "rough", False), (65, "fork", 0.25, 1.0e6, "boxes", False),
    (64, "fork", 0.0, 10.0, "boxes", True),
]


@pytest.mark.parametrize("N,pattern,cell,max_distance,which,yaw_only", CASES)
def test_walk_is_bit_identical_to_the_exhaustive_search(N, pattern, cell, max_distance, which, yaw_only):
    from oracle.raycast import raycast_woop_f32

    cfg = (fork_cfg if pattern == "fork" else lidar7_cfg)(max_distance, yaw_only)
    s, pos, quat = cast(cfg, N, which, cell, pose_seed=5)
    R = s.num_rays
    assert R == (360 if pattern == "fork" else 7)
    sw, dw = s.ray_starts_w.cpu().numpy().reshape(-1, 3), s.ray_directions_w.cpu().numpy().reshape(-1, 3)
    hits = s._data.ray_hits_w.cpu().numpy().reshape(-1, 3)
    v, t = terrain(which)
    _, t32, _ = raycast_woop_f32(v, t, sw, dw, max_distance)
    hit = np.isfinite(t32)
    # misses are +inf in all three components, hits finite in all three
    assert np.array_equal(np.isposinf(hits).all(1), ~hit) and np.array_equal(np.isfinite(hits).all(1), hit)
    # ray_hits_w = start + t * dir in fp32 with the brute force's t: equal bits mean equal t
    want = sw[hit] + t32[hit, None] * dw[hit]
    assert np.array_equal(hits[hit], want.astype(np.float32)), int((hits[hit] != want).any(1).sum())
    # ... and bit for bit what the existing walk gives on the same rays, distances included
    h2, d2, _, _ = s.mesh.raycast(s.ray_starts_w, s.ray_directions_w, max_distance, return_distance=True)
    d2 = d2.cpu().numpy().reshape(-1)
    assert np.array_equal(np.isfinite(d2), hit) and np.array_equal(d2[hit], t32[hit])
    assert np.array_equal(h2.cpu().numpy().reshape(-1, 3)[hit], hits[hit])
    if which == "rough" and N >= 63:
        print(f"hit fraction {hit.mean():.3f}")
        if pattern == "fork" and not yaw_only:
            assert hit.mean() > 0.2
    # pos_w / quat_w are the body pose (no drift here)
    assert np.array_equal(s._data.pos_w.cpu().numpy(), pos) and np.array_equal(s._data.quat_w.cpu().numpy(), quat)


@pytest.mark.parametrize("yaw_only", [False, True])
def test_geometry_against_fp64(yaw_only):
    from oracle.raycast import raycast_f64

    cfg = fork_cfg(1.0e6, yaw_only, offset={"pos": (0.05, -0.02, 0.1), "rot": (0.9238795, 0.0, 0.3826834, 0.0)})
    s, pos, quat = cast(cfg, 129, "rough", 0.1, pose_seed=5)
    sw, dw = s.ray_starts_w.cpu().numpy(), s.ray_directions_w.cpu().numpy()
    s64, d64 = world_rays64(pos, quat, s.ray_starts.cpu().numpy(), s.ray_directions.cpu().numpy(), yaw_only)
    print("world rays vs fp64: dirs %.2e starts %.2e" % (np.abs(dw - d64).max(), np.abs(sw - s64).max()))
    assert np.abs(dw - d64).max() <= 1e-6 and np.abs(sw - s64).max() <= 1e-5
    v, t = terrain("rough")
    sw, dw = sw.reshape(-1, 3), dw.reshape(-1, 3)
    hits = s._data.ray_hits_w.cpu().numpy().reshape(-1, 3)
    _, t64, f64 = raycast_f64(v, t, sw, dw, 1.0e6)
    got = np.isfinite(hits[:, 0])
    flips = np.flatnonzero(got != np.isfinite(t64))
    assert flips.size == 0, flips[:10]
    dist = np.linalg.norm(hits[got].astype(np.float64) - sw[got], axis=1) / np.linalg.norm(dw[got].astype(np.float64), axis=1)
    tri = v[t[f64[got]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    cosi = np.abs((n * dw[got]).sum(1)) / np.maximum(np.linalg.norm(n, axis=1), 1e-30)
    err = np.abs(dist - t64[got])
    steep = cosi > 0.2
    rel = err / np.maximum(t64[got], 1.0)
    print("hits vs fp64: max err*cos %.2e, max rel err steep %.2e (%d steep of %d)" % ((err * np.maximum(cosi, 1e-3)).max(), rel[steep].max(),
                                                                                      steep.sum(), got.sum()))
    assert (err * np.maximum(cosi, 1e-3)).max() <= 1e-5 and rel[steep].max() <= 1e-5


def test_envs_that_are_not_outdated_keep_their_hits_and_ranges_follow_the_hits():
    N = 65
    v, _ = terrain("rough")
    s, pos, quat = cast(fork_cfg(1.0e6), N, "rough", 0.1, pose_seed=7)
    first = s._data.ray_hits_w.clone()
    assert not bool(s._is_outdated.any())
    pos2, quat2 = make_poses(N, v, 8)
    p2, q2 = torch.from_numpy(pos2).cuda(), torch.from_numpy(quat2).cuda()
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[::3] = True
    s.update(0.02, p2, q2, force_recompute=True, reset_mask=mask)  # 0.02 < update_period: only the reset envs are outdated
    now = s._data.ray_hits_w
    keep = ~mask.cpu().numpy()
    assert np.array_equal(now.cpu().numpy().view(np.uint32)[keep], first.cpu().numpy().view(np.uint32)[keep])
    assert np.array_equal(s._data.pos_w.cpu().numpy()[~keep], pos2[~keep]) and np.array_equal(s._data.pos_w.cpu().numpy()[keep], pos[keep])
    assert not np.array_equal(now.cpu().numpy()[~keep], first.cpu().numpy()[~keep])
    ts = s._timestamp.cpu().numpy()
    assert np.array_equal(ts[~keep], np.full((~keep).sum(), np.float32(0.02))) and np.array_equal(ts[keep], np.full(keep.sum(), np.float32(0.02) + np.float32(0.02)))
    # the range image, for the refreshed envs and for those that kept their hits: min(||hits - pos_w||, clip), misses = clip
    r = s.ranges(10.0).cpu().numpy()
    hits, pw = s._data.ray_hits_w.cpu().numpy().astype(np.float64), s._data.pos_w.cpu().numpy().astype(np.float64)
    miss = ~np.isfinite(hits[..., 0])
    with np.errstate(invalid="ignore"):
        want = np.minimum(np.linalg.norm(hits - pw[:, None, :], axis=-1), 10.0)
    assert miss.any() and (~miss).any() and np.array_equal(r[miss], np.full(miss.sum(), np.float32(10.0)))
    assert np.abs(r[~miss] - want[~miss]).max() <= 1e-5 * 10.0 and (np.abs(r[~miss] - want[~miss]) <= 1e-5 * want[~miss] + 1e-12).all()
    assert np.array_equal(s.ranges(3.0).cpu().numpy(), np.minimum(r, np.float32(3.0)))  # another clip, nobody outdated


def test_same_seed_same_drift_and_the_drift_moves_the_sensor():
    N = 64
    v, _ = terrain("rough")
    pos, quat = make_poses(N, v, 9)
    p, q = torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda()
    out = []
    for seed in (3, 3, 4):
        s = make_sensor(fork_cfg(10.0, drift_range=(-0.05, 0.15)), N, mesh_of("rough", 0.1), seed=seed)
        s.reset()
        s.update(0.02, p, q, force_recompute=True)
        out.append((s.drift.cpu().numpy().copy(), s._data.pos_w.cpu().numpy().copy()))
    assert np.array_equal(out[0][0], out[1][0]) and not np.array_equal(out[0][0], out[2][0])
    d = out[0][0]
    assert d.min() >= -0.05 and d.max() <= 0.15 and d.std() > 0.02 and len(np.unique(d)) > N
    assert np.array_equal(out[0][1], pos + d)
    s.reset(env_ids=[1, 5])  # a second reset draws again, for those envs only
    d2 = s.drift.cpu().numpy()
    changed = (d2 != out[2][0]).any(1)
    assert changed[[1, 5]].all() and changed.sum() == 2
    u = torch.rand(N, 3, device="cuda")
    s.reset(uniforms=u)
    lo, hi = np.float32(-0.05), np.float32(0.15)  # Tensor.uniform_(lo, hi): u * (hi - lo) + lo in fp32
    assert np.array_equal(s.drift.cpu().numpy(), u.cpu().numpy() * (hi - lo) + lo)


def test_one_launch_in_a_captured_graph_replays_the_eager_call():
    N = 129
    v, _ = terrain("rough")
    pos, quat = make_poses(N, v, 11)
    p, q = torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda()
    eager = make_sensor(fork_cfg(10.0), N, mesh_of("rough", 0.1))
    eager.update(0.02, p, q, force_recompute=True)
    want_r = eager.ranges(10.0).clone()
    graphed = make_sensor(fork_cfg(10.0), N, mesh_of("rough", 0.1))
    graphed.update(0.0, p, q, substeps=0)  # (binds the pose; nothing advances)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update(0.02, p, q, force_recompute=True)
        graphed.ranges(10.0)
    graphed._timestamp.zero_(); graphed._timestamp_last_update.zero_(); graphed._is_outdated.fill_(True)  # (warm-up / capture state)
    graphed._data.ray_hits_w.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in ((graphed._data.ray_hits_w, eager._data.ray_hits_w), (graphed._ranges, want_r), (graphed._timestamp, eager._timestamp),
                 (graphed._data.pos_w, eager._data.pos_w), (graphed.ray_starts_w, eager.ray_starts_w)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert not bool(graphed._is_outdated.any())


def test_fixture_sensor_semantics_on_the_device():
    """Fixture (b) (tools/gen_golden_ray_caster.py: the real RayCaster / SensorBase): the recorded world rays in both attach modes with a
    rotated offset and non-zero drift, and the flags and clocks over 12 updates with a partial reset after the seventh."""
    z = np.load(SENSOR_NPZ)
    N = int(z["pos"].shape[0])
    for mode, yaw_only in (("full", False), ("yaw", True)):
        cfg = fork_cfg(1.0e6, yaw_only, offset={"pos": tuple(z["offset_pos"]), "rot": tuple(z["offset_rot"])}, drift_range=tuple(z["drift_range"]))
        s = make_sensor(cfg, N, mesh_of("rough", 0.1))
        s.reset(uniforms=torch.from_numpy(z["uniforms0"]).cuda())
        s.update(0.02, torch.from_numpy(z["pos"]).cuda(), torch.from_numpy(z["quat"]).cuda(), force_recompute=True)
        assert np.abs(s.ray_starts_w.cpu().numpy() - z[f"{mode}/ray_starts_w"]).max() <= 1e-6
        assert np.abs(s.ray_directions_w.cpu().numpy() - z[f"{mode}/ray_directions_w"]).max() <= 1e-6
        assert np.abs(s._data.pos_w.cpu().numpy() - z[f"{mode}/pos_w"]).max() <= 1e-6
        assert np.array_equal(s._data.quat_w.cpu().numpy(), z["quat"])
    # the clocks: 12 updates of dt = 0.02 at update_period = 0.1, data asked after each, envs `reset_ids` reset after the seventh
    s = make_sensor(fork_cfg(10.0), N, mesh_of("rough", 0.1))
    p, q = torch.from_numpy(z["pos"]).cuda(), torch.from_numpy(z["quat"]).cuda()
    for k in range(12):
        s.update(0.02, p, q)
        assert np.array_equal(s._is_outdated.cpu().numpy(), z["clock/outdated_before"][k]), k
        s.data
        assert np.array_equal(s._timestamp.cpu().numpy(), z["clock/timestamp"][k]) and np.array_equal(s._timestamp_last_update.cpu().numpy(), z["clock/last_update"][k]), k
        assert not bool(s._is_outdated.any())
        if k == 6:
            s.reset(env_ids=z["clock/reset_ids"].tolist())
            assert np.array_equal(s._is_outdated.cpu().numpy(), z["clock/outdated_after_reset"])


def lidar_ranges(env):
    """A Python-evaluated observation term reading the lidar's range image (the fork's lidarfly_env.py:211-218)."""
    return env.scene["lidar"].ranges(10.0) / 10.0


def test_env_scene_lidar(tmp_path):
    import copy

    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed
    from isaaclab_amd.terrain import make_rough_terrain

    N = 64
    fx = copy.deepcopy(load_task_cfg("Isaac-Velocity-Rough-Anymal-C-v0"))
    blob0 = compile_plan(fx["env"], ROBOTS[fx["robot"]]).blob.copy()
    lidar = dict(fork_cfg(10.0), class_type="isaaclab.sensors.ray_caster.ray_caster:RayCaster", prim_path="{ENV_REGEX_NS}/Robot/base")
    fx["env"]["scene"]["lidar"] = lidar
    assert np.array_equal(compile_plan(fx["env"], ROBOTS[fx["robot"]]).blob, blob0)  # the plan does not know the sensor
    v, t, e = make_rough_terrain(2, 3, tile=4.0, border=2.0, seed=21)
    feed = StateFeed(ROBOTS[fx["robot"]], N, "cuda:0", seed=9, num_snapshots=7, extent_xy=(e[0] - 1.0, e[1] - 1.0))
    env = ManagerBasedRLEnv(fx, state_feed=feed, terrain=(v, t), terrain_cell=0.1)
    assert np.array_equal(env.plan.blob, blob0) and env._ray_sensors == [] and "lidar" in env.scene.keys()
    env.reset()
    assert env._ray_sensors == []  # never asked: nothing built, nothing launched
    sensor = env.scene["lidar"]
    assert len(env._ray_sensors) == 1 and sensor.num_rays == 360 and env.scene["lidar"] is sensor
    alone = make_sensor(fork_cfg(10.0), N, env.terrain)
    act = torch.zeros(N, env.plan.action_dim, device="cuda:0")
    refreshed, step_resets = [], torch.zeros(N, dtype=torch.bool, device="cuda:0")
    for k in range(11):
        before = sensor._sensor._timestamp_last_update.clone()
        was_outdated = sensor._sensor._is_outdated.clone()
        hits = sensor.data.ray_hits_w
        refreshed.append(was_outdated.cpu().numpy())
        assert not bool(sensor._sensor._is_outdated.any())
        assert torch.equal(sensor._sensor._timestamp_last_update != before, was_outdated & (sensor._sensor._timestamp != before))
        if bool(was_outdated.any()):  # the stand-alone producer on the feed's root pose at the same moment
            alone._is_outdated.fill_(True)
            alone.update(0.0, feed["root_pos_w"].contiguous(), feed["root_quat_w"].contiguous(), force_recompute=True, substeps=0)
            assert torch.equal(hits[was_outdated].view(torch.int32), alone._data.ray_hits_w[was_outdated].view(torch.int32))
            assert bool(torch.isfinite(hits[was_outdated]).any())
        env.step(act)
        step_resets |= env.reset_buf
        if k == 2:  # env.reset(env_ids) reaches the sensor: those envs restart their clocks and are outdated at once
            env.reset(env_ids=[3, 4])
            assert sensor._sensor._is_outdated.cpu().numpy().nonzero()[0].tolist() == [3, 4]
            assert float(sensor._sensor._timestamp[3]) == 0.0 and float(sensor._sensor._timestamp[0]) > 0.0
            sensor.data
    # update_period 0.1 at step_dt 0.02 (4 x 0.005): every fifth env step; the envs reset after the third step five steps after that
    refreshed = np.stack(refreshed)  # (step, env)
    quiet = ~step_resets.cpu().numpy()
    quiet[[3, 4]] = False
    assert quiet.sum() > N // 2
    assert np.array_equal(refreshed[:, quiet].T.nonzero()[1].reshape(-1, 3), np.tile([0, 5, 10], (quiet.sum(), 1))), refreshed[:, quiet].sum(1)
    if not step_resets[3]:
        assert refreshed[:, 3].nonzero()[0].tolist() == [0, 8], refreshed[:, 3]

    # learn(1) with a Python-evaluated observation term reading the range image
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    fx2 = copy.deepcopy(fx)
    fx2["env"]["observations"]["policy"]["lidar"] = {"func": lidar_ranges, "params": {}, "_dim": 360}
    feed2 = StateFeed(ROBOTS[fx["robot"]], N, "cuda:0", seed=9, num_snapshots=7, extent_xy=(e[0] - 1.0, e[1] - 1.0))
    env2 = ManagerBasedRLEnv(fx2, state_feed=feed2, terrain=(v, t), terrain_cell=0.1)
    venv = RslRlVecEnvWrapper(env2)
    runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=6), log_dir=None, device="cuda:0", use_graph=False)
    runner.learn(1)
    torch.cuda.synchronize()
    obs = runner.alg.storage.observations
    assert obs.shape[-1] == env.plan.obs_dim + 360 and bool(torch.isfinite(obs).all())
    lid = obs[..., -360:]
    assert float(lid.min()) >= 0.0 and float(lid.max()) <= 1.0 and float(lid.std()) > 0.01
