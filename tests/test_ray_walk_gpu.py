"""GPU: the RayCaster's z-pruned walk (``cast_ray_pruned``, csrc/imx_ray_walk.h) and its bounds (``k_ray_bounds_cell`` / ``_dilate`` /
``_tile``, csrc/ray_caster.hip) on every mesh of the zoo plus the two translated ones, with the ray families of tests/_ray_walk_cases.py.

Every ray gets the three assertions of test_ray_caster_gpu.py::test_walk_is_bit_identical_to_the_exhaustive_search (in
``run_walk_case``), none is excluded and there is no tolerance: the miss mask is the brute force's, ``ray_hits_w`` is start + t32 dir with
the brute force's t32 bit for bit, and ``TerrainMesh.raycast`` (the unpruned ``cast_ray``) gives the same mask, distances and points.
That the families hold their edges and both outcomes is asserted by the CPU dry run (tests/test_ray_walk_cases.py)."""
import numpy as np
import pytest

import _ray_walk_cases as wc

pytestmark = pytest.mark.gpu

SMALL = "C_overlap_coplanar_slab"
POSITIONS = np.asarray([[0.0, 0.0, 0.0], [1.25, -0.5, 0.3], [-2.0, 3.0, -0.7]], np.float32)


@pytest.mark.parametrize("name,family", wc.case_families())
def test_walk_on_the_zoo(name, family):
    case = wc.walk_cases()[name]
    fr = []
    for max_distance in wc.distances(name, family):  # 1e6; random, grazing and long also at 10, 0, and t, t-, t+ of a hit of their own
        fig = wc.run_walk_case(case, family, max_distance)
        fr.append(f"{max_distance:.9g}: {fig['hit_fraction']:.3f}")
    print(f"hit fraction {name}/{family} by max_distance: " + ", ".join(fr))


@pytest.mark.parametrize("name", [SMALL, "A_hs0.125_tile6"])
def test_three_envs_at_three_positions(name):
    """Block = env, and the pose adds to the starts: the comparison is on the world rays the kernel stored."""
    fig = wc.run_walk_case(wc.walk_cases()[name], "random", 1.0e6, positions=POSITIONS)
    sw = fig["sensor"].ray_starts_w.cpu().numpy()
    s0, _ = wc.rays(name, "random")
    assert np.array_equal(sw, s0[None] + POSITIONS[:, None, :])  # one fp32 addition per component
    t = fig["t32"].reshape(3, -1)
    assert all(np.isfinite(t[e]).any() for e in range(3)) and not np.array_equal(np.isfinite(t[0]), np.isfinite(t[1]))


@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 513])
def test_ray_count_partition(R):
    """passes = ceil(R / 256), threads = the rays of a pass rounded up to whole waves: 257 and 513 rays take 2 and 3 passes, 1 and 63 a
    partial wave.  Every ray of every env is written (``feed_sensor`` pre-fills ``ray_hits_w`` with NaN, ``run_walk_case`` finds none)."""
    fig = wc.run_walk_case(wc.walk_cases()[SMALL], "random", 1.0e6, count=R, positions=POSITIONS[:2])
    assert fig["rays"] == 2 * R
    hits = fig["sensor"]._data.ray_hits_w.cpu().numpy()
    assert hits.shape == (2, R, 3) and not np.isnan(hits).any()


def test_a_second_sensor_reuses_the_bounds():
    from isaaclab_amd.env import TerrainMesh

    case = wc.walk_cases()[SMALL]
    mesh = TerrainMesh(case.verts, case.tris, case.cell)
    s, d = wc.rays(SMALL, "long")
    first = wc.feed_sensor(mesh, s, d, 1.0e6)
    second = wc.feed_sensor(mesh, s, d, 1.0e6)
    a, b = first.bounds_info, second.bounds_info
    assert a["build_ns"] > 0 and b["build_ns"] == 0
    assert (a["cells"], a["tiles"], a["bytes"]) == (b["cells"], b["tiles"], b["bytes"])
    assert a["cells"] == 64 * a["tiles"] and a["tiles"] == ((mesh.nx + 7) // 8) * ((mesh.ny + 7) // 8)
    h1, h2 = first._data.ray_hits_w.cpu().numpy(), second._data.ray_hits_w.cpu().numpy()
    assert np.isfinite(h1).any() and np.array_equal(h1.view(np.uint32), h2.view(np.uint32))
