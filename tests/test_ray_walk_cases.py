"""CPU dry run of the ray-walk harness (tests/_ray_walk_cases.py) with the fp32 brute force (``raycast_woop_f32``) in the sensor's
place, for every (case, family) the GPU test runs: the families are deterministic, every edge kind a family advertises is there in
non-zero number, the brute force gives hits and misses wherever both are possible, and the three max_distance values taken from a hit
decide that hit the way the ``t <= best`` rule says.  An input the oracle cannot make sense of is a wrong input."""
import numpy as np
import pytest

import _ray_walk_cases as wc

PAIRS = wc.case_families()
# No family is all-miss by construction: each holds rays aimed at or across the mesh.  All-miss by construction are the SUB-sets counted
# as ``outside_zero`` (a zero component beside the grid), ``beside_slab`` (dz == 0 above or below the slab) and most sky rays.  On the
# single triangle and on the 2e6 m plane the structured families still get both outcomes from their own aimed / downward rays.
# What each family must hold (the counts of _ray_walk_cases.edge_kinds):
NEEDS = {"random": (),
         "axis": ("dx0", "dy0", "dz0", "dxy0_dz0", "down", "up", "outside_zero", "beside_slab", "at_slab_edge", "denormal", "tiny"),
         "gridline": ("on_line", "on_node", "diagonal", "tie", "dx0", "dy0", "dz0"),
         "grazing": ("t0_xy", "t0_z", "dz0", "start_moved"),
         "long": ("t0_xy", "diagonal", "t1_z")}


def test_cases_and_families_are_deterministic_and_in_range():
    names = list(wc.walk_cases())
    assert len(names) == len(wc.zoo()) + 2 and sum(n.startswith("F_far_") for n in names) == 2
    for name in wc.FAR_OF:  # the translated cases: the same triangles, the vertices moved and rounded to fp32
        c, f = wc.zoo()[name], wc.walk_cases()["F_far_" + name]
        assert np.array_equal(c.tris, f.tris) and f.verts.dtype == np.float32
        assert np.abs(f.verts.astype(np.float64) - c.verts - np.asarray(wc.FAR_SHIFT)).max() <= np.spacing(np.float32(2048.0)) / 2
    for name, family in PAIRS:
        a, b = wc.make_rays(name, family), wc.make_rays(name, family)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, family)
        s, d = a
        assert s.dtype == np.float32 and d.dtype == np.float32 and s.shape == d.shape and 0 < len(s) <= wc.MAX_RAYS
        assert np.isfinite(s).all() and np.isfinite(d).all() and float(np.abs(s).max()) <= 2.0e6 and (d != 0).any(1).all()
        assert not np.signbit(s[s == 0]).any()


@pytest.mark.parametrize("name,family", PAIRS)
def test_family_holds_its_edges_and_the_brute_force_both_outcomes(name, family):
    case = wc.walk_cases()[name]
    s, d = wc.rays(name, family)
    fig = wc.run_walk_case(case, family, 1.0e6, product=False)
    kinds = fig["kinds"]
    print(f"[walk] {name}/{family}: " + ", ".join(f"{k} {v}" for k, v in kinds.items() if v), flush=True)
    for k in NEEDS[family]:
        assert kinds[k] > 0, f"{name}/{family}: no ray of kind '{k}'"
    g = wc.grid_of(name)
    if family == "axis" and g.tops:
        assert kinds["in_face_plane"] > 0
    if family == "grazing" and g.tops:
        assert kinds["in_face_plane"] > 0, f"{name}: no grazing ray in the plane of a horizontal face"
    if family == "gridline" and g.nx > 8 and g.ny > 8:  # a tile line that is no edge of the grid, and the last line
        on_tile = lambda o, x0, n: any((o == wc.F(x0 + wc.F(wc.F(k) * g.cell))).any() for k in range(8, n, 8))  # noqa: E731
        assert on_tile(s[:, 0], g.x0, g.nx) and on_tile(s[:, 1], g.y0, g.ny)
        assert (s[:, 0] == g.x1).any() and (s[:, 1] == g.y1).any()
    assert fig["hits"] > 0 and fig["misses"] > 0, f"{name}/{family}: {fig['hits']} hits, {fig['misses']} misses"


@pytest.mark.parametrize("name,family", [p for p in PAIRS if p[1] in wc.DISTANCE_FAMILIES])
def test_distances_taken_from_a_hit_decide_that_hit(name, family):
    from oracle.raycast import raycast_woop_f32

    case = wc.walk_cases()[name]
    s, d = wc.rays(name, family)
    r, t, below, above = wc.hit_distances(name, family)
    assert 0.0 < below < t < above < 1.0e6
    out = [raycast_woop_f32(case.verts, case.tris, s[r:r + 1], d[r:r + 1], m)[1][0] for m in (t, above, below)]
    assert out[0] == np.float32(t) and out[1] == np.float32(t), out  # on and above t: the hit, at t
    assert np.isposinf(out[2]), out  # below: no hit at this t, and none nearer (t was the closest)
    assert wc.distances(name, family) == [1.0e6, 10.0, 0.0, t, below, above]


def test_n3_and_ray_count_inputs():
    """The inputs of the GPU file's N = 3 and ray-count runs, through the same harness."""
    case = wc.walk_cases()["C_overlap_coplanar_slab"]
    pos = np.asarray([[0.0, 0.0, 0.0], [1.25, -0.5, 0.3], [-2.0, 3.0, -0.7]], np.float32)
    fig = wc.run_walk_case(case, "random", 1.0e6, product=False, positions=pos)
    assert fig["rays"] == 3 * len(wc.rays(case.name, "random")[0]) and fig["hits"] > 0 and fig["misses"] > 0
    for R in (1, 63, 513):
        assert wc.run_walk_case(case, "random", 1.0e6, product=False, count=R, positions=pos[:2])["rays"] == 2 * R
