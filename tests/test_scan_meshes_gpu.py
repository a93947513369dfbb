"""The height scanner's fast vertical-ray path on the mesh zoo of tests/_scan_cases.py: every zoo case through each of the three
vertical observation kernels (k_obs_lean<false>, k_obs<false,true>, k_obs<false,false> -- asserted by imx_observations_kernel_name),
through the real env, against the fp64 brute force over all triangles under the comparison rule of that module.  Each case asserts
what it is there for from the builder's own cell counts; the grid-line sets assert their share of rays within tau of a grid line;
the other-diagonal height field proves that a wave of the single-wave kernel had more than 16 GENERAL-cell owners (the second to
fourth round of cast_ray_vertical_wave).  Two more classes: ray origins between surfaces (under box tops and a floating slab:
raycast_mesh semantics = the closest hit with t >= 0, i.e. the next face below) and an upward scanner from below the mesh.

Defect found by these tests: a downward ray that starts below the top surface of a QH cell got `miss` (vertical_cell dropped the
negative t of the top height and never looked at the reference list); see test_origin_between_surfaces_and_upward."""
import pytest

import _scan_cases as sc

pytestmark = pytest.mark.gpu

CASES = list(sc.zoo())


@pytest.mark.parametrize("variant", list(sc.VARIANTS))
@pytest.mark.parametrize("name", CASES)
def test_zoo_case_matches_fp64_brute_force(name, variant):
    case = sc.zoo()[name]
    fig = sc.run_scan_case(case, variant, product=True)
    assert fig["kernel"] == sc.VARIANTS[variant][0]
    assert fig["hits"] > 0 and fig["unsettled_share"] <= sc.UNSETTLED_CAP
    if case.axis_features and variant == "lean":
        assert fig["exact"] > 0, "no ray landed exactly on a feature line"
    if case.premise == "all_general" and variant == "lean":
        # every used cell is GENERAL (asserted from the builder's counts), so these rays were owners in cast_ray_vertical_wave
        assert fig["max_owners"] > 16, f"at most {fig['max_owners']} owners in a wave: the rounds past the first never ran"


@pytest.mark.parametrize("variant", list(sc.VARIANTS))
@pytest.mark.parametrize("name,mode", [("C_pitch_narrow_thin_pit", "between"), ("C_overlap_coplanar_slab", "between"), ("C_rotated", "between"),
                                       ("C_overlap_coplanar_slab", "up"), ("B_metre_steps", "up"), ("A_bench_cell0", "up")])
def test_origin_between_surfaces_and_upward(name, mode, variant):
    """``between``: the scanner 0.35 m under a root at ~0.6 m: rays start at z ~ 0.25, inside boxes with tops of 0.3 to 0.8 m and under
    the slab at 1.0 m.  Before the fix in
    vertical_cell every such ray over a QH cell whose top lay above the origin reported a miss where the fp64 reference hits the ground
    (or the next box) below.  ``up``: direction (0, 0, 1) from 30 m below the root."""
    fig = sc.run_scan_case(sc.zoo()[name], variant, mode=mode, product=True)
    assert fig["hits"] > 0


@pytest.mark.parametrize("variant", list(sc.VARIANTS))
@pytest.mark.parametrize("name,N", [("A_hs0.125_tile6", 1), ("C_overlap_coplanar_slab", 1), ("B_other_diagonal", 65)])
def test_single_env_and_ragged_batches(name, N, variant):
    sc.run_scan_case(sc.zoo()[name], variant, N=N, product=True, seed=3)
