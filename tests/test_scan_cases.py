"""CPU dry run of the height-scanner harness (tests/_scan_cases.py) with the fp32 brute force (oracle ``raycast_woop_f32``) in the
product's place: the zoo is deterministic and within its triangle budget, the host-side premises hold, the unsettled share of the
random-pose rays stays under its cap on every case, and the fp32 oracle alone passes the comparison rule everywhere -- an input the
oracle cannot pass is a wrong input, not a reason for a wider tolerance."""
import numpy as np
import pytest

import _scan_cases as sc

CASES = list(sc.zoo())
SPECIAL = [("C_pitch_narrow_thin_pit", "between"), ("C_overlap_coplanar_slab", "between"), ("C_rotated", "between"),
           ("C_overlap_coplanar_slab", "up"), ("B_metre_steps", "up"), ("A_bench_cell0", "up")]


def test_zoo_is_deterministic_and_within_budget():
    a, b = sc.build_zoo(), sc.build_zoo()
    assert list(a) == list(b) == CASES and len(CASES) == len(set(CASES))
    assert {c.family for c in a.values()} == set("ABCDE")
    for name in CASES:
        ca, cb = a[name], b[name]
        assert ca.verts.dtype == np.float32 and ca.tris.dtype == np.uint32
        assert ca.verts.tobytes() == cb.verts.tobytes() and ca.tris.tobytes() == cb.tris.tobytes(), name
        assert 1 <= len(ca.tris) <= sc.MAX_TRIANGLES, (name, len(ca.tris))
        assert int(ca.tris.max()) < len(ca.verts) and np.isfinite(ca.verts).all()


def test_host_side_premises():
    z = sc.zoo()
    # a pure height field of pitch p: the automatic cell is p (fp32), so the grid lines coincide with the lattice lines
    for name in ("B_other_diagonal", "B_rotated_order"):
        assert abs(sc.grid_cell(z[name]) - 0.1) < 1e-6
    assert sc.grid_cell(z["D_ground_plane_2e6"]) == 2.0e6
    assert sc.grid_cell(z["A_bench_cell0"]) not in (0.1, 0.05, 0.2)
    for c in z.values():
        cell, pitch = sc.grid_cell(c), sc.pattern_pitch(c)
        assert cell > 0 and (cell > 10.0 or abs(pitch / cell - round(pitch / cell)) < 1e-9), c.name  # pattern pitch = a multiple of the cell
        if c.cell > 0:  # the table stays far below the builder's 2^27 cells
            assert (np.ptp(c.verts[:, 0]) / cell + 1) * (np.ptp(c.verts[:, 1]) / cell + 1) < 2 ** 23, c.name
    # the degenerate case really holds what it says
    e = z["E_degenerate"]
    tri = e.verts[e.tris].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    rep = (e.tris[:, 0] == e.tris[:, 1]) | (e.tris[:, 1] == e.tris[:, 2]) | (e.tris[:, 0] == e.tris[:, 2])
    assert int(rep.sum()) >= 3 and int((area == 0).sum()) >= 5
    assert len(np.unique(e.tris, axis=0)) < len(e.tris) and len(np.unique(e.verts, axis=0)) < len(e.verts)
    assert len(np.unique(e.tris.reshape(-1))) < len(e.verts)
    assert len(z["E_single_triangle"].tris) == 1
    # the thin walls are thinner than 2 tau cells, the narrow box narrower than a cell
    c = z["C_pitch_narrow_thin_pit"]
    assert np.float32(4.1004) - np.float32(4.1) < 2 * sc.TAU * c.cell and 0.1 < c.cell


@pytest.mark.parametrize("variant", list(sc.VARIANTS))
@pytest.mark.parametrize("name", CASES)
def test_fp32_oracle_passes_the_rule(name, variant):
    case = sc.zoo()[name]
    fig = sc.run_scan_case(case, variant, product=False)
    assert fig["unsettled_share"] <= sc.UNSETTLED_CAP
    assert fig["hits"] > 0
    if case.axis_features and variant == "lean":
        assert fig["exact"] > 0, "no ray landed exactly on a feature line"
    if case.premise == "all_general" and variant == "lean":
        assert fig["max_owners"] > 16, fig["max_owners"]


@pytest.mark.parametrize("name,mode", SPECIAL)
def test_fp32_oracle_passes_the_rule_between_surfaces_and_upward(name, mode):
    fig = sc.run_scan_case(sc.zoo()[name], "lean", mode=mode, product=False)
    assert fig["hits"] > 0


def test_single_env_and_partial_waves():
    for variant in sc.VARIANTS:
        sc.run_scan_case(sc.zoo()["A_hs0.125_tile6"], variant, N=1, product=False)
