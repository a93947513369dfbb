"""The RayCaster's z-pruned grid walk (``cast_ray_pruned``, csrc/imx_ray_walk.h, and the bounds kernels of csrc/ray_caster.hip) on the
mesh zoo of tests/_scan_cases.py, with ray sets made for the walk's own branches, and one harness that feeds them to the sensor as they
are and holds every ray, bit for bit, to the fp32 brute force (``oracle.raycast.raycast_woop_f32``) and to the unpruned ``cast_ray``.

Feeding exact rays: ``producers.RayCaster`` keeps its local pattern in ``ray_starts`` / ``ray_directions`` (device tensors whose pointers
the launch struct holds); with ``attach_yaw_only`` the kernel leaves the directions alone and rotates the starts by the yaw quaternion
only.  The harness builds a sensor from an R x 1 grid pattern, copies the family's rays into the two tensors in place and updates with an
identity quaternion and a zero position: the *exact* families must come back from ``ray_starts_w`` / ``ray_directions_w`` bit for bit.

Families (functions of the case's vertices, grid origin, cell and z-range; fixed seeds; |coordinate| <= 2e6, finite):
  random   origins over the case's region grown by 2 m, z from zmin - 1 to zmax + 3, directions uniform on the sphere;
  axis     (exact) zero direction components: dx == 0, dy == 0, both with dz == 0, dx == dy == 0 (the delegation to cast_ray), a zero
           component with the origin outside the grid on that axis (the early ``return false``), dz == 0 at zmin, zmax and the box-top
           heights and +-1 ulp, +-3 mm of them (just past the slack), denormal and 1e-30 components beside a unit one;
  gridline (exact) origins on the grid's lines and nodes x0 + k cell (fp32, as the kernel computes them), k also on the tile lines and on
           the last line, shifted by SHIFTS x tau x cell; directions along the lines, on exact diagonals (tmx == tmy at every step) and
           1 ulp off them;
  grazing  rays from outside the grid's box (t0 from the xy clip) aimed at mesh vertices, edge midpoints and face centroids: from a
           random height, in the horizontal plane of the target (the plane of the face when the target's face is horizontal), from 50 m
           above zmax (t0 from the z clip) and from below zmin pointing up;
  long     near-horizontal rays (|dz| / |dxy| from 1e-4 to 1e-1) across the whole grid on diagonals and 3:1 slopes at heights through
           the slab, and sky rays from inside the footprint.
The *far* cases are two zoo cases translated by (+1000, -2000, +500) (vertices rounded to fp32 after the shift): the relative part of the
slack and the running tmx / tmy sums at their largest.  They take the random, grazing and long families in the shifted frame.

``walk_setup`` restates the walk's clip and start cell in numpy fp32.  It serves the edge counts of the dry run only (which t0 a ray
gets, whether it leaves early, whether its first step is a tie); nothing is compared against it."""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass, replace

import numpy as np

from _scan_cases import SHIFTS, TAU, Case, grid_cell, zoo
from oracle.raycast import raycast_woop_f32

F = np.float32
FAMILIES = ("random", "axis", "gridline", "grazing", "long")
EXACT = ("axis", "gridline")  # the fed rays must come back bit for bit
FAR_FAMILIES = ("random", "grazing", "long")
DISTANCE_FAMILIES = ("random", "grazing", "long")  # also run at max_distance 10, 0 and the three values around a hit's own t
FAR_SHIFT = (1000.0, -2000.0, 500.0)
FAR_OF = ("B_metre_steps", "C_overlap_coplanar_slab")  # one height field, one box scene
MAX_RAYS = 16384


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def walk_cases() -> dict:
    """The zoo plus the two translated cases."""
    out = dict(zoo())
    sh = np.asarray(FAR_SHIFT, np.float64)
    for name in FAR_OF:
        c = zoo()[name]
        v = (c.verts.astype(np.float64) + sh).astype(np.float32)
        x0, x1, y0, y1 = c.region
        far = replace(c, name="F_far_" + name, family="F", verts=v, cell=grid_cell(c), premise="any",
                      region=(x0 + sh[0], x1 + sh[0], y0 + sh[1], y1 + sh[1]), centers=())
        out[far.name] = far
    return out


def case_families():
    """Every (case name, family) the GPU test runs, the cases slowest."""
    return [(n, f) for n, c in walk_cases().items() for f in (FAR_FAMILIES if c.family == "F" else FAMILIES)]


@dataclass(frozen=True)
class Grid:
    x0: np.float32
    y0: np.float32
    cell: np.float32
    inv_cell: np.float32
    nx: int
    ny: int
    x1: np.float32  # x0 + nx * cell in fp32, the far edge as cast_ray computes it
    y1: np.float32
    zmin: np.float32
    zmax: np.float32
    tops: tuple  # the heights of the horizontal faces
    mx1: float  # the mesh's own far edge (the grid reaches up to a cell beyond it; the 2e6 m plane's, a whole 2e6 m cell)
    my1: float

    def line_x(self, k):
        return F(self.x0 + F(F(k) * self.cell))

    def line_y(self, k):
        return F(self.y0 + F(F(k) * self.cell))


@functools.lru_cache(maxsize=None)
def grid_of(name: str) -> Grid:
    """The grid imx_mesh_create lays over the case (origin = the smallest vertex coordinates, unused vertices included) and the z-range
    of the triangles."""
    c = walk_cases()[name]
    v = c.verts
    x0, y0, cell = F(v[:, 0].min()), F(v[:, 1].min()), F(grid_cell(c))
    nx = int(math.floor((float(v[:, 0].max()) - float(x0)) / float(cell))) + 1
    ny = int(math.floor((float(v[:, 1].max()) - float(y0)) / float(cell))) + 1
    tri = v[c.tris]
    flat = (tri[:, 0, 2] == tri[:, 1, 2]) & (tri[:, 1, 2] == tri[:, 2, 2])
    e1, e2 = (tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64)
    flat &= np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) > 0
    used = v[np.unique(c.tris.reshape(-1))]
    return Grid(x0, y0, cell, F(F(1.0) / cell), nx, ny, F(x0 + F(F(nx) * cell)), F(y0 + F(F(ny) * cell)), F(used[:, 2].min()),
                F(used[:, 2].max()), tuple(float(z) for z in np.unique(tri[flat, 0, 2])), float(v[:, 0].max()), float(v[:, 1].max()))


def horizontal_faces(case: Case):
    tri = case.verts[case.tris]
    flat = (tri[:, 0, 2] == tri[:, 1, 2]) & (tri[:, 1, 2] == tri[:, 2, 2])
    e1, e2 = (tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64)
    return tri[flat & (np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) > 0)]


# ---------------------------------------------------------------------------------------------------------------- the walk's set-up, fp32
def walk_setup(g: Grid, starts, dirs, max_dist=1.0e6) -> dict:
    """cast_ray's and cast_ray_pruned's clip and start cell, operation by operation in numpy fp32 (no contraction): which t0 each walk
    starts from, which rays leave before the walk, whether the first step is a tmx == tmy tie.  For the edge counts only."""
    s, d = np.asarray(starts, F), np.asarray(dirs, F)
    ox, oy, oz, dx, dy, dz = s[:, 0], s[:, 1], s[:, 2], d[:, 0], d[:, 1], d[:, 2]
    R = len(s)
    with np.errstate(all="ignore"):
        t0, t1 = np.zeros(R, F), np.full(R, F(max_dist), F)
        outside_zero = np.zeros(R, bool)
        for o, dd, lo, hi in ((ox, dx, g.x0, g.x1), (oy, dy, g.y0, g.y1)):
            nz = dd != 0
            ta, tb = (lo - o) / dd, (hi - o) / dd
            t0 = np.where(nz, np.fmax(t0, np.fmin(ta, tb)), t0)
            t1 = np.where(nz, np.fmin(t1, np.fmax(ta, tb)), t1)
            outside_zero |= ~nz & ((o < lo) | (o > hi))
        vertical = (dx == 0) & (dy == 0)
        slack0 = F(1.0e-3) + F(1.0e-5) * (np.abs(oz) + max(abs(g.zmin), abs(g.zmax)))
        z_lo, z_hi = g.zmin - F(2.0) * slack0, g.zmax + F(2.0) * slack0
        nz = dz != 0
        ta, tb = (z_lo - oz) / dz, (z_hi - oz) / dz
        te, tx = np.fmin(ta, tb), np.fmax(ta, tb)
        t0p = np.where(nz, np.fmax(t0, te - F(1.0e-4) * np.abs(te)), t0)
        t1p = np.where(nz, np.fmin(t1, tx + F(1.0e-4) * np.abs(tx)), t1)
        beside_slab = ~nz & ((oz < z_lo) | (oz > z_hi))

        def start(t):
            ix = np.clip(np.floor((F(ox + t * dx) - g.x0) * g.inv_cell), 0, g.nx - 1).astype(np.int64)
            iy = np.clip(np.floor((F(oy + t * dy) - g.y0) * g.inv_cell), 0, g.ny - 1).astype(np.int64)
            bx = g.x0 + (ix + (dx > 0)).astype(F) * g.cell
            by = g.y0 + (iy + (dy > 0)).astype(F) * g.cell
            tmx = np.where(dx != 0, (bx - ox) / dx, F(np.inf))
            tmy = np.where(dy != 0, (by - oy) / dy, F(np.inf))
            return ix, iy, tmx, tmy

        ix, iy, tmx, tmy = start(t0)
        ixp, iyp, _, _ = start(t0p)
    walks = ~vertical & ~outside_zero & (t0 <= t1)
    return dict(walks=walks, vertical=vertical, outside_zero=outside_zero & ~vertical, beside_slab=beside_slab & walks,
                t0_xy=walks & (t0 > 0), t0_z=walks & (t0p > t0), t1_z=walks & (t1p < t1), tie=walks & np.isfinite(tmx) & (tmx == tmy),
                start_moved=walks & (t0p <= t1p) & ((ix != ixp) | (iy != iyp)))


def _on_line(g: Grid, o, axis):
    """Origins that are bit for bit a grid line x0 + k cell, 0 <= k <= n."""
    x0, n = (g.x0, g.nx) if axis == 0 else (g.y0, g.ny)
    k = np.clip(np.rint((o.astype(np.float64) - float(x0)) / float(g.cell)), 0, n)
    return F(x0 + k.astype(F) * g.cell) == o


def edge_kinds(name: str, starts, dirs) -> dict:
    """Counts of the edge kinds among the rays (dry run: every advertised kind must be there)."""
    g = grid_of(name)
    s, d = np.asarray(starts, F), np.asarray(dirs, F)
    w = walk_setup(g, s, d)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    tiny = np.finfo(F).tiny
    onx, ony = _on_line(g, s[:, 0], 0), _on_line(g, s[:, 1], 1)
    tops = np.asarray(g.tops, F)
    k = dict(rays=len(s), dx0=(dx == 0) & (dy != 0), dy0=(dy == 0) & (dx != 0), dz0=dz == 0, dxy0_dz0=((dx == 0) ^ (dy == 0)) & (dz == 0),
             down=w["vertical"] & (dz < 0), up=w["vertical"] & (dz > 0), outside_zero=w["outside_zero"], beside_slab=w["beside_slab"],
             denormal=((np.abs(d) < tiny) & (d != 0)).any(1), tiny=((np.abs(d) <= F(1e-30)) & (d != 0)).any(1), on_line=onx | ony, on_node=onx & ony,
             diagonal=(np.abs(dx) == np.abs(dy)) & (dx != 0), tie=w["tie"], t0_xy=w["t0_xy"], t0_z=w["t0_z"], t1_z=w["t1_z"],
             start_moved=w["start_moved"], in_face_plane=(dz == 0) & np.isin(s[:, 2], tops),
             at_slab_edge=(dz == 0) & ((s[:, 2] == g.zmin) | (s[:, 2] == g.zmax)))
    return {a: (int(b.sum()) if isinstance(b, np.ndarray) else b) for a, b in k.items()}


# ---------------------------------------------------------------------------------------------------------------- the families
def _rng(name, family):
    return np.random.default_rng(zlib.crc32(f"{name}/{family}".encode()))


def _sphere(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _cat(parts):
    s = np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 3) for p in parts]).astype(F)
    d = np.concatenate([np.asarray(p[1], np.float64).reshape(-1, 3) for p in parts]).astype(F)
    s[s == 0] = 0.0  # (no -0: the exact families compare bits, and 0 + (-0) is +0 in the kernel's start + pos_w)
    assert np.isfinite(s).all() and np.isfinite(d).all() and float(np.abs(s).max()) <= 2.0e6 and len(s) <= MAX_RAYS
    assert (d != 0).any(1).all()
    return s, d


def _fam_random(c: Case, g: Grid, rng, n=4096):
    x0, x1, y0, y1 = c.region
    o = np.stack([rng.uniform(x0 - 2, x1 + 2, n), rng.uniform(y0 - 2, y1 + 2, n), rng.uniform(float(g.zmin) - 1, float(g.zmax) + 3, n)], 1)
    return _cat([(o, _sphere(rng, n))])


def _heights(g: Grid):
    """zmin, zmax, the box tops (at most six, or two vertex-free stand-ins between zmin and zmax), each +-1 ulp and +-3 mm."""
    base = [g.zmin, g.zmax] + [F(z) for z in (g.tops[:: max(1, len(g.tops) // 6)][:6] if g.tops else (0.5 * (float(g.zmin) + float(g.zmax)),))]
    out = []
    for z in base:
        out += [z, np.nextafter(z, F(np.inf)), np.nextafter(z, F(-np.inf)), F(float(z) + 3.0e-3), F(float(z) - 3.0e-3)]
    return np.asarray(out, F)


def _fam_axis(c: Case, g: Grid, rng):
    X0, X1, Y0, Y1, zl, zh = float(g.x0), g.mx1, float(g.y0), g.my1, float(g.zmin), float(g.zmax)
    parts = []

    def inside(n, grow=1.0):
        return np.stack([rng.uniform(X0 - grow, X1 + grow, n), rng.uniform(Y0 - grow, Y1 + grow, n), rng.uniform(zl - 0.5, zh + 1.0, n)], 1)

    # one horizontal component zero, the other not; dz zero in a third of them
    for comp in (0, 1):
        n = 192
        o = inside(n)
        o[:, comp] = rng.uniform((X0, Y0)[comp], (X1, Y1)[comp], n)  # inside the grid on the axis that does not move
        d = np.zeros((n, 3))
        d[:, 1 - comp] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)
        d[:, 2] = rng.choice([0.0, -0.3, 0.4, -1.0, 1.0e-3, -2.0e-2], n)
        parts.append((o, d))
    # dx == dy == 0 in both signs (cast_ray itself): from above, from below, from inside the slab
    n = 128
    o = inside(n, 0.3)
    d = np.zeros((n, 3))
    d[:, 2] = np.where(np.arange(n) % 2 == 0, -1.0, 1.0) * rng.choice([1.0, 0.5], n)
    o[:, 2] = np.where(np.arange(n) % 4 < 2, np.where(d[:, 2] < 0, zh + 1.0, zl - 1.0), o[:, 2])
    parts.append((o, d))
    # a zero component with the origin outside the grid on that axis (1 ulp and 1 m outside), and exactly on its first and last line
    for comp, (lo, hi) in ((0, (g.x0, g.x1)), (1, (g.y0, g.y1))):
        edge = [np.nextafter(lo, F(-np.inf)), F(float(lo) - 1.0), np.nextafter(hi, F(np.inf)), F(float(hi) + 1.0), lo, hi]
        edge = np.asarray([e for e in edge if abs(float(e)) <= 2.0e6], np.float64)  # (the plane's grid ends at 3e6: its near side only)
        n = 16 * len(edge)
        o = inside(n)
        o[:, comp] = np.tile(edge, 16)
        d = np.zeros((n, 3))
        d[:, 1 - comp] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)
        d[:, 2] = rng.choice([0.0, -0.2, -1.0], n)
        parts.append((o, d))
    # dz == 0 at the slab's edges and the box tops, +-1 ulp, +-3 mm: along the axes and oblique
    hs = _heights(g)
    for k in range(8):
        n = len(hs)
        o = inside(n)
        o[:, 2] = hs
        a = rng.uniform(0, 2 * math.pi, n)
        d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)
        if k < 4:
            d[:] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)][k]
            o[:, 1 - k // 2] = rng.uniform((Y0, X0)[k // 2], (Y1, X1)[k // 2], n)
        parts.append((o, d))
    # denormal and 1e-30 components beside a unit one
    den, sub = 1.0e-40, float(np.finfo(F).smallest_subnormal)
    tiny = [(1, 1e-30, 0), (1e-30, 1, 0), (1, 0, 1e-30), (1, den, -den), (den, -1, 1e-30), (1e-30, 1e-30, -1), (sub, 0, 1), (0, sub, -1),
            (-den, den, -1), (1, -1e-30, -0.5), (-1e-30, -1, -0.5), (den, 1, -0.1), (-1, -den, 0), (sub, sub, -1), (1, 1, sub), (-1, 1e-30, -1e-30)]
    for _ in range(6):
        o = inside(len(tiny), 0.2)
        o[:, 2] = rng.choice([zh + 0.7, zl - 0.7, 0.5 * (zl + zh)], len(tiny))
        d = np.asarray(tiny, np.float64)
        d[:, 2] = np.where((o[:, 2] < zl) & (np.abs(d[:, 2]) == 1), 1.0, d[:, 2])
        parts.append((o, d))
    return _cat(parts)


def _line_ks(n, rng):
    """Line indices 0 .. n: the first, the last two, every tile line near the ends, the last tile line of a grid that is no multiple of 8."""
    ks = {0, 1, n - 1, n, 7, 8, 9, 16, 8 * ((n - 1) // 8), 8 * ((n - 1) // 8) - 8} | set(int(k) for k in rng.integers(0, n + 1, 4))
    return sorted(k for k in ks if 0 <= k <= n)


def _fam_gridline(c: Case, g: Grid, rng):
    zl, zh = float(g.zmin), float(g.zmax)
    kx, ky = _line_ks(g.nx, rng), _line_ks(g.ny, rng)
    lx, ly = np.asarray([g.line_x(k) for k in kx], F), np.asarray([g.line_y(k) for k in ky], F)
    lx, ly = lx[np.abs(lx) < 1.9e6], ly[np.abs(ly) < 1.9e6]  # (the plane's last line lies at 3e6)
    S, D = [], []
    a = float(F(math.sqrt(0.5)))
    a_up, a_dn = float(np.nextafter(F(a), F(1))), float(np.nextafter(F(a), F(0)))
    for shift in SHIFTS:
        off = F(shift * TAU * float(g.cell))
        sx, sy = (lx + off).astype(F), (ly + off).astype(F)  # fp32 sums, as the kernel adds
        # along the lines: on an x-line moving in y, on a y-line moving in x
        for axis, lines, (lo, hi) in ((0, sx, (float(g.y0), g.my1)), (1, sy, (float(g.x0), g.mx1))):
            for v in lines:
                for sign in (-1.0, 1.0):
                    for dz in (0.0, -0.3, -1.5):
                        o = np.zeros(3)
                        o[axis] = v
                        o[1 - axis] = rng.uniform(lo - 0.5, hi + 0.5)
                        o[2] = rng.uniform(zl, zh) if dz == 0.0 else zh + rng.uniform(0.2, 1.0)
                        d = np.zeros(3)
                        d[1 - axis], d[2] = sign, dz
                        S.append(o), D.append(d)
        # from the nodes: exact diagonals and 1 ulp off them
        for _ in range(12):
            i, j = int(rng.integers(len(sx))), int(rng.integers(len(sy)))
            for qx, qy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                for ddy in (a, a_up, a_dn):
                    for dz in (0.0, -0.3, -1.5):
                        S.append((sx[i], sy[j], rng.uniform(zl, zh) if dz == 0.0 else zh + rng.uniform(0.2, 1.0)))
                        D.append((qx * a, qy * ddy, dz))
    return _cat([(np.asarray(S, np.float64), np.asarray(D, np.float64))])


def _targets(c: Case, rng, n):
    """n mesh vertices, n edge midpoints, n face centroids, and up to n of the three from horizontal faces alone."""
    v64 = c.verts.astype(np.float64)
    tri = v64[c.tris]
    f = rng.integers(0, len(tri), n)
    e = rng.integers(0, 3, n)
    pts = [v64[c.tris[rng.integers(0, len(tri), n), rng.integers(0, 3, n)]], 0.5 * (tri[f, e] + tri[f, (e + 1) % 3]), tri[rng.integers(0, len(tri), n)].mean(1)]
    hf = horizontal_faces(c).astype(np.float64)
    if len(hf):
        f = rng.integers(0, len(hf), n)
        third = n // 3
        pts += [hf[f[:third], 0], 0.5 * (hf[f[third:2 * third], 1] + hf[f[third:2 * third], 2]), hf[f[2 * third:]].mean(1)]
    return np.concatenate(pts).astype(F).astype(np.float64)  # (the targets as fp32 numbers: a horizontal face's height stays exact)


def _fam_grazing(c: Case, g: Grid, rng, n=128):
    T = _targets(c, rng, n)
    m = len(T)
    cx, cy = 0.5 * (float(g.x0) + g.mx1), 0.5 * (float(g.y0) + g.my1)
    half = 0.5 * math.hypot(g.mx1 - float(g.x0), g.my1 - float(g.y0))
    # beyond the mesh's half diagonal by more than a cell's diagonal: outside the grid's box (but for the 2e6 m cell of the plane, whose
    # grid reaches 2e6 m past the mesh on the far sides: there the rays from the near sides are the ones with an xy clip)
    th, r = rng.uniform(0, 2 * math.pi, m), half + rng.uniform(1.0, 3.0, m)
    oxy = np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)
    zl, zh = float(g.zmin), float(g.zmax)
    parts = []
    for oz in (rng.uniform(zl - 1, zh + 3, m), T[:, 2].copy(), np.full(m, zh + 50.0), np.full(m, zl - 5.0)):
        o = np.concatenate([oxy, oz[:, None]], 1).astype(F).astype(np.float64)
        d = T - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        parts.append((o, d))
    s, d = _cat(parts)
    assert (d[m:2 * m, 2] == 0).all() and (s[m:2 * m, 2] == T[:, 2].astype(F)).all()
    return s, d


def _fam_long(c: Case, g: Grid, rng):
    X0, X1, Y0, Y1, zl, zh = float(g.x0), g.mx1, float(g.y0), g.my1, float(g.zmin), float(g.zmax)
    S, D = [], []
    slopes = [(qx * px, qy * py) for px, py in ((1, 1), (3, 1), (1, 3)) for qx in (-1, 1) for qy in (-1, 1)]
    for ux, uy in slopes:
        nrm = F(1.0 / math.hypot(ux, uy))
        dx, dy = float(F(ux) * nrm), float(F(uy) * nrm)  # (|dx| == |dy| on the diagonals, whatever the rounding)
        for ratio in np.logspace(-4, -1, 7):
            for sign in (-1.0, 1.0):
                for _ in range(8):
                    px, py = rng.uniform(X0, X1), rng.uniform(Y0, Y1)
                    back = min((px - X0) / dx if dx > 0 else (X1 - px) / -dx, (py - Y0) / dy if dy > 0 else (Y1 - py) / -dy) + 0.5
                    S.append((px - back * dx, py - back * dy, rng.uniform(zl - 0.05, zh + 0.05)))
                    D.append((dx, dy, sign * ratio))
    n = 512  # sky rays from inside the footprint
    o = np.stack([rng.uniform(X0, X1, n), rng.uniform(Y0, Y1, n), rng.uniform(zl - 0.5, zh + 0.5, n)], 1)
    d = _sphere(rng, n)
    d[:, 2] = np.abs(d[:, 2]) + 0.05
    return _cat([(np.asarray(S), np.asarray(D)), (o, d)])


_FAMILY = {"random": _fam_random, "axis": _fam_axis, "gridline": _fam_gridline, "grazing": _fam_grazing, "long": _fam_long}


def make_rays(name: str, family: str, count: int | None = None):
    """A fresh build of the family's rays for the case: (starts, dirs), (R, 3) fp32.  ``count``: that many rays of the random family."""
    c = walk_cases()[name]
    if count is not None:
        assert family == "random"
        return _fam_random(c, grid_of(name), _rng(name, f"random{count}"), count)
    return _FAMILY[family](c, grid_of(name), _rng(name, family))


@functools.lru_cache(maxsize=8)
def rays(name: str, family: str, count: int | None = None):
    s, d = make_rays(name, family, count)
    s.setflags(write=False), d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=8)
def brute_1e6(name: str, family: str):
    """The brute force's own t at max_distance 1e6, computed once and left unchanged."""
    c = walk_cases()[name]
    s, d = rays(name, family)
    h, t, _ = raycast_woop_f32(c.verts, c.tris, s, d, 1.0e6)
    h.setflags(write=False), t.setflags(write=False)
    return h, t


def hit_distances(name: str, family: str):
    """(ray, t, nextafter(t, 0), nextafter(t, inf)) of a chosen hit ray of the family: the median hit among those with 1e-3 < t < 1e5."""
    _, t = brute_1e6(name, family)
    cand = np.flatnonzero(np.isfinite(t) & (t > 1.0e-3) & (t < 1.0e5))
    assert len(cand), f"{name}/{family}: the brute force has no hit to take a distance from"
    r = int(cand[np.argsort(t[cand], kind="stable")[len(cand) // 2]])
    return r, float(t[r]), float(np.nextafter(t[r], F(0))), float(np.nextafter(t[r], F(np.inf)))


def distances(name: str, family: str):
    """The max_distance values the family runs at."""
    if family not in DISTANCE_FAMILIES:
        return [1.0e6]
    _, t, below, above = hit_distances(name, family)
    return [1.0e6, 10.0, 0.0, t, below, above]


# ---------------------------------------------------------------------------------------------------------------- the harness
_MESH = [None, None]


def mesh_of(name: str):
    """The case's TerrainMesh (one kept at a time: the tests run case by case)."""
    if _MESH[0] != name:
        from isaaclab_amd.env import TerrainMesh

        _MESH[0], _MESH[1] = None, None
        c = walk_cases()[name]
        _MESH[1] = TerrainMesh(c.verts, c.tris, c.cell)
        _MESH[0] = name
        g = grid_of(name)
        assert (_MESH[1].nx, _MESH[1].ny, _MESH[1].cell_size) == (g.nx, g.ny, float(g.cell)), (name, _MESH[1].nx, _MESH[1].ny, g)
    return _MESH[1]


def sensor_cfg(R: int, max_distance: float) -> dict:
    return {"pattern_cfg": {"func": "isaaclab.sensors.ray_caster.patterns.patterns:grid_pattern", "resolution": 1.0, "size": [float(R - 1), 0.0],
                            "direction": (0.0, 0.0, -1.0)},
            "offset": {"pos": (0.0, 0.0, 0.0), "rot": (1.0, 0.0, 0.0, 0.0)}, "attach_yaw_only": True, "max_distance": float(max_distance),
            "update_period": 0.0, "drift_range": (0.0, 0.0)}


def feed_sensor(mesh, starts, dirs, max_distance, positions=None):
    """A RayCaster on ``mesh`` whose local pattern is ``starts`` / ``dirs`` as they are, updated once with an identity quaternion and
    ``positions`` ((N, 3), default one env at zero).  ``ray_hits_w`` is pre-filled with NaN: every ray of every env must be written."""
    import torch

    from isaaclab_amd.producers import RayCaster

    R = len(starts)
    pos = np.zeros((1, 3), F) if positions is None else np.ascontiguousarray(positions, F)
    N = len(pos)
    s = RayCaster(sensor_cfg(R, max_distance), N, "cuda", mesh, keep_world_rays=True)
    assert s.num_rays == R and tuple(s.ray_starts.shape) == (R, 3) and s.cfg.attach_yaw_only
    s.ray_starts.copy_(torch.from_numpy(np.array(starts, F)))  # (a writable copy: the cached rays are read-only)
    s.ray_directions.copy_(torch.from_numpy(np.array(dirs, F)))
    s._data.ray_hits_w.fill_(float("nan"))
    quat = torch.zeros(N, 4)
    quat[:, 0] = 1.0
    s.update(0.02, torch.from_numpy(pos).cuda(), quat.cuda(), force_recompute=True)
    return s


def run_walk_case(case: Case, family: str, max_distance: float = 1.0e6, product: bool = True, *, count: int | None = None, positions=None):
    """One family of rays on one case at one max_distance.  ``product``: through the sensor, with the three assertions of
    test_walk_is_bit_identical_to_the_exhaustive_search on every ray (and, for the exact families, the fed rays back bit for bit);
    ``product=False`` puts ``raycast_woop_f32`` in the sensor's place.  Returns the figures: rays, hits, misses, t32, the edge counts."""
    name = case.name
    s0, d0 = rays(name, family, count)
    R = len(s0)
    pos = np.zeros((1, 3), F) if positions is None else np.ascontiguousarray(positions, F)
    N = len(pos)
    what = f"{name}/{family} R={R} N={N} max_distance={max_distance!r}"
    sensor = None
    if product:
        sensor = feed_sensor(mesh_of(name), s0, d0, max_distance, positions)
        sw, dw = sensor.ray_starts_w.cpu().numpy().reshape(-1, 3), sensor.ray_directions_w.cpu().numpy().reshape(-1, 3)
        hits = sensor._data.ray_hits_w.cpu().numpy().reshape(-1, 3)
        assert not np.isnan(hits).any(), f"{what}: {int(np.isnan(hits).any(1).sum())} rays were never written"
        assert np.array_equal(dw.view(np.uint32), np.tile(d0, (N, 1)).view(np.uint32)), f"{what}: the directions did not reach the kernel as fed"
        if positions is None and family in EXACT:
            assert np.array_equal(sw.view(np.uint32), s0.view(np.uint32)), f"{what}: the starts did not reach the kernel as fed"
    else:
        sw, dw = (s0[None] + pos[:, None, :]).astype(F).reshape(-1, 3), np.tile(d0, (N, 1))
    if positions is None and max_distance == 1.0e6 and count is None and np.array_equal(sw.view(np.uint32), s0.view(np.uint32)):
        h32, t32 = brute_1e6(name, family)
    else:
        h32, t32, _ = raycast_woop_f32(case.verts, case.tris, sw, dw, max_distance)
    hit = np.isfinite(t32)
    if not product:
        hits = h32

    d2 = None
    if product:  # (before the assertions, so that a failure says which of the two walks it is)
        h2, d2, _, _ = sensor.mesh.raycast(sensor.ray_starts_w, sensor.ray_directions_w, max_distance, return_distance=True)
        d2, h2 = d2.cpu().numpy().reshape(-1), h2.cpu().numpy().reshape(-1, 3)

    def show(rows):
        """(ray, start, direction, the brute force's t, the sensor's hit point, cast_ray's t) of the first four"""
        return [(int(i), sw[i].tolist(), dw[i].tolist(), float(t32[i]), hits[i].tolist(), None if d2 is None else float(d2[i])) for i in rows[:4]]

    # 1. the miss mask: +inf in all three components on a miss, finite in all three on a hit
    bad = np.flatnonzero((np.isposinf(hits).all(1) != ~hit) | (np.isfinite(hits).all(1) != hit))
    assert bad.size == 0, f"{what}: {bad.size} rays differ from the brute force in hit / miss: {show(bad)}"
    # 2. ray_hits_w = start + t32 * dir in fp32 with the brute force's t32, bit for bit
    want = (sw[hit] + t32[hit, None] * dw[hit]).astype(F)
    bad = np.flatnonzero(hit)[(hits[hit].view(np.uint32) != want.view(np.uint32)).any(1)]
    assert bad.size == 0, f"{what}: {bad.size} hit points differ from start + t32 dir: {show(bad)}"
    # 3. the unpruned cast_ray on the same world rays: the same mask, the same distances, the same hit points
    if product:
        bad = np.flatnonzero(np.isfinite(d2) != hit)
        assert bad.size == 0, f"{what}: cast_ray differs from the brute force in hit / miss on {bad.size} rays: {show(bad)}"
        bad = np.flatnonzero(hit)[d2[hit].view(np.uint32) != t32[hit].view(np.uint32)]
        assert bad.size == 0, f"{what}: cast_ray's distances differ from t32 on {bad.size} rays: {show(bad)}"
        assert np.array_equal(h2[hit].view(np.uint32), hits[hit].view(np.uint32)), f"{what}: cast_ray's hit points differ from the sensor's"
    fig = dict(rays=len(sw), hits=int(hit.sum()), misses=int((~hit).sum()), t32=t32, hit_fraction=float(hit.mean()), sensor=sensor,
               kinds=edge_kinds(name, sw, dw))  # (of the world rays the cast used)
    print(f"[walk] {what}: {fig['hits']} hits, {fig['misses']} misses, hit fraction {fig['hit_fraction']:.3f}", flush=True)
    return fig
