// Closest hit of a GENERAL ray (any direction, any origin) against the terrain grid, with pruning in z.
//
// cast_ray (imx_raycast.h) walks the xy grid cell by cell and tests the 3x3 block of cell lists at every cell it visits: the right
// cost for the handful of cells a near-vertical ray crosses, not for a lidar ray that flies 20 m over the terrain before it comes down,
// or one that points at the sky and walks to the edge of the grid.  cast_ray_pruned visits the SAME cells in the same order, with the
// same per-triangle arithmetic (woop_setup / test_cell), and gives the same closest hit bit for bit; what is new is what it skips:
//
//   * the ray is clipped to the slab [zmin, zmax] of the whole mesh, as it is to the grid's x and y extent: a ray that points at the
//     sky stops where it leaves the slab, one that starts high above the terrain starts walking where it enters it;
//   * per 8x8 tile (the layout of imx_cell_index) and per cell, a z-range that covers every triangle of the 3x3 block of cell lists a
//     visit of that cell would test (RayBoundsView, built by ray_caster.hip: the cell's own range, dilated over its 3x3 block -- a
//     triangle missing from a cell it overlaps by less than IMX_GRID_TAU is in a neighbour's list, hence in the dilated range).  A
//     cell is skipped when the ray's z-interval over [t_enter, t_exit] of that cell misses its range; a tile likewise, over the ray's
//     stay in the tile (plus one cell's crossing time, see below), and then its cells are stepped over without a load.
//
// Why no hit is lost: a triangle that the Woop test accepts is crossed by the ray (up to rounding) at a point P inside the triangle, so
// P.z lies in the triangle's z-range.  The walk is in the cell c with t_enter <= t(P) <= t_exit at that moment; the existing walk finds
// the triangle in c's 3x3 block (its own premise), so the dilated range of c contains the triangle's, and the ray's z over
// [t_enter, t_exit] contains P.z: the two intervals meet and c is not skipped.  The ray's interval is widened by `slack` (1 mm + 1e-5
// relative in z + 1e-6 of the origin's xy distance to the far side of the grid) for the rounding of t, of the ray's z and of a grazing
// ray's hit parameter, which is a convex combination of the corners'.
#pragma once

#include "imx_raycast.h"

struct RayBoundsView {
    const float2* cell_z;  // (ntx*nty*64) {lowest, highest} z of the 3x3 block of cell lists, cell order of imx_cell_index; empty = {+inf, -inf}
    const float2* tile_z;  // (ntx*nty) the same over the 64 cells of a tile
    float zmin, zmax;      // of the whole mesh
};

IMX_DEV bool z_miss(float za, float zb, float slack, float2 b) {
    return fmaxf(za, zb) + slack < b.x || fminf(za, zb) - slack > b.y;
}

// Closest hit with t in [0, max_dist]; returns false on a miss.  Same result as cast_ray.
IMX_DEV bool cast_ray_pruned(const MeshView& m, const RayBoundsView& zb, float ox, float oy, float oz, float dx, float dy, float dz,
                             float max_dist, float& t_hit, int32_t& face) {
    if (dx == 0.0f && dy == 0.0f) return cast_ray(m, ox, oy, oz, dx, dy, dz, max_dist, t_hit, face);  // vertical: one cell (+ snapped neighbours)
    const WoopRay r = woop_setup(ox, oy, oz, dx, dy, dz);
    float best = max_dist;
    face = -1;
    const float gm = grid_margin(m, ox, oy);  // (the clip of cast_ray, see there)
    const float gx_lo = m.x0 - gm, gy_lo = m.y0 - gm, gx_hi = m.x0 + m.nx * m.cell + gm, gy_hi = m.y0 + m.ny * m.cell + gm;
    float t0 = 0.0f, t1 = max_dist;
    if (dx != 0.0f) {
        const float ta = (gx_lo - ox) / dx, tb = (gx_hi - ox) / dx;
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    } else if (ox < gx_lo || ox > gx_hi) {
        return false;
    }
    if (dy != 0.0f) {
        const float ta = (gy_lo - oy) / dy, tb = (gy_hi - oy) / dy;
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    } else if (oy < gy_lo || oy > gy_hi) {
        return false;
    }
    // the slab of the mesh in z, widened by the slack of the cell test (a ray is never clipped tighter than its cells are tested)
    // The hit parameter is t = sum w_i t_i over the corners' own parameters t_i = (corner - origin)[kz] / d[kz] with the computed weights
    // w_i; its rounding, times dz, is a height error of a few ulps of the largest |corner - origin| in x or y -- nothing on a terrain a
    // few tens of metres wide, 0.1 m on the 2e6 m ground plane, where a ray that starts a few centimetres past the plane and points
    // away is still a hit (t = 0) of the exhaustive search.  1e-6 (16 ulps) of the origin's distance to the far side of the grid
    const float far_xy = fmaxf(fmaxf(fabsf(ox - gx_lo), fabsf(ox - gx_hi)), fmaxf(fabsf(oy - gy_lo), fabsf(oy - gy_hi)));
    const float slack_xy = 1.0e-3f + 1.0e-6f * far_xy;
    const float slack0 = slack_xy + 1.0e-5f * (fabsf(oz) + fmaxf(fabsf(zb.zmin), fabsf(zb.zmax)));
    const float z_lo = zb.zmin - 2.0f * slack0, z_hi = zb.zmax + 2.0f * slack0;
    if (dz != 0.0f) {
        const float ta = (z_lo - oz) / dz, tb = (z_hi - oz) / dz;
        const float te = fminf(ta, tb), tx = fmaxf(ta, tb);
        // (1e-4 relative on the way in and out: the division's rounding must not move the clip inside the slab)
        t0 = fmaxf(t0, te - 1.0e-4f * fabsf(te));
        t1 = fminf(t1, tx + 1.0e-4f * fabsf(tx));
    } else if (oz < z_lo || oz > z_hi) {
        return false;
    }
    if (!(t0 <= t1)) return false;
    const float px = ox + t0 * dx, py = oy + t0 * dy;
    int ix = min(max((int)floorf((px - m.x0) * m.inv_cell), 0), m.nx - 1);
    int iy = min(max((int)floorf((py - m.y0) * m.inv_cell), 0), m.ny - 1);
    const int sx = dx > 0.0f ? 1 : -1, sy = dy > 0.0f ? 1 : -1;
    const float inf = __builtin_huge_valf();
    float tmx = inf, tmy = inf, tdx = inf, tdy = inf;
    if (dx != 0.0f) {
        const float bx = m.x0 + (ix + (sx > 0 ? 1 : 0)) * m.cell;
        tmx = (bx - ox) / dx;
        tdx = m.cell / fabsf(dx);
    }
    if (dy != 0.0f) {
        const float by = m.y0 + (iy + (sy > 0 ? 1 : 0)) * m.cell;
        tmy = (by - oy) / dy;
        tdy = m.cell / fabsf(dy);
    }
    float t_enter = t0;
    int tile = -1;           // the tile whose range was looked at last
    bool tile_out = false;   // ... and missed: its cells are stepped over
    const int max_steps = m.nx + m.ny + 2;
    for (int step = 0; step < max_steps; ++step) {
        if (ix < 0 || iy < 0 || ix >= m.nx || iy >= m.ny) break;
        if (t_enter > t1 || (face >= 0 && best < t_enter)) break;
        const float t_exit = fminf(tmx, tmy);
        const int tl = (iy >> 3) * m.ntx + (ix >> 3);
        if (tl != tile) {
            // the ray's stay in this tile ends at the tile's far line in x or y, whichever comes first (or where the ray ends)
            tile = tl;
            float tt = t1;
            if (dx != 0.0f) tt = fminf(tt, (m.x0 + (float)((((ix >> 3) + (sx > 0 ? 1 : 0)) << 3)) * m.cell - ox) / dx);
            if (dy != 0.0f) tt = fminf(tt, (m.y0 + (float)((((iy >> 3) + (sy > 0 ? 1 : 0)) << 3)) * m.cell - oy) / dy);
            // tmx / tmy are running sums: after hundreds of cells they lag or lead the directly computed tt by their accumulated rounding,
            // which stays below one cell (the premise of the walk itself: the 3x3 block covers one cell of error).  The walk's last
            // cell of this tile may therefore end up to one cell's crossing time after tt
            tt = fmaxf(tt + fminf(tdx, tdy), t_exit);
            const float za = oz + t_enter * dz, zc = oz + tt * dz;
            const float slack = slack_xy + 1.0e-5f * (fabsf(oz) + fabsf(za) + fabsf(zc));
            tile_out = z_miss(za, zc, 2.0f * slack, zb.tile_z[tl]);
        }
        if (!tile_out) {
            const float za = oz + t_enter * dz, zc = oz + fminf(t_exit, t1) * dz;
            const float slack = slack_xy + 1.0e-5f * (fabsf(oz) + fabsf(za) + fabsf(zc));
            if (!z_miss(za, zc, slack, zb.cell_z[imx_cell_index(ix, iy, m.ntx)])) {
                for (int jy = -1; jy <= 1; ++jy)
                    for (int jx = -1; jx <= 1; ++jx) test_cell(m, r, ix + jx, iy + jy, best, face);
            }
        }
        if (tmx < tmy) {
            t_enter = tmx;
            tmx += tdx;
            ix += sx;
        } else {
            t_enter = tmy;
            tmy += tdy;
            iy += sy;
        }
    }
    if (face < 0) return false;
    t_hit = best;
    return true;
}
