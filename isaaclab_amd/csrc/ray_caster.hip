// RayCaster (isaaclab/sensors/ray_caster/ray_caster.py:107-114,220-260 under SensorBase, sensors/sensor_base.py:182-205,287-296) in one
// launch: reset, clocks, and for the outdated envs the sensor pose, the world rays, the cast and the optional range image.  Any ray
// pattern (plan.py: bpearl_pattern, lidar_pattern, grid_pattern), full orientation or yaw only.  The cast is cast_ray_pruned
// (imx_ray_walk.h); its z-bounds are built here, once per mesh, from the device-resident cell records, reference lists and triangle
// records (imx_mesh_build_ray_bounds).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "imx_internal.h"
#include "imx_ray_walk.h"

// ------------------------------------------------------------------------------------------------- the bounds
// (ix, iy) of linear cell index c in the 8x8-tiled layout (the inverse of imx_cell_index)
IMX_DEV void cell_xy(int c, int ntx, int& ix, int& iy) {
    const int tile = c >> 6;
    ix = ((tile % ntx) << 3) | (c & 7);
    iy = ((tile / ntx) << 3) | ((c >> 3) & 7);
}

// pass 1: the z-range of what test_cell (imx_raycast.h) tests in this cell: the four corner heights of a LATTICE cell, every triangle
// record of a QH / GENERAL cell's reference list
__global__ void k_ray_bounds_cell(MeshView M, int ncell, float2* __restrict__ raw) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    int ix, iy;
    cell_xy(c, M.ntx, ix, iy);
    const float inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    if (ix < M.nx && iy < M.ny) {
        const int4 b4 = M.cells[2 * (size_t)c + 1];
        const int kind = b4.x & 0xFF;
        if (kind == IMX_CELL_LATTICE) {
            const int4 a4 = M.cells[2 * (size_t)c];
            const float za = __int_as_float(a4.x), zd = __int_as_float(a4.y), zc = __int_as_float(a4.z), zb = __int_as_float(a4.w);
            lo = fminf(fminf(za, zd), fminf(zc, zb));
            hi = fmaxf(fmaxf(za, zd), fmaxf(zc, zb));
        } else if (kind != IMX_CELL_EMPTY) {
            const int2 g = M.cell_list[c];
            for (int k = g.x; k < g.x + g.y; k += 2) {
                const int4 rr = M.refs[k >> 1];
                for (int h = 0; h < 2; ++h) {
                    const float4* q = M.tri_rec + (size_t)(h ? rr.z : rr.x) * 3;
                    const float az = q[0].z, bz = q[1].y, cz = q[2].x;  // ax ay az bx | by bz cx cy | cz face ztop 0
                    lo = fminf(lo, fminf(az, fminf(bz, cz)));
                    hi = fmaxf(hi, fmaxf(az, fmaxf(bz, cz)));
                }
            }
        }
    }
    raw[c] = make_float2(lo, hi);
}

// pass 2: a visit of cell (ix, iy) tests the lists of its 3x3 block
__global__ void k_ray_bounds_dilate(int ntx, int nx, int ny, int ncell, const float2* __restrict__ raw, float2* __restrict__ cell_z) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    int ix, iy;
    cell_xy(c, ntx, ix, iy);
    const float inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    if (ix < nx && iy < ny) {
        for (int jy = -1; jy <= 1; ++jy)
            for (int jx = -1; jx <= 1; ++jx) {
                const int x = ix + jx, y = iy + jy;
                if (x < 0 || y < 0 || x >= nx || y >= ny) continue;
                const float2 b = raw[imx_cell_index(x, y, ntx)];
                lo = fminf(lo, b.x);
                hi = fmaxf(hi, b.y);
            }
    }
    cell_z[c] = make_float2(lo, hi);
}

// pass 3: the 64 cells of a tile
__global__ void k_ray_bounds_tile(int ntile, const float2* __restrict__ cell_z, float2* __restrict__ tile_z) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntile) return;
    const float inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    for (int k = 0; k < 64; ++k) {
        const float2 b = cell_z[(size_t)t * 64 + k];
        lo = fminf(lo, b.x);
        hi = fmaxf(hi, b.y);
    }
    tile_z[t] = make_float2(lo, hi);
}

extern "C" int imx_mesh_build_ray_bounds(imx_mesh_t* m, imx_stream_t stream, int64_t* info4) {
    IMX_REQUIRE(m, "imx_mesh_build_ray_bounds: null mesh");
    const int ntile = m->v.ntx * m->v.nty, ncell = ntile * 64;
    int64_t took = 0;
    if (!m->d_ray_cell_z) {
        IMX_REQUIRE(m->d_cell && ntile > 0, "imx_mesh_build_ray_bounds: the mesh has no device tables (no GPU visible when it was created)");
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        IMX_HIP(hipStreamIsCapturing((hipStream_t)stream, &cs));
        IMX_REQUIRE(cs == hipStreamCaptureStatusNone, "imx_mesh_build_ray_bounds: the bounds of this mesh do not exist yet and cannot be built "
                    "inside a stream capture (the build allocates and synchronises): call it, or imx_ray_caster, once before capturing");
        const auto t_start = std::chrono::steady_clock::now();
        float2 *raw = nullptr, *cell_z = nullptr, *tile_z = nullptr;
        IMX_HIP(hipMalloc((void**)&raw, (size_t)ncell * sizeof(float2)));
        if (hipMalloc((void**)&cell_z, (size_t)ncell * sizeof(float2)) != hipSuccess || hipMalloc((void**)&tile_z, (size_t)ntile * sizeof(float2)) != hipSuccess) {
            (void)hipFree(raw);
            if (cell_z) (void)hipFree(cell_z);
            IMX_FAIL("imx_mesh_build_ray_bounds: out of device memory for %d cells", ncell);
        }
        hipStream_t s = (hipStream_t)stream;
        hipLaunchKernelGGL(k_ray_bounds_cell, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s, m->v, ncell, raw);
        hipLaunchKernelGGL(k_ray_bounds_dilate, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s, m->v.ntx, m->v.nx, m->v.ny, ncell, raw, cell_z);
        hipLaunchKernelGGL(k_ray_bounds_tile, dim3((unsigned)((ntile + 255) / 256)), dim3(256), 0, s, ntile, cell_z, tile_z);
        std::vector<float2> h((size_t)ntile);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h.data(), tile_z, (size_t)ntile * sizeof(float2), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(raw);
        if (e != hipSuccess) {
            (void)hipFree(cell_z);
            (void)hipFree(tile_z);
            IMX_FAIL("imx_mesh_build_ray_bounds: %s", hipGetErrorString(e));
        }
        float zmin = INFINITY, zmax = -INFINITY;
        for (const float2& b : h) {
            zmin = std::min(zmin, b.x);
            zmax = std::max(zmax, b.y);
        }
        m->d_ray_cell_z = reinterpret_cast<float*>(cell_z);
        m->d_ray_tile_z = reinterpret_cast<float*>(tile_z);
        m->ray_zmin = zmin;
        m->ray_zmax = zmax;
        took = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_start).count();
        m->ray_bounds_ns = took;
    }
    if (info4) {
        info4[0] = ((int64_t)ncell + ntile) * (int64_t)sizeof(float2);
        info4[1] = took;
        info4[2] = ncell;
        info4[3] = ntile;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------- the sensor
// One block per env.  Thread 0 is the env's SensorBase: reset, clocks, the decision to refresh, the sensor pose; the block's threads
// then take the rays, neighbouring rays of the pattern in neighbouring lanes.  An env that is not refreshed leaves after the barrier and
// keeps its hits.
__global__ void __launch_bounds__(256) k_ray_caster(imx_ray_caster_t c, MeshView M, RayBoundsView Z) {
    const int64_t e = blockIdx.x;
    __shared__ float s_pose[8];  // pos_w xyz, the rotation's w x y z (the yaw quaternion's for attach_yaw_only)
    __shared__ int s_go;
    if (threadIdx.x == 0) {
        float ts = c.timestamp_d[e], last = c.timestamp_last_update_d[e];
        bool outdated = c.is_outdated_d[e] != 0;
        if (c.reset_mask_d && c.reset_mask_d[e]) {  // SensorBase.reset, then RayCaster.reset: drift.uniform_(lo, hi)
            ts = 0.0f; last = 0.0f; outdated = true;
            const uint32_t step = (uint32_t)c.reset_count_d[e];
            const float w = c.drift_hi - c.drift_lo;
            for (int k = 0; k < 3; ++k) {
                const float u = c.uniforms_d ? c.uniforms_d[e * 3 + k] : uniform01(c.seed ^ 0x4C1DA2ull, step, (uint64_t)e * 3 + k);
                c.drift_d[e * 3 + k] = u * w + c.drift_lo;
            }
            c.reset_count_d[e] = (int32_t)(step + 1u);
        }
        for (int k = 0; k < c.substeps; ++k) {  // SensorBase.update(dt), fp32 like the tensors
            ts = ts + c.dt;
            outdated = outdated || (ts - last + 1.0e-6f >= c.update_period);
        }
        const bool go = outdated && c.refresh != 0;
        if (go) {  // _update_buffers_impl: the pose; _update_outdated_buffers: last update <- timestamp, no longer outdated
            const float px = c.body_pos_w_d[e * 3] + c.drift_d[e * 3], py = c.body_pos_w_d[e * 3 + 1] + c.drift_d[e * 3 + 1],
                        pz = c.body_pos_w_d[e * 3 + 2] + c.drift_d[e * 3 + 2];
            const float4 q = reinterpret_cast<const float4*>(c.body_quat_w_d)[e];
            c.pos_w_d[e * 3] = px; c.pos_w_d[e * 3 + 1] = py; c.pos_w_d[e * 3 + 2] = pz;
            reinterpret_cast<float4*>(c.quat_w_d)[e] = q;
            s_pose[0] = px; s_pose[1] = py; s_pose[2] = pz;
            if (c.attach_yaw_only) {
                float yw, yz;
                yaw_quat_wz(q.x, q.y, q.z, q.w, yw, yz);
                s_pose[3] = yw; s_pose[4] = 0.0f; s_pose[5] = 0.0f; s_pose[6] = yz;
            } else {
                s_pose[3] = q.x; s_pose[4] = q.y; s_pose[5] = q.z; s_pose[6] = q.w;
            }
            last = ts;
            outdated = false;
        }
        c.timestamp_d[e] = ts;
        c.timestamp_last_update_d[e] = last;
        c.is_outdated_d[e] = outdated ? 1 : 0;
        s_go = go ? 1 : ((c.refresh != 0 && c.ranges_d) ? 2 : 0);
    }
    __syncthreads();
    if (!s_go) return;
    if (s_go == 2) {  // not refreshed, but a range image is asked for (possibly with another clip): from the hits and pos_w the env keeps
        const float kx = c.pos_w_d[e * 3], ky = c.pos_w_d[e * 3 + 1], kz = c.pos_w_d[e * 3 + 2];
        for (int j = threadIdx.x; j < c.num_rays; j += blockDim.x) {
            const size_t o = ((size_t)e * c.num_rays + j) * 3;
            const float ex = c.ray_hits_w_d[o] - kx, ey = c.ray_hits_w_d[o + 1] - ky, ez = c.ray_hits_w_d[o + 2] - kz;
            c.ranges_d[(size_t)e * c.num_rays + j] = fminf(sqrtf((ex * ex + ey * ey) + ez * ez), c.range_clip);
        }
        return;
    }
    const float px = s_pose[0], py = s_pose[1], pz = s_pose[2], qw = s_pose[3], qx = s_pose[4], qy = s_pose[5], qz = s_pose[6];
    const float inf = __builtin_huge_valf();
    for (int j = threadIdx.x; j < c.num_rays; j += blockDim.x) {
        const float lx = c.ray_starts_d[j * 3], ly = c.ray_starts_d[j * 3 + 1], lz = c.ray_starts_d[j * 3 + 2];
        float dx = c.ray_directions_d[j * 3], dy = c.ray_directions_d[j * 3 + 1], dz = c.ray_directions_d[j * 3 + 2];
        float sx, sy, sz;
        if (c.attach_yaw_only) {  // quat_apply_yaw(quat_w, start) + pos_w; the directions stay as they are
            quat_apply_yaw_only(qw, qz, lx, ly, lz, sx, sy, sz);
        } else {                  // quat_apply on both
            quat_apply(qw, qx, qy, qz, lx, ly, lz, sx, sy, sz);
            const float ux = dx, uy = dy, uz = dz;
            quat_apply(qw, qx, qy, qz, ux, uy, uz, dx, dy, dz);
        }
        sx = sx + px; sy = sy + py; sz = sz + pz;
        float t;
        int32_t f;
        const bool hit = cast_ray_pruned(M, Z, sx, sy, sz, dx, dy, dz, c.max_distance, t, f);
        const float hx = hit ? sx + t * dx : inf, hy = hit ? sy + t * dy : inf, hz = hit ? sz + t * dz : inf;
        const size_t o = ((size_t)e * c.num_rays + j) * 3;
        c.ray_hits_w_d[o] = hx; c.ray_hits_w_d[o + 1] = hy; c.ray_hits_w_d[o + 2] = hz;
        if (c.ranges_d) {  // min(||ray_hits_w - pos_w||, clip); a miss (+inf) gives the clip
            const float ex = hx - px, ey = hy - py, ez = hz - pz;
            c.ranges_d[(size_t)e * c.num_rays + j] = fminf(sqrtf((ex * ex + ey * ey) + ez * ez), c.range_clip);
        }
        if (c.ray_starts_w_d) { c.ray_starts_w_d[o] = sx; c.ray_starts_w_d[o + 1] = sy; c.ray_starts_w_d[o + 2] = sz; }
        if (c.ray_directions_w_d) { c.ray_directions_w_d[o] = dx; c.ray_directions_w_d[o + 1] = dy; c.ray_directions_w_d[o + 2] = dz; }
    }
}

extern "C" int imx_ray_caster(const imx_ray_caster_t* rc, int64_t N, imx_mesh_t* mesh, imx_stream_t stream) {
    IMX_REQUIRE(rc && mesh, "imx_ray_caster: null argument");
    IMX_REQUIRE(N > 0 && N < (1ll << 31), "imx_ray_caster: N out of range");
    IMX_REQUIRE(rc->num_rays > 0 && rc->num_rays <= (1 << 20) && (int64_t)rc->num_rays * N < (1ll << 40), "imx_ray_caster: num_rays %d out of range", rc->num_rays);
    IMX_REQUIRE(rc->substeps >= 0 && rc->substeps <= 1024, "imx_ray_caster: substeps %d outside [0, 1024]", rc->substeps);
    IMX_REQUIRE(rc->dt >= 0.0f && rc->update_period >= 0.0f, "imx_ray_caster: negative dt or update_period");
    IMX_REQUIRE(rc->max_distance >= 0.0f, "imx_ray_caster: max_distance %g", (double)rc->max_distance);
    IMX_REQUIRE(rc->drift_lo <= rc->drift_hi, "imx_ray_caster: drift_range (%g, %g)", (double)rc->drift_lo, (double)rc->drift_hi);
#define IMX_RC_NEED(field) IMX_REQUIRE(rc->field, "imx_ray_caster: " #field " missing")
    IMX_RC_NEED(ray_starts_d); IMX_RC_NEED(ray_directions_d); IMX_RC_NEED(body_pos_w_d); IMX_RC_NEED(body_quat_w_d); IMX_RC_NEED(reset_count_d);
    IMX_RC_NEED(timestamp_d); IMX_RC_NEED(timestamp_last_update_d); IMX_RC_NEED(is_outdated_d); IMX_RC_NEED(drift_d); IMX_RC_NEED(pos_w_d);
    IMX_RC_NEED(quat_w_d); IMX_RC_NEED(ray_hits_w_d);
#undef IMX_RC_NEED
    IMX_REQUIRE(((uintptr_t)rc->body_quat_w_d & 15) == 0 && ((uintptr_t)rc->quat_w_d & 15) == 0, "imx_ray_caster: body_quat_w_d / quat_w_d must be 16-byte aligned");
    IMX_REQUIRE(!rc->ranges_d || rc->range_clip >= 0.0f, "imx_ray_caster: range_clip %g", (double)rc->range_clip);
    if (!mesh->d_ray_cell_z && imx_mesh_build_ray_bounds(mesh, stream, nullptr)) return 1;
    RayBoundsView Z;
    Z.cell_z = reinterpret_cast<const float2*>(mesh->d_ray_cell_z);
    Z.tile_z = reinterpret_cast<const float2*>(mesh->d_ray_tile_z);
    Z.zmin = mesh->ray_zmin;
    Z.zmax = mesh->ray_zmax;
    // threads: the rays split evenly over as few passes of at most 256 as it takes, rounded up to whole waves (360 rays: 2 x 192)
    const int passes = (rc->num_rays + 255) / 256;
    const int threads = (((rc->num_rays + passes - 1) / passes) + 63) / 64 * 64;
    hipLaunchKernelGGL(k_ray_caster, dim3((unsigned)N), dim3((unsigned)threads), 0, (hipStream_t)stream, *rc, mesh->v, Z);
    IMX_HIP(hipGetLastError());
    return 0;
}
