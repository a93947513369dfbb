// The pose-2d command for ONE env: CommandTerm.reset / compute (isaaclab/managers/command_manager.py:120-187) + UniformPose2dCommand
// (isaaclab/envs/mdp/commands/pose_2d_command.py:26-143) and TerrainBasedPose2dCommand (:146-203).  Included by imx_producers.h: shared
// by the stand-alone kernel (producers.hip) and the orchestration kernel (orchestrate.hip), and by the host program
// tools/pose2d_host.cpp -- this file compiles as gfx950 device code and as plain host C++.
#pragma once
#include <math.h>

#include "../../include/imx_pose2d_struct.h"
#include "imx_quat.h"

// column k of {time_left, pos_x, pos_y, heading} of one resampling: the recorded table or the counter-based generator (the seeds and
// columns scheme of u_at, imx_producers.h)
IMX_HD float pose2d_u_at(const float* U, int64_t e, int k, uint64_t seed, uint32_t step) {
    return U ? U[e * 4 + k] : uniform01(seed + 0x1234567ull * (uint64_t)(k + 1), step, (uint64_t)e);
}

// Same contract as velocity_command_env / pose_command_env.  `reset`: CommandTerm.reset for this env first (metrics logged and zeroed,
// counter zeroed, resample); `do_compute`: then CommandTerm.compute(dt) -- _update_metrics (the metrics are ASSIGNED), time_left -= dt,
// resample when it ran out, _update_command.  mpos0 / mhead0 receive error_pos_2d / error_heading as they stood BEFORE the reset (what
// CommandTerm.reset logs).  The terrain indices and the patch id are clamped to the table: a bad index reads a wrong patch, never
// memory outside valid_targets.
IMX_HD void pose2d_command_env(int64_t N, int64_t e, const imx_pose2d_command_t& c, float dt, int do_compute, const float* root_pos,
                               const float* root_quat, bool reset, uint64_t seed, uint32_t step, float& mpos0, float& mhead0) {
    const float PI = 3.14159265358979323846f;
    const float qw = root_quat[e * 4], qx = root_quat[e * 4 + 1], qy = root_quat[e * 4 + 2], qz = root_quat[e * 4 + 3];
    const float rx = root_pos[e * 3], ry = root_pos[e * 3 + 1], rz = root_pos[e * 3 + 2];
    float fx, fy, fz;
    quat_apply(qw, qx, qy, qz, 1.0f, 0.0f, 0.0f, fx, fy, fz);  // heading_w (articulation_data.py:518-526)
    const float heading = atan2f(fy, fx);
    float pwx = c.pos_command_w_d[e * 3], pwy = c.pos_command_w_d[e * 3 + 1], pwz = c.pos_command_w_d[e * 3 + 2];
    float hw = c.heading_command_w_d[e];
    float tl = c.time_left_d[e];
    int64_t cnt = c.command_counter_d[e];
    float mpos = c.metric_error_pos_2d_d[e], mhead = c.metric_error_heading_d[e];
    mpos0 = mpos; mhead0 = mhead;
    bool resample = false;
    int draw = 0;  // which of the two possible resamplings of this call (reset, timer) -> distinct in-kernel streams
    if (reset) {  // CommandTerm.reset (command_manager.py:120-149): metrics, counter, resample
        mpos = 0.0f; mhead = 0.0f; cnt = 0;
        resample = true;
    }
    for (int pass = 0; pass < (do_compute ? 2 : 1); ++pass) {
        if (pass == 1) {  // CommandTerm.compute (:151-168): _update_metrics (pose_2d_command.py:82-85), timer
            const float dx = pwx - rx, dy = pwy - ry;
            mpos = sqrtf(dx * dx + dy * dy);
            mhead = fabsf(wrap_to_pi(hw - heading));
            tl -= dt;
            resample = tl <= 0.0f;
        }
        if (resample) {  // CommandTerm._resample (:172-187) + _resample_command (pose_2d_command.py:87-115 / :174-203)
            const float* U = c.uniforms_d ? c.uniforms_d + (size_t)draw * N * 4 : nullptr;
            const uint64_t sd = seed + 0x9E3779B97F4A7C15ull * (uint64_t)draw;
            tl = pose2d_u_at(U, e, 0, sd, step) * (c.cfg[1] - c.cfg[0]) + c.cfg[0];
            cnt += 1;
            if (c.kind == 1) {  // a valid patch of the env's terrain cell
                const int64_t P = c.num_patches;
                int64_t id = c.patch_ids_d ? c.patch_ids_d[(size_t)draw * N + e] : (int64_t)(pose2d_u_at(nullptr, e, 1, sd, step) * (float)P);
                id = id < 0 ? 0 : (id >= P ? P - 1 : id);
                int64_t lv = c.terrain_levels_d[e], ty = c.terrain_types_d[e];
                lv = lv < 0 ? 0 : (lv >= c.num_levels ? c.num_levels - 1 : lv);
                ty = ty < 0 ? 0 : (ty >= c.num_types ? c.num_types - 1 : ty);
                const float* t = c.valid_targets_d + ((size_t)(lv * c.num_types + ty) * P + id) * 3;
                pwx = t[0]; pwy = t[1];
                pwz = t[2] + c.default_root_z_d[e];
            } else {  // env origin + uniform offsets, at the robot's default root height
                pwx = c.env_origins_d[e * 3] + (pose2d_u_at(U, e, 1, sd, step) * (c.cfg[3] - c.cfg[2]) + c.cfg[2]);
                pwy = c.env_origins_d[e * 3 + 1] + (pose2d_u_at(U, e, 2, sd, step) * (c.cfg[5] - c.cfg[4]) + c.cfg[4]);
                pwz = c.env_origins_d[e * 3 + 2] + c.default_root_z_d[e];
            }
            if (c.simple_heading) {  // towards the target or away from it, whichever is closer to the current heading (strict <)
                const float td = atan2f(pwy - ry, pwx - rx);
                const float flipped = wrap_to_pi(td + PI);
                const float to_target = fabsf(wrap_to_pi(td - heading)), to_flipped = fabsf(wrap_to_pi(flipped - heading));
                hw = to_target < to_flipped ? td : flipped;
            } else {
                hw = pose2d_u_at(U, e, 3, sd, step) * (c.cfg[7] - c.cfg[6]) + c.cfg[6];
            }
            ++draw;
        }
        resample = false;
    }
    if (do_compute) {  // _update_command (pose_2d_command.py:117-121): the target in the yaw-only base frame
        float yw, yz;
        yaw_quat_wz(qw, qx, qy, qz, yw, yz);
        float bx, by, bz;
        quat_rotate_inverse(yw, 0.0f, 0.0f, yz, pwx - rx, pwy - ry, pwz - rz, bx, by, bz);
        float* cmd = c.command_d + e * 4;
        cmd[0] = bx; cmd[1] = by; cmd[2] = bz;
        cmd[3] = wrap_to_pi(hw - heading);
    }
    c.pos_command_w_d[e * 3] = pwx; c.pos_command_w_d[e * 3 + 1] = pwy; c.pos_command_w_d[e * 3 + 2] = pwz;
    c.heading_command_w_d[e] = hw;
    c.time_left_d[e] = tl;
    c.command_counter_d[e] = cnt;
    c.metric_error_pos_2d_d[e] = mpos;
    c.metric_error_heading_d[e] = mhead;
}

// the argument check both entry points share, as a message (NULL = fine): no launch is made with a pointer this names
static inline const char* pose2d_command_check(const imx_pose2d_command_t* c) {
    if (!c) return "null imx_pose2d_command_t";
    if (c->kind != 0 && c->kind != 1) return "kind is neither 0 (UniformPose2dCommand) nor 1 (TerrainBasedPose2dCommand)";
    if (!(c->cfg[1] > 0.0f)) return "resampling_time_range[1] must be positive";
    if (!c->default_root_z_d) return "default_root_z missing";
    if (c->kind == 0 && !c->env_origins_d) return "env_origins missing";
    if (c->kind == 1) {
        if (!c->valid_targets_d) return "kind 1 (TerrainBasedPose2dCommand) lacks valid_targets";
        if (!c->terrain_levels_d) return "kind 1 (TerrainBasedPose2dCommand) lacks terrain_levels";
        if (!c->terrain_types_d) return "kind 1 (TerrainBasedPose2dCommand) lacks terrain_types";
        if (c->num_levels <= 0 || c->num_types <= 0 || c->num_patches <= 0) return "num_levels, num_types and num_patches must be positive";
    }
    if (!c->command_d) return "command missing";
    if (!c->pos_command_w_d) return "pos_command_w missing";
    if (!c->heading_command_w_d) return "heading_command_w missing";
    if (!c->time_left_d) return "time_left missing";
    if (!c->command_counter_d) return "command_counter missing";
    if (!c->metric_error_pos_2d_d) return "metric error_pos_2d missing";
    if (!c->metric_error_heading_d) return "metric error_heading missing";
    return nullptr;
}
