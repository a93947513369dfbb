// The reset / interval orchestration around the env step as ONE masked kernel (include/imx.h imx_orch_t).
//
// Reference, per step (isaaclab/isaaclab/envs/manager_based_rl_env.py:215-236):
//     reset_env_ids = reset_buf.nonzero()                      # host sync
//     if len(reset_env_ids) > 0: _reset_idx(reset_env_ids)     # :347-392
//         curriculum_manager.compute(env_ids)                  # terrain_levels_vel -> TerrainImporter.update_env_origins
//         scene.reset(env_ids)                                 # ContactSensor.reset, actuator reset, (height scanner: k_term_rew)
//         event_manager.apply("reset", env_ids, step count)    # managers/event_manager.py:233-260 (min_step_count_between_reset)
//         ... manager resets -> extras["log"]                  # command_manager.reset: Metrics/*; curriculum_manager.reset: Curriculum/*
//     command_manager.compute(dt)                              # managers/command_manager.py:151-187
//     event_manager.apply("interval", dt)                      # event_manager.py:205-232: nonzero() + len() per term
// Here: one lane per env walks that list for its env; what the reference decides from id lists it decides from the env's reset flag and
// its timers.  Random draws come from the counter-based generator keyed by (seed, term, column, global step, env) or, in parity runs,
// from caller-supplied tables (the reference's torch.rand stream cannot be reproduced in a kernel).  The two means the log needs
// (metrics over the reset envs, terrain level over all envs) leave as per-workgroup partial sums for the step tail (step.hip).
#include "imx_internal.h"
#include "imx_manip_events.h"
#include "imx_producers.h"

namespace {

constexpr int ORCH_BLOCK = 64;

__device__ __forceinline__ float draw(const float* __restrict__ U, int64_t stride, int64_t e, int col, uint64_t seed, int term, uint32_t step) {
    return U ? U[e * stride + col] : uniform01(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(term * 256 + col + 1), step, (uint64_t)e);
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// POSE: the command term is a UniformPoseCommand (has_command == 2) instead of the velocity command; an instantiation of its own so that
// the velocity cfgs run the register budget they always had, dispatched on the host.  MANIP: the manipulation tasks' launch
// (imx_reset_orchestrate_manip) -- reset_scene_to_default, events on the scene's rigid object and the modify_reward_weight curriculum,
// with imx_orch_manip_t as a second kernel argument; again an instantiation of its own (k_reset_orchestrate_manip below)
// P2D: the command term is a pose-2d command (imx_reset_orchestrate_pose2d; imx_pose2d_command_t as a second kernel argument, has_command
// is 0): the third instantiation of its own (k_reset_orchestrate_pose2d below), no terrain curriculum
// ART2: the MANIP launch on a scene with a second articulation (imx_reset_orchestrate_scene; imx_orch_articulation_t as a third kernel
// argument, imx_event_term_t.asset = 2): the fourth instantiation of its own (k_reset_orchestrate_scene below).  Everything it adds sits
// behind `if (ART2 ...)`, so the three older kernels keep their instruction streams (DESIGN.md has the resource table)
template <bool POSE, bool MANIP, bool P2D = false, bool ART2 = false>
__device__ __forceinline__ void orch_body(const imx_orch_t& o, const imx_orch_manip_t* mp, const imx_pose2d_command_t* pc = nullptr,
                                          const imx_orch_articulation_t* ap = nullptr) {
    const int lane = threadIdx.x;
    const int64_t N = o.num_envs;
    const int64_t e0 = (int64_t)blockIdx.x * ORCH_BLOCK + lane;
    const bool live = e0 < N;
    const int64_t e = live ? e0 : N - 1;  // dead lanes read a valid env, never store
    const int J = (int)o.num_joints, NB = (int)o.num_bodies;
    const uint32_t step = o.step_counter_d ? (uint32_t)o.step_counter_d[0] : 0u;
    const bool reset = live && (o.reset_mask_d ? o.reset_mask_d[e] != 0 : true);

    // ---- CurriculumManager.compute: terrain_levels_vel (curriculums.py:26-55) + update_env_origins (terrain_importer.py:307-326)
    float ox = o.env_origins_d[e * 3], oy = o.env_origins_d[e * 3 + 1], oz = o.env_origins_d[e * 3 + 2];
    float level_f = 0.0f;
    if (!MANIP && !P2D && o.terrain_levels_d) {
        int64_t lv = o.terrain_levels_d[e];
        if (reset) {
            const float dx = o.root_pos_w_d[e * 3] - ox, dy = o.root_pos_w_d[e * 3 + 1] - oy;
            const float dist = sqrtf(dx * dx + dy * dy);  // torch.norm(dim=1)
            const float cx = o.vel_command_b_d[e * 3], cy = o.vel_command_b_d[e * 3 + 1];  // the command BEFORE its reset (:379-380 comes later)
            const bool up = dist > 0.5f * o.terrain_size_x;
            const bool down = (dist < sqrtf(cx * cx + cy * cy) * o.max_episode_length_s * 0.5f) && !up;
            lv = lv + (up ? 1 : 0) - (down ? 1 : 0);
            if (lv >= o.terrain_rows) {  // solved the last level: a random one (randint_like(levels, max_terrain_level))
                lv = o.rand_levels_d ? o.rand_levels_d[e] : (int64_t)(uniform01(o.seed + 991u, step, (uint64_t)e) * (float)o.terrain_rows);
                lv = lv >= o.terrain_rows ? o.terrain_rows - 1 : lv;
            } else if (lv < 0) {
                lv = 0;
            }
            o.terrain_levels_d[e] = lv;
            const float* t = o.terrain_origins_d + ((size_t)lv * o.terrain_cols + (size_t)o.terrain_types_d[e]) * 3;
            ox = t[0]; oy = t[1]; oz = t[2];
            o.env_origins_d[e * 3] = ox; o.env_origins_d[e * 3 + 1] = oy; o.env_origins_d[e * 3 + 2] = oz;
        }
        level_f = live ? (float)lv : 0.0f;
    }

    // ---- scene.reset(env_ids): the env-owned sensors / actuators of a reset env start over.  The WAVE zeroes the rows of each of its
    //      reset envs together (lanes stride over the row: coalesced stores, ~10 instructions per env) -- one lane walking its own env's
    //      272 + 384 floats was 650 store instructions in a divergent branch that 7 of 10 waves enter (25 us for the kernel).
    const uint64_t reset_lanes = __ballot(reset);
    if (MANIP) {
        // CurriculumManager.compute -> modify_reward_weight (envs/mdp/curriculums.py:21-36), run by _reset_idx only: a launch that resets
        // no env stores nothing.  `step` is common_step_counter here.  Every workgroup with a reset env stores the same word: idempotent;
        // the next imx_terminations_rewards launch reads it (stream order)
        for (int i = 0; i < mp->num_weight_terms; ++i) {
            const imx_weight_term_t& W = mp->weight_terms[i];
            if (W.weight == 0.0f && W.step_reward_d) {
                // a term this curriculum puts to sleep: the zero-weight skip never writes its step_reward column again, so the column
                // would keep the values of the last step the term was awake.  The launch that takes the word from non-zero to 0 leaves
                // 1 + its step count in *switch_step_d; from the NEXT step on every workgroup, with a reset env or without, zeroes the
                // entries of its own envs.  In the launch of the switch itself a workgroup reads either the old 0 or step + 1 there,
                // and stores nothing in both cases: that step's column keeps that step's values, whichever workgroup runs first
                const int32_t sw = *W.switch_step_d;
                if (sw != 0 && (int32_t)step >= sw && *W.weight_d == 0.0f && live) W.step_reward_d[e * mp->step_reward_stride] = 0.0f;
            }
            if (reset_lanes != 0ull && (int32_t)step > W.num_steps && lane == 0) {
                if (W.switch_step_d && W.weight == 0.0f && *W.weight_d != 0.0f) *W.switch_step_d = (int32_t)step + 1;
                *W.weight_d = W.weight;
            }
        }
    }
    if (o.cs_timestamp_d || o.lstm_hidden_d) {
        for (uint64_t m = reset_lanes; m != 0ull; m &= m - 1ull) {
            const int64_t er = (int64_t)blockIdx.x * ORCH_BLOCK + (__ffsll((long long)m) - 1);  // wave-uniform
            if (o.cs_timestamp_d) {  // ContactSensor.reset (contact_sensor.py:143-165) + SensorBase.reset (sensor_base.py:182-194)
                const int B = o.cs_num_bodies, H = o.cs_history_length;
                if (lane == 0) { o.cs_timestamp_d[er] = 0.0f; o.cs_timestamp_last_update_d[er] = 0.0f; o.cs_is_outdated_d[er] = 1; }
                for (int i = lane; i < B * 3; i += ORCH_BLOCK) o.cs_net_forces_w_d[(size_t)er * B * 3 + i] = 0.0f;
                if (o.cs_net_forces_w_history_d)
                    for (int i = lane; i < H * B * 3; i += ORCH_BLOCK) o.cs_net_forces_w_history_d[(size_t)er * H * B * 3 + i] = 0.0f;
                if (o.cs_last_air_time_d)
                    for (int b = lane; b < B; b += ORCH_BLOCK) {
                        o.cs_last_air_time_d[(size_t)er * B + b] = 0.0f; o.cs_current_air_time_d[(size_t)er * B + b] = 0.0f;
                        o.cs_last_contact_time_d[(size_t)er * B + b] = 0.0f; o.cs_current_contact_time_d[(size_t)er * B + b] = 0.0f;
                    }
            }
            if (o.lstm_hidden_d) {  // ActuatorNetLSTM.reset (actuators/actuator_net.py:66-70): hidden / cell state of the env's joints
                const int Hd = o.lstm_hidden_dim;
                for (int l = 0; l < o.lstm_layers; ++l)
                    for (int i = lane; i < J * Hd; i += ORCH_BLOCK) {
                        const size_t at = ((size_t)l * N * J + (size_t)er * J) * Hd + i;
                        o.lstm_hidden_d[at] = 0.0f;
                        o.lstm_cell_d[at] = 0.0f;
                    }
            }
        }
    }

    // ---- EventManager.apply("reset", env_ids, global_env_step_count) (event_manager.py:233-260), terms in cfg order
    for (int t = 0; t < o.num_terms; ++t) {
        const imx_event_term_t& T = o.terms[t];
        if (T.mode != 0) continue;
        bool valid = reset;
        if (reset) {
            if (T.min_step_count_between_reset == 0) {
                T.last_triggered_step_d[e] = (int32_t)step;
                T.triggered_once_d[e] = 1;
            } else {
                const int32_t last = T.last_triggered_step_d[e];
                const bool once = T.triggered_once_d[e] != 0;
                valid = ((int32_t)step - last >= T.min_step_count_between_reset) || (last == 0 && !once);
                if (valid) {
                    T.triggered_once_d[e] = 1;
                    T.last_triggered_step_d[e] = (int32_t)step;
                }
            }
        }
        const float* __restrict__ U = T.uniforms_d;
        if (MANIP && T.op == IMX_E_RESET_SCENE_TO_DEFAULT) {  // events.py:1096-1118: rigid objects, then articulations
            if (valid) {
                if (mp->object_default_root_state_d)
                    root_state_default_env(mp->object_default_root_state_d + e * 13, ox, oy, oz, mp->object_root_pose_out_d + e * 7,
                                           mp->object_root_vel_out_d + e * 6);
                root_state_default_env(o.default_root_state_d + e * 13, ox, oy, oz, o.root_pose_out_d + e * 7, o.root_vel_out_d + e * 6);
                if (ART2)
                    root_state_default_env(ap->default_root_state_d + e * 13, ox, oy, oz, ap->root_pose_out_d + e * 7, ap->root_vel_out_d + e * 6);
            }
            for (uint64_t m = __ballot(valid); m != 0ull; m &= m - 1ull) {  // the default joint state, unclamped: lane = joint
                const int64_t er = (int64_t)blockIdx.x * ORCH_BLOCK + (__ffsll((long long)m) - 1);  // wave-uniform
                for (int j = lane; j < J; j += ORCH_BLOCK) {
                    const size_t q = (size_t)er * J + j;
                    o.joint_pos_out_d[q] = o.default_joint_pos_d[q];
                    o.joint_vel_out_d[q] = o.default_joint_vel_d[q];
                }
                if (ART2) {
                    const int J2 = (int)ap->num_joints;
                    for (int j = lane; j < J2; j += ORCH_BLOCK) {
                        const size_t q = (size_t)er * J2 + j;
                        ap->joint_pos_out_d[q] = ap->default_joint_pos_d[q];
                        ap->joint_vel_out_d[q] = ap->default_joint_vel_d[q];
                    }
                }
            }
            continue;
        }
        if (ART2 && T.asset == 2) {  // an event on the second articulation: its defaults, its limits, its out buffers
            if (T.op == IMX_E_RESET_JOINTS_BY_SCALE || T.op == IMX_E_RESET_JOINTS_BY_OFFSET) {  // lane = joint, as for the robot below
                const int J2 = (int)ap->num_joints;
                const bool by_offset = T.op == IMX_E_RESET_JOINTS_BY_OFFSET;
                for (uint64_t m = __ballot(valid); m != 0ull; m &= m - 1ull) {
                    const int64_t er = (int64_t)blockIdx.x * ORCH_BLOCK + (__ffsll((long long)m) - 1);  // wave-uniform
                    for (int j = lane; j < J2; j += ORCH_BLOCK) {
                        const size_t q = (size_t)er * J2 + j;
                        joint_reset_env(by_offset, ap->default_joint_pos_d[q], ap->default_joint_vel_d[q], draw(U, 2 * (int64_t)J2, er, j, o.seed, t, step),
                                        draw(U, 2 * (int64_t)J2, er, J2 + j, o.seed, t, step), T.ranges, ap->soft_joint_pos_limits_d[2 * q],
                                        ap->soft_joint_pos_limits_d[2 * q + 1], ap->soft_joint_vel_limits_d[q], ap->joint_pos_out_d + q,
                                        ap->joint_vel_out_d + q);
                    }
                }
            } else if (valid && T.op == IMX_E_RESET_ROOT_STATE_UNIFORM) {  // as for the rigid object below
                const float* d = ap->default_root_state_d + e * 13;
                float rs[6], u6[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) rs[k] = draw(U, 12, e, k, o.seed, t, step) * (T.ranges[2 * k + 1] - T.ranges[2 * k]) + T.ranges[2 * k];
                root_pose_uniform_env(d, ox, oy, oz, rs, ap->root_pose_out_d + e * 7);
#pragma unroll
                for (int k = 0; k < 6; ++k) u6[k] = draw(U, 12, e, 6 + k, o.seed, t, step);
                root_vel_uniform_env(d, u6, T.ranges + 12, ap->root_vel_out_d + e * 6);
            }
            continue;
        }
        if (T.op == IMX_E_RESET_JOINTS_BY_SCALE || T.op == IMX_E_RESET_JOINTS_BY_OFFSET ||
            T.op == IMX_E_RESET_JOINTS_AROUND_DEFAULT) {  // events.py:987-1049, spot/mdp/events.py:26-60
            // lane = joint of one valid env at a time (the same draws, keyed by (env, column)): 2 J samples + clamps per env spread over
            // the wave instead of a J-trip loop on the env's own lane
            const bool by_offset = T.op == IMX_E_RESET_JOINTS_BY_OFFSET;
            for (uint64_t m = __ballot(valid); m != 0ull; m &= m - 1ull) {
                const int64_t er = (int64_t)blockIdx.x * ORCH_BLOCK + (__ffsll((long long)m) - 1);  // wave-uniform
                for (int j = lane; j < J; j += ORCH_BLOCK) {
                    const size_t q = (size_t)er * J + j;
                    if (T.op == IMX_E_RESET_JOINTS_AROUND_DEFAULT) {  // range clamped to the soft limits first, then sampled
                        const float vl = o.soft_joint_vel_limits_d[q];
                        o.joint_pos_out_d[q] = around_default(o.default_joint_pos_d[q], T.ranges[0], T.ranges[1], o.soft_joint_pos_limits_d[2 * q],
                                                              o.soft_joint_pos_limits_d[2 * q + 1], draw(U, 2 * (int64_t)J, er, j, o.seed, t, step));
                        o.joint_vel_out_d[q] = around_default(o.default_joint_vel_d[q], T.ranges[2], T.ranges[3], -vl, vl,
                                                              draw(U, 2 * (int64_t)J, er, J + j, o.seed, t, step));
                        continue;
                    }
                    const float sp = draw(U, 2 * (int64_t)J, er, j, o.seed, t, step) * (T.ranges[1] - T.ranges[0]) + T.ranges[0];
                    const float sv = draw(U, 2 * (int64_t)J, er, J + j, o.seed, t, step) * (T.ranges[3] - T.ranges[2]) + T.ranges[2];
                    float p = by_offset ? o.default_joint_pos_d[q] + sp : o.default_joint_pos_d[q] * sp;
                    float v = by_offset ? o.default_joint_vel_d[q] + sv : o.default_joint_vel_d[q] * sv;
                    p = fminf(fmaxf(p, o.soft_joint_pos_limits_d[2 * q]), o.soft_joint_pos_limits_d[2 * q + 1]);  // clamp_(lo, hi)
                    v = fminf(fmaxf(v, -o.soft_joint_vel_limits_d[q]), o.soft_joint_vel_limits_d[q]);
                    o.joint_pos_out_d[q] = p;
                    o.joint_vel_out_d[q] = v;
                }
            }
            continue;
        }
        if (!valid) continue;
        switch (T.op) {
            case IMX_E_RESET_ROOT_STATE_UNIFORM: {  // events.py:823-868, on the robot or (MANIP, asset = 1) the scene's rigid object
                const bool obj = MANIP && T.asset == 1;
                const float* d = (obj ? mp->object_default_root_state_d : o.default_root_state_d) + e * 13;
                float rs[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) rs[k] = draw(U, 12, e, k, o.seed, t, step) * (T.ranges[2 * k + 1] - T.ranges[2 * k]) + T.ranges[2 * k];
                root_pose_uniform_env(d, ox, oy, oz, rs, (obj ? mp->object_root_pose_out_d : o.root_pose_out_d) + e * 7);
                float* vel = (obj ? mp->object_root_vel_out_d : o.root_vel_out_d) + e * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    vel[k] = d[7 + k] + (draw(U, 12, e, 6 + k, o.seed, t, step) * (T.ranges[12 + 2 * k + 1] - T.ranges[12 + 2 * k]) + T.ranges[12 + 2 * k]);
            } break;
            case IMX_E_RESET_JOINTS_BY_SCALE:
            case IMX_E_RESET_JOINTS_BY_OFFSET:
            case IMX_E_RESET_JOINTS_AROUND_DEFAULT: break;  // (worked off by the whole wave, below)
            case IMX_E_APPLY_EXTERNAL_FORCE_TORQUE: {  // events.py:764-791: two sample_uniform calls (forces, then torques) of (k, nb, 3)
                const int nb = T.body_ids_d ? T.num_body_ids : NB;
                for (int b = 0; b < nb; ++b) {
                    const int body = T.body_ids_d ? T.body_ids_d[b] : b;
                    for (int c = 0; c < 3; ++c) {
                        const float uf = draw(U, 6 * (int64_t)nb, e, b * 3 + c, o.seed, t, step);
                        const float ut = draw(U, 6 * (int64_t)nb, e, nb * 3 + b * 3 + c, o.seed, t, step);
                        const size_t at = ((size_t)e * NB + body) * 3 + c;
                        o.ext_force_out_d[at] = uf * (T.ranges[1] - T.ranges[0]) + T.ranges[0];
                        o.ext_torque_out_d[at] = ut * (T.ranges[3] - T.ranges[2]) + T.ranges[2];
                    }
                }
            } break;
            case IMX_E_PUSH_BY_SETTING_VELOCITY: {  // a push configured as a reset event
                const float v6[6] = {o.root_lin_vel_w_d[e * 3], o.root_lin_vel_w_d[e * 3 + 1], o.root_lin_vel_w_d[e * 3 + 2],
                                     o.root_ang_vel_w_d[e * 3], o.root_ang_vel_w_d[e * 3 + 1], o.root_ang_vel_w_d[e * 3 + 2]};
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    o.root_vel_out_d[e * 6 + k] = v6[k] + (draw(U, 6, e, k, o.seed, t, step) * (T.ranges[2 * k + 1] - T.ranges[2 * k]) + T.ranges[2 * k]);
            } break;
            default: break;
        }
    }

    // ---- CommandTerm.reset for the reset envs (logs + zeroes the metrics, resamples), then CommandManager.compute(dt)
    float mxy0 = 0.0f, myaw0 = 0.0f;
    if (POSE && live && (!MANIP || o.has_command == 2)) {  // the same place, the same reset flag and the same two log columns as the velocity command
        PoseCmdCfg c;
        c.resample_lo = o.command_cfg[0]; c.resample_hi = o.command_cfg[1];
        c.pos_x_lo = o.command_cfg[2]; c.pos_x_hi = o.command_cfg[3]; c.pos_y_lo = o.command_cfg[4]; c.pos_y_hi = o.command_cfg[5];
        c.pos_z_lo = o.command_cfg[6]; c.pos_z_hi = o.command_cfg[7]; c.roll_lo = o.command_cfg[8]; c.roll_hi = o.command_cfg[9];
        c.pitch_lo = o.command_cfg[10]; c.pitch_hi = o.command_cfg[11]; c.yaw_lo = o.command_cfg[12]; c.yaw_hi = o.command_cfg[13];
        c.make_quat_unique = o.make_quat_unique;
        c.body_idx = o.pose_body_idx; c.num_bodies = NB;
        const PoseCmdState st{o.pose_command_b_d, o.pose_command_w_d, o.command_time_left_d, o.command_counter_d, o.metric_error_vel_xy_d,
                              o.metric_error_vel_yaw_d};
        pose_command_env(N, e, c, o.dt, o.do_step, o.root_pos_w_d, o.root_quat_w_d, o.body_pos_w_d, o.body_quat_w_d, reset,
                         o.command_uniforms_d, o.seed ^ 0xC0FFEEull, step, st, mxy0, myaw0);
    }
    if (P2D && live)  // the same place, the same reset flag and the same two log columns (error_pos_2d, error_heading)
        pose2d_command_env(N, e, *pc, o.dt, o.do_step, o.root_pos_w_d, o.root_quat_w_d, reset, o.seed ^ 0xC0FFEEull, step, mxy0, myaw0);
    if (!POSE && !P2D && o.has_command && live) {
        VelCmdCfg c;
        c.resample_lo = o.command_cfg[0]; c.resample_hi = o.command_cfg[1];
        c.lin_x_lo = o.command_cfg[2]; c.lin_x_hi = o.command_cfg[3]; c.lin_y_lo = o.command_cfg[4]; c.lin_y_hi = o.command_cfg[5];
        c.ang_z_lo = o.command_cfg[6]; c.ang_z_hi = o.command_cfg[7]; c.heading_lo = o.command_cfg[8]; c.heading_hi = o.command_cfg[9];
        c.rel_standing = o.command_cfg[10]; c.rel_heading = o.command_cfg[11]; c.stiffness = o.command_cfg[12];
        c.max_command_step = o.command_cfg[13];
        c.heading_command = o.heading_command;
        const VelCmdState st{o.vel_command_b_d, o.heading_target_d, o.is_heading_env_d, o.is_standing_env_d, o.command_time_left_d,
                             o.command_counter_d, o.metric_error_vel_xy_d, o.metric_error_vel_yaw_d};
        velocity_command_env(N, e, c, o.dt, o.do_step, o.root_quat_w_d, o.root_lin_vel_w_d, o.root_ang_vel_w_d, reset,
                             o.command_uniforms_d, o.seed ^ 0xC0FFEEull, step, st, mxy0, myaw0);
    }

    // ---- EventManager.apply("interval", dt) (event_manager.py:205-232)
    if (o.do_step) {
        for (int t = 0; t < o.num_terms; ++t) {
            const imx_event_term_t& T = o.terms[t];
            if (T.mode != 1) continue;
            bool fire;
            if (T.is_global_time) {  // one timer: slot [step & 1] -> slot [(step + 1) & 1]; a single draw; the term runs on EVERY env
                float tl = T.time_left_d[step & 1u] - o.dt;
                fire = tl < 1.0e-6f;
                if (fire) {
                    const float u = T.interval_uniforms_d ? T.interval_uniforms_d[0]
                                                          : uniform01(o.seed + 0x1717ull * (uint64_t)(t + 1), step, 0xFFFFFFFFull);
                    tl = u * (T.interval_hi - T.interval_lo) + T.interval_lo;
                }
                if (blockIdx.x == 0 && lane == 0) T.time_left_d[(step + 1u) & 1u] = tl;
            } else {
                float tl = T.time_left_d[e] - o.dt;
                fire = tl < 1.0e-6f;
                if (fire) {
                    const float u = T.interval_uniforms_d ? T.interval_uniforms_d[e]
                                                          : uniform01(o.seed + 0x1717ull * (uint64_t)(t + 1), step, (uint64_t)e);
                    tl = u * (T.interval_hi - T.interval_lo) + T.interval_lo;
                }
                if (live) T.time_left_d[e] = tl;
            }
            if (!fire || !live) continue;
            const float* __restrict__ U = T.uniforms_d;
            if (T.op == IMX_E_PUSH_BY_SETTING_VELOCITY) {  // events.py:795-820: root_vel_w + sample -> write_root_velocity_to_sim
                const float v6[6] = {o.root_lin_vel_w_d[e * 3], o.root_lin_vel_w_d[e * 3 + 1], o.root_lin_vel_w_d[e * 3 + 2],
                                     o.root_ang_vel_w_d[e * 3], o.root_ang_vel_w_d[e * 3 + 1], o.root_ang_vel_w_d[e * 3 + 2]};
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    o.root_vel_out_d[e * 6 + k] = v6[k] + (draw(U, 6, e, k, o.seed, t, step) * (T.ranges[2 * k + 1] - T.ranges[2 * k]) + T.ranges[2 * k]);
            } else if (T.op == IMX_E_APPLY_EXTERNAL_FORCE_TORQUE) {
                const int nb = T.body_ids_d ? T.num_body_ids : NB;
                for (int b = 0; b < nb; ++b) {
                    const int body = T.body_ids_d ? T.body_ids_d[b] : b;
                    for (int c = 0; c < 3; ++c) {
                        const size_t at = ((size_t)e * NB + body) * 3 + c;
                        o.ext_force_out_d[at] = draw(U, 6 * (int64_t)nb, e, b * 3 + c, o.seed, t, step) * (T.ranges[1] - T.ranges[0]) + T.ranges[0];
                        o.ext_torque_out_d[at] = draw(U, 6 * (int64_t)nb, e, nb * 3 + b * 3 + c, o.seed, t, step) * (T.ranges[3] - T.ranges[2]) + T.ranges[2];
                    }
                }
            }
        }
    }

    // ---- partial sums for the log (fixed-shape shuffle tree: deterministic)
    if (o.ev_part_d) {
        const float a = wsum(reset ? mxy0 : 0.0f), b = wsum(reset ? myaw0 : 0.0f), c = wsum(level_f), d = wsum(reset ? 1.0f : 0.0f);
        if (lane == 0) {
            float4* p = reinterpret_cast<float4*>(o.ev_part_d) + blockIdx.x;
            *p = make_float4(a, b, c, d);
        }
    }
}

template <bool POSE>
__global__ void __launch_bounds__(ORCH_BLOCK) k_reset_orchestrate(imx_orch_t o) {
    orch_body<POSE, false>(o, nullptr);
}

__global__ void __launch_bounds__(ORCH_BLOCK) k_reset_orchestrate_manip(imx_orch_t o, imx_orch_manip_t m) {
    orch_body<true, true>(o, &m);
}

__global__ void __launch_bounds__(ORCH_BLOCK) k_reset_orchestrate_pose2d(imx_orch_t o, imx_pose2d_command_t c) {
    orch_body<false, false, true>(o, nullptr, &c);
}

__global__ void __launch_bounds__(ORCH_BLOCK) k_reset_orchestrate_scene(imx_orch_t o, imx_orch_manip_t m, imx_orch_articulation_t a) {
    orch_body<true, true, false, true>(o, &m, nullptr, &a);
}

}  // namespace

extern "C" size_t imx_orch_part_floats(int64_t num_envs) { return num_envs > 0 ? (size_t)((num_envs + ORCH_BLOCK - 1) / ORCH_BLOCK) * 4 : 0; }

// the argument checks of the entry points (m = NULL and pc = NULL: imx_reset_orchestrate; pc: imx_reset_orchestrate_pose2d; m and a:
// imx_reset_orchestrate_scene) and the launch
static int orch_launch(const imx_orch_t* o, const imx_orch_manip_t* m, imx_stream_t stream, const imx_pose2d_command_t* pc = nullptr,
                       const imx_orch_articulation_t* a = nullptr) {
    IMX_REQUIRE(o, "imx_reset_orchestrate: null descriptor");
    IMX_REQUIRE(o->num_envs > 0 && o->num_envs < (1ll << 31), "imx_reset_orchestrate: num_envs out of range");
    IMX_REQUIRE(o->num_terms >= 0 && o->num_terms <= IMX_ORCH_MAX_TERMS, "imx_reset_orchestrate: %d event terms (at most %d)", o->num_terms,
                IMX_ORCH_MAX_TERMS);
    IMX_REQUIRE(o->env_origins_d, "imx_reset_orchestrate: env_origins missing");
    if (pc)
        IMX_REQUIRE(o->has_command == 0, "imx_reset_orchestrate_pose2d: has_command is %d: the pose-2d command travels in "
                    "imx_pose2d_command_t, has_command must be 0 here", o->has_command);
    bool need_root = false, need_vel = false;
    for (int t = 0; t < o->num_terms; ++t) {
        const imx_event_term_t& T = o->terms[t];
        IMX_REQUIRE(T.mode == 0 || T.mode == 1, "imx_reset_orchestrate: term %d has mode %d (0 reset, 1 interval)", t, T.mode);
        if (T.mode == 0) IMX_REQUIRE(T.last_triggered_step_d && T.triggered_once_d, "imx_reset_orchestrate: reset term %d lacks its trigger state", t);
        if (T.mode == 1) {
            IMX_REQUIRE(T.time_left_d, "imx_reset_orchestrate: interval term %d lacks its timer", t);
            IMX_REQUIRE(T.op == IMX_E_PUSH_BY_SETTING_VELOCITY || T.op == IMX_E_APPLY_EXTERNAL_FORCE_TORQUE,
                        "imx_reset_orchestrate: interval term %d: op %d is not an interval event here", t, T.op);
        }
        IMX_REQUIRE(T.asset == 0 || (T.asset == 1 && T.op == IMX_E_RESET_ROOT_STATE_UNIFORM) || (T.asset == 2 && a),
                    "imx_reset_orchestrate: term %d: asset %d with op %d (0 the robot; 1 the rigid object, reset_root_state_uniform only; 2 the "
                    "second articulation, which travels in imx_orch_articulation_t: that is imx_reset_orchestrate_scene)", t, T.asset, T.op);
        if (T.asset == 2) {
            const bool joints = T.op == IMX_E_RESET_JOINTS_BY_SCALE || T.op == IMX_E_RESET_JOINTS_BY_OFFSET;
            IMX_REQUIRE(T.mode == 0 && (joints || T.op == IMX_E_RESET_ROOT_STATE_UNIFORM),
                        "imx_reset_orchestrate_scene: term %d: op %d in mode %d on the second articulation has no kernel (the reset events "
                        "reset_root_state_uniform, reset_joints_by_offset and reset_joints_by_scale have)", t, T.op, T.mode);
            IMX_REQUIRE(a->default_root_state_d || joints, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks default_root_state", t);
            IMX_REQUIRE(a->root_pose_out_d || joints, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks root_pose_out", t);
            IMX_REQUIRE(a->root_vel_out_d || joints, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks root_vel_out", t);
            if (joints) {
                IMX_REQUIRE(a->default_joint_pos_d, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks default_joint_pos", t);
                IMX_REQUIRE(a->default_joint_vel_d, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks default_joint_vel", t);
                IMX_REQUIRE(a->soft_joint_pos_limits_d, "imx_reset_orchestrate_scene: term %d is a joint event on the second articulation, which lacks soft_joint_pos_limits", t);
                IMX_REQUIRE(a->soft_joint_vel_limits_d, "imx_reset_orchestrate_scene: term %d is a joint event on the second articulation, which lacks soft_joint_vel_limits", t);
                IMX_REQUIRE(a->joint_pos_out_d, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks joint_pos_out", t);
                IMX_REQUIRE(a->joint_vel_out_d, "imx_reset_orchestrate_scene: term %d acts on the second articulation, which lacks joint_vel_out", t);
            }
            continue;
        }
        if (T.asset == 1) {
            IMX_REQUIRE(m, "imx_reset_orchestrate: term %d acts on the rigid object: that is imx_reset_orchestrate_manip", t);
            IMX_REQUIRE(m->object_default_root_state_d && m->object_root_pose_out_d && m->object_root_vel_out_d,
                        "imx_reset_orchestrate_manip: term %d acts on the rigid object, which lacks its default root state or an out buffer", t);
            continue;
        }
        switch (T.op) {
            case IMX_E_RESET_SCENE_TO_DEFAULT:
                IMX_REQUIRE(m, "imx_reset_orchestrate: term %d is reset_scene_to_default: that is imx_reset_orchestrate_manip", t);
                IMX_REQUIRE(T.mode == 0, "imx_reset_orchestrate_manip: reset_scene_to_default is a reset event (term %d has mode %d)", t, T.mode);
                IMX_REQUIRE(o->default_root_state_d && o->root_pose_out_d && o->root_vel_out_d && o->num_joints > 0 && o->default_joint_pos_d &&
                            o->default_joint_vel_d && o->joint_pos_out_d && o->joint_vel_out_d,
                            "imx_reset_orchestrate_manip: reset_scene_to_default needs the robot's default root and joint state and their outputs");
                IMX_REQUIRE(!m->object_default_root_state_d || (m->object_root_pose_out_d && m->object_root_vel_out_d),
                            "imx_reset_orchestrate_manip: the rigid object lacks an out buffer");
                if (a) {  // reset_scene_to_default walks every articulation of the scene
                    IMX_REQUIRE(a->default_root_state_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks default_root_state", t);
                    IMX_REQUIRE(a->default_joint_pos_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks default_joint_pos", t);
                    IMX_REQUIRE(a->default_joint_vel_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks default_joint_vel", t);
                    IMX_REQUIRE(a->root_pose_out_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks root_pose_out", t);
                    IMX_REQUIRE(a->root_vel_out_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks root_vel_out", t);
                    IMX_REQUIRE(a->joint_pos_out_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks joint_pos_out", t);
                    IMX_REQUIRE(a->joint_vel_out_d, "imx_reset_orchestrate_scene: term %d (reset_scene_to_default): the second articulation lacks joint_vel_out", t);
                }
                break;
            case IMX_E_RESET_ROOT_STATE_UNIFORM:
                IMX_REQUIRE(o->default_root_state_d && o->root_pose_out_d && o->root_vel_out_d, "imx_reset_orchestrate: reset_root_state_uniform needs "
                            "default_root_state, root_pose_out and root_vel_out");
                break;
            case IMX_E_RESET_JOINTS_BY_SCALE: case IMX_E_RESET_JOINTS_BY_OFFSET: case IMX_E_RESET_JOINTS_AROUND_DEFAULT:
                IMX_REQUIRE(o->num_joints > 0 && o->default_joint_pos_d && o->default_joint_vel_d && o->soft_joint_pos_limits_d &&
                            o->soft_joint_vel_limits_d && o->joint_pos_out_d && o->joint_vel_out_d,
                            "imx_reset_orchestrate: a joint reset needs the joint defaults, limits and outputs");
                break;
            case IMX_E_PUSH_BY_SETTING_VELOCITY:
                need_vel = true;
                IMX_REQUIRE(o->root_vel_out_d, "imx_reset_orchestrate: push_by_setting_velocity needs root_vel_out");
                break;
            case IMX_E_APPLY_EXTERNAL_FORCE_TORQUE:
                IMX_REQUIRE(o->num_bodies > 0 && o->ext_force_out_d && o->ext_torque_out_d, "imx_reset_orchestrate: apply_external_force_torque needs "
                            "the body count and the force / torque outputs");
                IMX_REQUIRE(!T.body_ids_d || (T.num_body_ids > 0 && T.num_body_ids <= o->num_bodies), "imx_reset_orchestrate: bad body id count");
                break;
            default: IMX_FAIL("imx_reset_orchestrate: term %d has unknown op %d", t, T.op);
        }
    }
    if (o->terrain_levels_d) {
        need_root = true;
        IMX_REQUIRE(o->terrain_origins_d && o->terrain_types_d && o->terrain_rows > 0 && o->terrain_cols > 0 && o->vel_command_b_d,
                    "imx_reset_orchestrate: the terrain curriculum needs terrain origins, types, the grid size and the velocity command");
    }
    IMX_REQUIRE(o->has_command >= 0 && o->has_command <= 2, "imx_reset_orchestrate: has_command is %d (0 none, 1 velocity, 2 pose)", o->has_command);
    if (o->has_command == 2) {
        need_root = true;
        IMX_REQUIRE(!o->terrain_levels_d, "imx_reset_orchestrate: the terrain curriculum (terrain_levels_vel) reads a velocity command; the "
                    "command term is a pose command");
        IMX_REQUIRE(o->pose_command_b_d, "imx_reset_orchestrate: the pose command lacks pose_command_b");
        IMX_REQUIRE(o->pose_command_w_d, "imx_reset_orchestrate: the pose command lacks pose_command_w");
        IMX_REQUIRE(o->command_time_left_d && o->command_counter_d, "imx_reset_orchestrate: the pose command lacks its timer or counter");
        IMX_REQUIRE(o->metric_error_vel_xy_d && o->metric_error_vel_yaw_d, "imx_reset_orchestrate: the pose command lacks a metric tensor");
        IMX_REQUIRE(o->root_quat_w_d, "imx_reset_orchestrate: root_quat_w missing");
        IMX_REQUIRE(o->body_pos_w_d && o->body_quat_w_d, "imx_reset_orchestrate: the pose command needs body_pos_w and body_quat_w");
        IMX_REQUIRE(o->num_bodies > 0 && o->pose_body_idx >= 0 && o->pose_body_idx < o->num_bodies,
                    "imx_reset_orchestrate: pose_body_idx %d outside [0, %lld)", o->pose_body_idx, (long long)o->num_bodies);
        IMX_REQUIRE(o->command_cfg[1] > 0.0f, "imx_reset_orchestrate: resampling_time_range[1] must be positive");
    }
    if (o->has_command == 1) {
        need_vel = true;
        IMX_REQUIRE(o->root_quat_w_d && o->vel_command_b_d && o->heading_target_d && o->is_heading_env_d && o->is_standing_env_d &&
                    o->command_time_left_d && o->command_counter_d && o->metric_error_vel_xy_d && o->metric_error_vel_yaw_d,
                    "imx_reset_orchestrate: the command term lacks a state tensor");
        IMX_REQUIRE(o->command_cfg[13] > 0.0f, "imx_reset_orchestrate: max_command_step must be positive");
    }
    IMX_REQUIRE(!need_root || o->root_pos_w_d, "imx_reset_orchestrate: root_pos_w missing");
    IMX_REQUIRE(!need_vel || (o->root_lin_vel_w_d && o->root_ang_vel_w_d), "imx_reset_orchestrate: root velocities missing");
    if (o->cs_timestamp_d)
        IMX_REQUIRE(o->cs_timestamp_last_update_d && o->cs_is_outdated_d && o->cs_net_forces_w_d && o->cs_num_bodies > 0 &&
                    (o->cs_last_air_time_d == nullptr) == (o->cs_current_air_time_d == nullptr) &&
                    (o->cs_last_air_time_d == nullptr) == (o->cs_last_contact_time_d == nullptr) &&
                    (o->cs_last_air_time_d == nullptr) == (o->cs_current_contact_time_d == nullptr),
                    "imx_reset_orchestrate: incomplete contact-sensor state");
    if (o->lstm_hidden_d) IMX_REQUIRE(o->lstm_cell_d && o->lstm_layers > 0 && o->lstm_hidden_dim > 0 && o->num_joints > 0,
                                      "imx_reset_orchestrate: incomplete actuator-net state");
    const unsigned grid = (unsigned)((o->num_envs + ORCH_BLOCK - 1) / ORCH_BLOCK);
    if (pc) {
        IMX_REQUIRE(!o->terrain_levels_d, "imx_reset_orchestrate_pose2d: the terrain curriculum (terrain_levels_vel) reads a velocity command "
                    "and moves env_origins; it is not part of this launch");
        if (const char* why = pose2d_command_check(pc)) IMX_FAIL("imx_reset_orchestrate_pose2d: %s", why);
        IMX_REQUIRE(o->root_pos_w_d, "imx_reset_orchestrate_pose2d: root_pos_w missing");
        IMX_REQUIRE(o->root_quat_w_d, "imx_reset_orchestrate_pose2d: root_quat_w missing");
        hipLaunchKernelGGL(k_reset_orchestrate_pose2d, dim3(grid), dim3(ORCH_BLOCK), 0, (hipStream_t)stream, *o, *pc);
    } else if (m) {
        IMX_REQUIRE(o->has_command != 1, "imx_reset_orchestrate_manip: the command term is a velocity command (has_command 0 or 2 here)");
        IMX_REQUIRE(!o->terrain_levels_d, "imx_reset_orchestrate_manip: the terrain curriculum is not part of this launch");
        IMX_REQUIRE(m->num_weight_terms >= 0 && m->num_weight_terms <= IMX_ORCH_MAX_WEIGHT_TERMS,
                    "imx_reset_orchestrate_manip: %d weight terms (at most %d)", m->num_weight_terms, IMX_ORCH_MAX_WEIGHT_TERMS);
        IMX_REQUIRE(m->num_weight_terms == 0 || o->step_counter_d, "imx_reset_orchestrate_manip: the weight curriculum reads step_counter");
        for (int i = 0; i < m->num_weight_terms; ++i) {
            IMX_REQUIRE(m->weight_terms[i].weight_d, "imx_reset_orchestrate_manip: weight term %d has no weight address", i);
            IMX_REQUIRE(!m->weight_terms[i].step_reward_d || (m->step_reward_stride > 0 && m->weight_terms[i].switch_step_d),
                        "imx_reset_orchestrate_manip: weight term %d has a step_reward column but no switch_step word or no step_reward_stride (%d)",
                        i, m->step_reward_stride);
        }
        if (a) {
            IMX_REQUIRE(a->num_joints > 0 && a->num_joints < (1ll << 20), "imx_reset_orchestrate_scene: the second articulation has %lld joints",
                        (long long)a->num_joints);
            hipLaunchKernelGGL(k_reset_orchestrate_scene, dim3(grid), dim3(ORCH_BLOCK), 0, (hipStream_t)stream, *o, *m, *a);
        } else
            hipLaunchKernelGGL(k_reset_orchestrate_manip, dim3(grid), dim3(ORCH_BLOCK), 0, (hipStream_t)stream, *o, *m);
    } else if (o->has_command == 2)
        hipLaunchKernelGGL(k_reset_orchestrate<true>, dim3(grid), dim3(ORCH_BLOCK), 0, (hipStream_t)stream, *o);
    else
        hipLaunchKernelGGL(k_reset_orchestrate<false>, dim3(grid), dim3(ORCH_BLOCK), 0, (hipStream_t)stream, *o);
    IMX_HIP(hipGetLastError());
    return 0;
}

extern "C" int imx_reset_orchestrate(const imx_orch_t* o, imx_stream_t stream) { return orch_launch(o, nullptr, stream); }

extern "C" int imx_reset_orchestrate_manip(const imx_orch_t* o, const imx_orch_manip_t* m, imx_stream_t stream) {
    IMX_REQUIRE(m, "imx_reset_orchestrate_manip: null imx_orch_manip_t");
    return orch_launch(o, m, stream);
}

extern "C" int imx_reset_orchestrate_pose2d(const imx_orch_t* o, const imx_pose2d_command_t* cmd, imx_stream_t stream) {
    IMX_REQUIRE(cmd, "imx_reset_orchestrate_pose2d: null imx_pose2d_command_t");
    return orch_launch(o, nullptr, stream, cmd);
}

extern "C" int imx_reset_orchestrate_scene(const imx_orch_t* o, const imx_orch_manip_t* m, const imx_orch_articulation_t* a, imx_stream_t stream) {
    IMX_REQUIRE(m, "imx_reset_orchestrate_scene: null imx_orch_manip_t");
    IMX_REQUIRE(a, "imx_reset_orchestrate_scene: null imx_orch_articulation_t");
    return orch_launch(o, m, stream, nullptr, a);
}
