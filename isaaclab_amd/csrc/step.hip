// Post-physics env-step kernels (gfx950): action affine, terminations + rewards + reset bookkeeping, observations.
//
// Layout: one environment per lane ("env-per-lane") for the reduction-shaped work (terminations, rewards: every term
// is a small per-env reduction over joints/bodies), one OUTPUT ELEMENT per lane for the observation matrix so that
// the (N,D) row-major store is perfectly coalesced.  Term tables are wave-uniform, so the interpreter's switch is a
// scalar branch; per-term constants come through the scalar cache.  All arithmetic is fp32 in the reference's
// association order (compile with -ffp-contract=off).
#include "imx_internal.h"
#include "imx_raycast.h"
#include "imx_obs_device.h"
// Scalar-register budget of the lean observation kernel.  On gfx950 a SIMD has 800 SGPRs, allocated in blocks of 16: the 106 the compiler
// takes by default (100 + VCC / FLAT_SCRATCH / XNACK) round to 112 = SEVEN waves per SIMD although the 57 VGPRs allow eight.  Capped,
// the compiler parks ~30 rarely used scalars in VGPR lanes; measured at 65 536 envs: 102 -> 142 us, 96 -> 132, 88 -> 132, 80 -> 126,
// 72 -> 129, 64 -> 135 (at 4096 envs all within 0.2 us).
#ifndef IMX_LEAN_SGPRS
#define IMX_LEAN_SGPRS 80
#endif

// ------------------------------------------------------------------------------------------------- helpers
IMX_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
IMX_DEV int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sequential-order sum of f(ids[i]), i = 0..n-1 (torch.sum's left-to-right order for these short rows).  Full trips of 8 issue
// their loads before the first add; the remainder runs one by one -- no padded duplicates: for the force-history terms one
// element costs ~40 instructions and the slowest term is the kernel's critical path.
template <class F>
IMX_DEV float sum_ids(const int32_t* __restrict__ ids, int n, F f) {
    float acc = 0.0f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = f(ids[i + u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; i + 4 <= n; i += 4) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = f(ids[i + u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += x[u];
    }
    for (; i < n; ++i) acc += f(ids[i]);
    return acc;
}
template <class F>
IMX_DEV float sum_range(int n, F f) {
    float acc = 0.0f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = f(i + u);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; i + 4 <= n; i += 4) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = f(i + u);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += x[u];
    }
    for (; i < n; ++i) acc += f(i);
    return acc;
}
template <class F>
IMX_DEV bool any_ids(const int32_t* __restrict__ ids, int n, F f) {
    bool acc = false;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        bool x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = f(ids[i + u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc || x[u];
    }
    for (; i < n; ++i) acc = f(ids[i]) || acc;
    return acc;
}

// max over history of the force norm on body b (rewards.py:266, terminations.py:157): max_h sqrt(s_h) with s_h = (x^2 + y^2) + z^2.
// sqrtf is correctly rounded and monotone, so max_h sqrt(s_h) == sqrt(max_h s_h) bit for bit: ONE square root per body.

IMX_DEV float max_hist_force(const float* __restrict__ F, int64_t e, int H, int B, int b) {
    const float* f = F + ((size_t)e * H * B + b) * 3;
    float m = 0.0f;  // squared norms are >= 0
    int h = 0;
    for (; h + 3 <= H; h += 3) {  // the usual history_length = 3 in one trip
        float v[9];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const float* g = f + (size_t)(h + u) * B * 3;
            v[3 * u] = g[0]; v[3 * u + 1] = g[1]; v[3 * u + 2] = g[2];
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) m = fmaxf(m, (v[3 * u] * v[3 * u] + v[3 * u + 1] * v[3 * u + 1]) + v[3 * u + 2] * v[3 * u + 2]);
    }
    for (; h < H; ++h) {
        const float* g = f + (size_t)h * B * 3;
        m = fmaxf(m, (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    }
    return sqrtf(m);
}

// the gate of Spot's gait / air-time / joint-position terms (isaaclab_tasks .../velocity/config/spot/mdp/rewards.py:52-53):
// torch.norm(cmd, dim=1) > 0 over all three command components, or torch.linalg.norm(v_b[:, :2]) > velocity_threshold
IMX_DEV bool spot_active(float cx, float cy, float cz, float vx, float vy, float vth) {
    return sqrtf((cx * cx + cy * cy) + cz * cz) > 0.0f || sqrtf(vx * vx + vy * vy) > vth;
}

// ---- classic/humanoid/mdp (isaaclab_tasks .../classic/humanoid/mdp: Isaac-Ant-v0, Isaac-Humanoid-v0)
// progress_reward's potential (rewards.py:43-78): -torch.norm(target - root_pos_w, dim=-1) / step_dt in the reference's fp32 sequence --
// separately rounded squares, (x + y) + z, a correctly rounded sqrtf and a true IEEE division by fp32(step_dt) (the potentials are
// ~6e4: one ulp is 4e-3, so only the exact sequence reproduces the reward).  __call__ zeroes z first (z_on = false); reset() keeps it
// (z_on = true).  The ONE formula of the step kernel and of k_term_state_reset.
IMX_DEV float progress_potential(float tx, float ty, float tz, float px, float py, float pz, float dt, bool z_on) {
    const float dx = tx - px, dy = ty - py, dz = z_on ? tz - pz : 0.0f;
    return -sqrtf((dx * dx + dy * dy) + dz * dz) / dt;
}

// The reward functions of classic/humanoid/mdp/rewards.py for env ec -- the raw value f.  Evaluated in phase 2 of
// k_term_rew<true, false>, next to is_alive: progress_reward needs the reset flag there anyway, and phase 2 holds far fewer live values
// than the phase-1 switch.
IMX_DEV float classic_reward(const PlanView& P, const imx_state_t& S, const imx_buffers_t& Bf, const int32_t* __restrict__ r, int op,
                             int64_t ec, int64_t N) {
    const int J = P.J;
    const float p0 = f_of(r[IMX_R_P0]);
    const float4 q4 = reinterpret_cast<const float4*>(S.root_quat_w)[ec];
    switch (op) {
        case IMX_W_UPRIGHT_POSTURE_BONUS: {  // :21-27, up_proj = -projected_gravity_b.z (the phase-0 function, same inputs: same bits)
            float pgx, pgy, pgz;
            quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, P.gx, P.gy, P.gz, pgx, pgy, pgz);
            return (-pgz > p0) ? 1.0f : 0.0f;
        }
        case IMX_W_MOVE_TO_TARGET_BONUS: {  // :30-40
            const float hp = heading_proj(q4.x, q4.y, q4.z, q4.w, f_of(r[IMX_R_P1]), f_of(r[IMX_R_P2]), S.root_pos_w[ec * 3], S.root_pos_w[ec * 3 + 1]);
            return hp > p0 ? 1.0f : hp / p0;
        }
        case IMX_W_PROGRESS_REWARD: {  // :64-78: potentials - prev_potentials (the caller stores the new potential)
            const float cur = progress_potential(p0, f_of(r[IMX_R_P1]), 0.0f, S.root_pos_w[ec * 3], S.root_pos_w[ec * 3 + 1], 0.0f, P.step_dt, false);
            return cur - Bf.term_state[(size_t)r[IMX_R_AUX0] * N + ec];
        }
        case IMX_W_JOINT_POS_LIMITS_PENALTY_RATIO: {  // :81-111, every joint; gear table at ids2; p1 = f32(1 - threshold)
            const int32_t* ids = P.w + r[IMX_R_IDS_OFF];
            const float* __restrict__ gr = reinterpret_cast<const float*>(P.w + r[IMX_R_IDS2_OFF]);
            const float p1 = f_of(r[IMX_R_P1]);
            float acc = 0.0f;  // (sum_ids' left-to-right order, one joint per trip: its 8 loads in flight cost registers the kernel has not)
            for (int i = 0, n = r[IMX_R_NIDS]; i < n; ++i) {
                const int j = ids[i];
                const float2 lim = reinterpret_cast<const float2*>(S.soft_joint_pos_limits)[ec * J + j];
                const float offset = (lim.x + lim.y) * 0.5f;  // scale_transform (utils/math.py:22-40)
                const float s = fabsf(2.0f * (S.joint_pos[ec * J + j] - offset) / (lim.y - lim.x));
                const float v = (s - p0) / p1 * gr[j];
                acc += (s > p0 ? 1.0f : 0.0f) * v;
            }
            return acc;
        }
        case IMX_W_POWER_CONSUMPTION: {  // :114-140: |raw action x joint_vel x gear| (env.action_manager.action, A == J)
            const int32_t* ids = P.w + r[IMX_R_IDS_OFF];
            const float* __restrict__ gr = reinterpret_cast<const float*>(P.w + r[IMX_R_IDS2_OFF]);
            const int A = P.A;
            float acc = 0.0f;
            for (int i = 0, n = r[IMX_R_NIDS]; i < n; ++i) {
                const int j = ids[i];
                acc += fabsf(Bf.action[ec * A + j] * S.joint_vel[ec * J + j] * gr[j]);
            }
            return acc;
        }
        default: return 0.0f;
    }
}

// ---- manipulation/reach/mdp (isaaclab_tasks .../manipulation/reach/mdp: Isaac-Reach-Franka-v0, Isaac-Reach-UR10-v0)
// quat_error_magnitude(q1, q2) (utils/math.py:678-690) = ||axis_angle_from_quat(quat_mul(q1, quat_conjugate(q2)))||; quat_mul_ref and
// axis_angle_magnitude live in imx_internal.h (the pose command's metrics use them too)
IMX_DEV float quat_error_magnitude(float4 q1, float4 q2) {
    return axis_angle_magnitude(quat_mul_ref(q1, make_float4(q2.x, -q2.y, -q2.z, -q2.w)));
}
// des_pos_w = root_pos_w + quat_apply(root_quat_w, cmd[:3]) (combine_frame_transforms: t01 + quat_apply(q01, t12)): the commanded
// position in the world frame, for the reach rewards and the lift terms alike; rq = the root quaternion, c = cmd[:3]
IMX_DEV void command_des_pos_w(const float* __restrict__ root_pos, float4 rq, float cx, float cy, float cz, float& x, float& y, float& z) {
    float ox, oy, oz;
    quat_apply(rq.x, rq.y, rq.z, rq.w, cx, cy, cz, ox, oy, oz);
    x = root_pos[0] + ox;
    y = root_pos[1] + oy;
    z = root_pos[2] + oz;
}
IMX_DEV void command_des_pos_w(const PlanView& P, const imx_state_t& S, int64_t ec, float& x, float& y, float& z) {
    const float* __restrict__ cmd = S.command + ec * P.CMD;
    command_des_pos_w(S.root_pos_w + ec * 3, reinterpret_cast<const float4*>(S.root_quat_w)[ec], cmd[0], cmd[1], cmd[2], x, y, z);
}
// The reward functions of manipulation/reach/mdp/rewards.py for env ec -- the raw value f.  Evaluated in phase 2 of k_term_rew<false,
// true> (the classic terms' place: phase 2 holds far fewer live values than the phase-1 switch).  ids[0] = asset_cfg.body_ids[0].
IMX_DEV float reach_reward(const PlanView& P, const imx_state_t& S, const int32_t* __restrict__ r, int op, int64_t ec) {
    const int b = P.w[r[IMX_R_IDS_OFF]];
    if (op == IMX_W_ORIENTATION_COMMAND_ERROR) {  // :56-72: des_quat_w = quat_mul(root_quat_w, cmd[3:7])
        const float4 rq = reinterpret_cast<const float4*>(S.root_quat_w)[ec];
        const float* __restrict__ cmd = S.command + ec * P.CMD;
        const float4 des = quat_mul_ref(rq, make_float4(cmd[3], cmd[4], cmd[5], cmd[6]));
        const float4 cur = reinterpret_cast<const float4*>(S.body_quat_w)[ec * P.NB + b];
        return quat_error_magnitude(cur, des);
    }
    // :19-53
    float px, py, pz;
    command_des_pos_w(P, S, ec, px, py, pz);
    const float dx = S.body_pos_w[(ec * P.NB + b) * 3] - px;
    const float dy = S.body_pos_w[(ec * P.NB + b) * 3 + 1] - py;
    const float dz = S.body_pos_w[(ec * P.NB + b) * 3 + 2] - pz;
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    return op == IMX_W_POSITION_COMMAND_ERROR_TANH ? 1.0f - tanhf(d / f_of(r[IMX_R_P0])) : d;
}

// ---- manipulation/lift/mdp (isaaclab_tasks .../manipulation/lift/mdp: Isaac-Lift-Cube-Franka-v0); the object = S.object_root_pos_w
// ||des_pos_w - object_pos_w||: object_goal_distance (rewards.py:60-65) and object_reached_goal (terminations.py:46-50)
IMX_DEV float object_goal_dist(const float* __restrict__ obj, float px, float py, float pz) {
    const float dx = px - obj[0], dy = py - obj[1], dz = pz - obj[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}
// The reward functions of manipulation/lift/mdp/rewards.py for env ec -- the raw value f; next to the reach rewards in phase 2 of
// k_term_rew_lift.
IMX_DEV float lift_reward(const PlanView& P, const imx_state_t& S, const int32_t* __restrict__ r, int op, int64_t ec) {
    const float p0 = f_of(r[IMX_R_P0]);
    const float oz = S.object_root_pos_w[ec * 3 + 2];
    if (op == IMX_W_OBJECT_IS_LIFTED) return oz > p0 ? 1.0f : 0.0f;  // :20-25
    if (op == IMX_W_OBJECT_GOAL_DISTANCE)                            // :48-67: (z > minimal_height) * (1 - tanh(distance / std))
    {
        float px, py, pz;
        command_des_pos_w(P, S, ec, px, py, pz);
        return (oz > f_of(r[IMX_R_P1]) ? 1.0f : 0.0f) * (1.0f - tanhf(object_goal_dist(S.object_root_pos_w + ec * 3, px, py, pz) / p0));
    }
    // object_ee_distance :28-45: ee_w = body_pos_w + quat_apply(body_quat_w, offset) of the frame's body (frame_transformer.py:358)
    const int64_t b = ec * P.NB + P.w[r[IMX_R_IDS_OFF]];
    const float4 bq = reinterpret_cast<const float4*>(S.body_quat_w)[b];
    float ox, oy, oz2;
    quat_apply(bq.x, bq.y, bq.z, bq.w, f_of(r[IMX_R_P1]), f_of(r[IMX_R_P2]), f_of(r[IMX_R_P3]), ox, oy, oz2);
    const float dx = S.object_root_pos_w[ec * 3] - (S.body_pos_w[b * 3] + ox);
    const float dy = S.object_root_pos_w[ec * 3 + 1] - (S.body_pos_w[b * 3 + 1] + oy);
    const float dz = oz - (S.body_pos_w[b * 3 + 2] + oz2);
    return 1.0f - tanhf(sqrtf((dx * dx + dy * dy) + dz * dz) / p0);
}

// ---- navigation/mdp/rewards.py (Isaac-Navigation-Flat-Anymal-C-v0): the (N, 4) pose-2d command in the base frame; in phase 2 of
// k_term_rew_nav.  position_command_error_tanh :17-22: torch.norm(cmd[:, :3], dim=1) = sqrt of the sequential sum of squares;
// heading_command_error_abs :25-29
IMX_DEV float nav_reward(const PlanView& P, const imx_state_t& S, const int32_t* __restrict__ r, int op, int64_t ec) {
    const float* __restrict__ cmd = S.command + ec * P.CMD;
    if (op == IMX_W_NAV_HEADING_COMMAND_ERROR_ABS) return fabsf(cmd[3]);
    const float d = sqrtf((cmd[0] * cmd[0] + cmd[1] * cmd[1]) + cmd[2] * cmd[2]);
    return 1.0f - tanhf(d / f_of(r[IMX_R_P0]));
}

// ---- manipulation/inhand/mdp/rewards.py (Isaac-Repose-Cube-Allegro-v0): the (N, 7) command = goal position in the env frame + goal
// quaternion in the world frame; in phase 2 of k_term_rew_inhand.  dtheta = the env's orientation error, computed once in phase 1.
// track_orientation_inv_l2 :71-96, success_bonus :20-44 (`<=`), track_pos_l2 :47-68: torch.norm(goal_pos_e - object_pos_e) with
// object_pos_e = object_root_pos_w - env_origins
IMX_DEV float inhand_reward(const PlanView& P, const imx_state_t& S, const int32_t* __restrict__ r, int op, int64_t ec, float dtheta) {
    const float p0 = f_of(r[IMX_R_P0]);
    if (op == IMX_W_TRACK_ORIENTATION_INV_L2) return 1.0f / (dtheta + p0);
    if (op == IMX_W_SUCCESS_BONUS) return dtheta <= p0 ? 1.0f : 0.0f;
    const float* __restrict__ cmd = S.command + ec * P.CMD;
    const float dx = cmd[0] - (S.object_root_pos_w[ec * 3] - S.env_origins[ec * 3]);
    const float dy = cmd[1] - (S.object_root_pos_w[ec * 3 + 1] - S.env_origins[ec * 3 + 1]);
    const float dz = cmd[2] - (S.object_root_pos_w[ec * 3 + 2] - S.env_origins[ec * 3 + 2]);
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// ---- manipulation/cabinet/mdp/rewards.py (Isaac-Open-Drawer-Franka-v0); in phase 2 of k_term_rew_cabinet.  fr = the env's frames
// in LDS (row k at fr[k * 64]: 0-2 tcp position, 3-6 tcp quaternion, 7-9 handle position, 10-13 handle quaternion, 14-16 / 17-19 left /
// right fingertip position), computed once per env in phase 1.  J2 = joints of the second articulation (X.joint_pos's row width).
// x and z columns of matrix_from_quat (utils/math.py:144-174): two_s = 2 / sum(q * q); column 0 = (1 - two_s (j j + k k), two_s (i j + k r),
// two_s (i k - j r)), column 1 = (two_s (i j - k r), 1 - two_s (i i + k k), two_s (j k + i r)), column 2 = (two_s (i k + j r),
// two_s (j k - i r), 1 - two_s (i i + j j))
IMX_DEV void quat_matrix_column(float r, float i, float j, float k, int col, float& x, float& y, float& z) {
    const float two_s = 2.0f / (((r * r + i * i) + j * j) + k * k);
    if (col == 0) { x = 1.0f - two_s * (j * j + k * k); y = two_s * (i * j + k * r); z = two_s * (i * k - j * r); }
    else if (col == 1) { x = two_s * (i * j - k * r); y = 1.0f - two_s * (i * i + k * k); z = two_s * (j * k + i * r); }
    else { x = two_s * (i * k + j * r); y = two_s * (j * k - i * r); z = 1.0f - two_s * (i * i + j * j); }
}
IMX_DEV float cabinet_reward(const PlanView& P, const imx_state_t& S, const imx_articulation_state_t& X, const int32_t* __restrict__ r, int op,
                             int64_t ec, const float* __restrict__ fr, int J2) {
    const float p0 = f_of(r[IMX_R_P0]);
    auto F = [&](int k) { return fr[k * 64]; };
    // is_graspable (:88, :112): the right fingertip below the handle and the left one above it
    auto graspable = [&]() { const float hz = F(9); return ((F(19) < hz) && (F(16) > hz)) ? 1.0f : 0.0f; };
    // the drawer joint's position (:143, :155): asset_cfg.joint_ids[0] of the robot or of the second articulation
    auto drawer = [&]() {
        const int j = P.w[r[IMX_R_IDS_OFF]];
        return r[IMX_R_AUX1] ? X.joint_pos[ec * J2 + j] : S.joint_pos[ec * P.J + j];
    };
    switch (op) {
        case IMX_W_APPROACH_EE_HANDLE: case IMX_W_GRASP_HANDLE: {  // :18-40, :117-135: distance = ||handle - tcp||
            const float dx = F(7) - F(0), dy = F(8) - F(1), dz = F(9) - F(2);
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (op == IMX_W_APPROACH_EE_HANDLE) {
                float rw = 1.0f / (1.0f + d * d);
                rw = rw * rw;
                return d <= p0 ? 2.0f * rw : rw;
            }
            const float open = f_of(r[IMX_R_P1]);
            const float s = sum_ids(P.w + r[IMX_R_IDS_OFF], r[IMX_R_NIDS], [&](int j) { return open - S.joint_pos[ec * P.J + j]; });
            return (d <= p0 ? 1.0f : 0.0f) * s;
        }
        case IMX_W_ALIGN_EE_HANDLE: {  // :43-72
            float hxx, hxy, hxz, hyx, hyy, hyz, exx, exy, exz, ezx, ezy, ezz;
            quat_matrix_column(F(10), F(11), F(12), F(13), 0, hxx, hxy, hxz);
            quat_matrix_column(F(10), F(11), F(12), F(13), 1, hyx, hyy, hyz);
            quat_matrix_column(F(3), F(4), F(5), F(6), 0, exx, exy, exz);
            quat_matrix_column(F(3), F(4), F(5), F(6), 2, ezx, ezy, ezz);
            const float az = (ezx * -hxx + ezy * -hxy) + ezz * -hxz;  // bmm(ee_tcp_z, -handle_x)
            const float ax = (exx * -hyx + exy * -hyy) + exz * -hyz;  // bmm(ee_tcp_x, -handle_y)
            const float sz = az > 0.0f ? 1.0f : (az < 0.0f ? -1.0f : 0.0f), sx = ax > 0.0f ? 1.0f : (ax < 0.0f ? -1.0f : 0.0f);
            return 0.5f * (sz * (az * az) + sx * (ax * ax));
        }
        case IMX_W_ALIGN_GRASP_AROUND_HANDLE: return graspable();  // :75-91
        case IMX_W_APPROACH_GRIPPER_HANDLE: {  // :94-114
            const float hz = F(9);
            return graspable() * ((p0 - fabsf(F(16) - hz)) + (p0 - fabsf(F(19) - hz)));
        }
        case IMX_W_OPEN_DRAWER_BONUS: return (graspable() + 1.0f) * drawer();  // :138-146
        case IMX_W_MULTI_STAGE_OPEN_DRAWER: {  // :149-162: open_easy + open_medium + open_hard
            const float q = drawer(), g = graspable();
            return ((q > 0.01f ? 0.5f : 0.0f) + (q > 0.2f ? g : 0.0f)) + (q > 0.3f ? g : 0.0f);
        }
        default: return 0.0f;
    }
}

// scratch layout for k_term_rew (4-byte words, nw = number of env groups; sized for the smallest group: ceil(N/16) groups)
//   [0, nw*KA)               float  per-group partial sums of episode_sums over reset envs
//   [.., + nw*NT)            int    per-group counts of term_dones over reset envs
//   [.., + nw)               int    per-group reset counts
//   [.., + nw*64)            int    per-group compacted local reset ids
struct StepScratch {
    float* log_part;
    int* term_part;
    int* wave_cnt;
    int* ids_local;
};
// envs per workgroup of k_term_rew: every lane of a wave reads its own row of the (N, dof|bodies) state tensors, so a load instruction
// touches one cache line per live lane and the CU's L1 serves one line per clock -- at 4096 envs 64-env groups keep 64 of the 256
// CUs busy walking 64 lines per load (phase 1 measured 9.4 us), 16-env groups spread the same lines over all 256 CUs.  Full waves
// win once there are enough groups to fill the chip anyway.
static inline int step_group_size(int64_t N) { return N <= 8192 ? 16 : (N <= 16384 ? 32 : 64); }
static inline size_t step_scratch_words(int64_t N, int KA, int NT) {
    const size_t nw = (size_t)((N + 15) / 16);
    return nw * KA + nw * NT + nw + nw * 64;
}
static inline StepScratch carve(void* base, int64_t N, int KA, int NT) {
    const size_t nw = (size_t)((N + 15) / 16);
    StepScratch s;
    s.log_part = (float*)base;
    s.term_part = (int*)(s.log_part + nw * KA);
    s.wave_cnt = s.term_part + nw * NT;
    s.ids_local = s.wave_cnt + nw;
    return s;
}

// per-env frame table written by k_frame, read by k_obs: IMX_ES_WORDS floats per env, behind the step scratch
#define IMX_ES_WORDS 24  // 0-2 lin vel b, 3-5 ang vel b, 6-8 projected gravity, 9-11 root pos, 12-15 root quat, 16-17 scanner yaw quat (w, z),
                         // 18-19 free, 20 scanner flags (1 = cast this step, 2 = keep the hit heights), 21-22 sensor x / y, 23 data.pos_w z
static inline size_t frame_offset_bytes(const imx_plan_t* plan, int64_t N) {
    const size_t b = 4 * step_scratch_words(N, plan->nrew_all > 0 ? plan->nrew_all : 1, plan->nterm > 0 ? plan->nterm : 1);
    return (b + 255) & ~(size_t)255;
}

extern "C" size_t imx_plan_scratch_bytes(const imx_plan_t* plan, int64_t num_envs) {
    if (!plan || num_envs <= 0) return 0;
    return frame_offset_bytes(plan, num_envs) + (size_t)num_envs * IMX_ES_WORDS * sizeof(float) + 256;
}

// ------------------------------------------------------------------------------------------------- action affine
// ActionManager.process_action (action_manager.py:318-337): prev <- cur; cur <- a; per term
// processed = raw*scale + offset [clamp]  (joint_actions.py:130-139)
__global__ void k_action(PlanView P, int64_t N, const float* __restrict__ actions, float pre_clip, imx_state_t S,
                         imx_buffers_t Bf) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * P.A) return;
    const int64_t e = i / P.A;
    const int c = (int)(i - e * P.A);
    action_process_element<false>(P, S, Bf, e, c, actions[i], pre_clip);
}
// the same for a plan with a binary joint term (processed width != raw width): the affine tasks' kernel stays as it was
__global__ void k_action_binary(PlanView P, int64_t N, const float* __restrict__ actions, float pre_clip, imx_state_t S, imx_buffers_t Bf) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * P.A) return;
    const int64_t e = i / P.A;
    const int c = (int)(i - e * P.A);
    action_process_element<true>(P, S, Bf, e, c, actions[i], pre_clip);
}

// The height scanner as a SensorBase (sensor_base.py:182-205,287-297; ray_caster.py:107-114,236-237): per-env timestamps decide whether
// this env's rays are cast this step (update_period), a per-env drift re-drawn at reset moves the sensor frame.  One row per env
// {timestamp, last update, drift xyz, data.pos_w z, outdated, step stamp}, advanced by ONE lane per env where the env's frame row is
// produced (the step kernel, which knows the reset flag, or k_frame) -- the observation kernel only reads the outcome from the frame
// row with its other scalar loads: no barrier, no extra round trip there.  The stamp tells a repeated call within the same step
// (ObservationManager.compute() by user code), which repeats the decision instead of advancing the clock again.
// Returns {flags (1 cast, 2 keep hit heights), sensor x, sensor y, data.pos_w z}.
IMX_DEV float4 scanner_step(const PlanView& P, const imx_buffers_t& Bf, int64_t e, uint32_t step, bool was_reset, float rx, float ry, float rz) {
    if (!P.scan_stateful) return make_float4(1.0f, rx, ry, rz);
    const uint64_t seed = (uint64_t)(uint32_t)Bf.counters[4] | ((uint64_t)(uint32_t)Bf.counters[5] << 32);  // the caller's drift seed
    float* row = Bf.scan_state + (size_t)e * 8;
    float ts = row[0], last = row[1], drx = row[2], dry = row[3], drz = row[4], pz_data = row[5];
    bool outdated = row[6] != 0.0f;
    const bool repeat = __float_as_uint(row[7]) == step + 1u;  // stamp = step + 1 (0 = never)
    if (!repeat) {
        for (int k = 0; k < P.scan_substeps; ++k) ts = ts + P.scan_dt;  // SensorBase.update(dt): once per physics step, fp32 like the tensor
        outdated = outdated || (ts - last + 1.0e-6f >= P.scan_period);
    } else {
        outdated = last == ts;  // the first call of this step refreshed the sensor: cast again (same pose, same hits)
    }
    // SensorBase.reset + RayCaster.reset: timers to zero, outdated, new drift.  Also on a repeated call of the same step: env.reset()
    // / env.reset(env_ids) after a step go through k_frame with the stamp k_term_rew left (manager_based_env.py:264-315 -> scene.reset);
    // for an env the step itself reset this repeats the same assignment (same seed, step, env -> same drift).
    if (was_reset) {
        ts = 0.0f; last = 0.0f; outdated = true;
        if (Bf.scan_drift_feed) {
            drx = Bf.scan_drift_feed[e * 3]; dry = Bf.scan_drift_feed[e * 3 + 1]; drz = Bf.scan_drift_feed[e * 3 + 2];
        } else {
            const float w = P.drift_hi - P.drift_lo;  // Tensor.uniform_(lo, hi)
            drx = uniform01(seed ^ 0xD21F7ull, step, (uint64_t)e * 3) * w + P.drift_lo;
            dry = uniform01(seed ^ 0xD21F7ull, step, (uint64_t)e * 3 + 1) * w + P.drift_lo;
            drz = uniform01(seed ^ 0xD21F7ull, step, (uint64_t)e * 3 + 2) * w + P.drift_lo;
        }
    }
    float flags = 0.0f;
    if (outdated) {  // _update_buffers_impl: pos_w = root pos + drift; _update_outdated_buffers: last update <- timestamp
        pz_data = rz + drz;
        last = ts;
        float ts2 = ts;  // will this env's sensor be outdated at the next step?  If not, its hit heights must survive this one
        for (int k = 0; k < P.scan_substeps; ++k) ts2 = ts2 + P.scan_dt;
        flags = !(ts2 - last + 1.0e-6f >= P.scan_period) ? 3.0f : 1.0f;
    }
    float4* o = reinterpret_cast<float4*>(row);
    o[0] = make_float4(ts, last, drx, dry);
    o[1] = make_float4(drz, pz_data, 0.0f, __uint_as_float(step + 1u));
    return make_float4(flags, rx + (outdated ? drx : 0.0f), ry + (outdated ? dry : 0.0f), pz_data);
}

#ifdef IMX_TRACE  // tools/trace_kobs.py only: per-wave start / end stamps (100 MHz wall clock) and placement; never in libimx.so
__device__ uint64_t* g_trace = nullptr;
extern "C" int imx_debug_trace(uint64_t* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf)); }
#endif
#ifdef IMX_TRACE
#define IMX_STAMP(k) do { if (g_trace && lane == 0) g_trace[((size_t)blockIdx.x * 16 + wv) * 8 + (k)] = wall_clock64(); } while (0)
#else
#define IMX_STAMP(k) do { } while (0)
#endif
#define IMX_TR_MAX_WAVES 16
// The end of the step: ordered concatenation of the per-group reset-id lists (reset_env_ids = reset_buf.nonzero(),
// manager_based_rl_env.py:215), the reset count, and the Episode_* log reductions of RewardManager.reset / TerminationManager.reset
// (reward_manager.py:115-121, termination_manager.py:142-144) in a fixed order (deterministic, no float atomics).  ONE workgroup
// runs it after every group's partials are visible: the last-arriving workgroup of k_term_rew, or -- inside env.step() -- an extra
// workgroup of the observation kernel that follows (a kernel boundary instead of a fence + ticket: 4.9 us off the step kernel).
// The work splits in `nparts` workgroups so that it can ride along a kernel of small workgroups: part 0 orders the reset ids, parts
// 1.. share the log entries (each wave re-derives the reset count from the group counts: a handful of loads); nparts == 1 does both.
IMX_DEV void step_tail(const PlanView& P, int64_t N, const imx_buffers_t& Bf, const StepScratch& sc, int G, int part, int nparts) {
    __shared__ int s_scan[IMX_TR_MAX_WAVES];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int nw = (int)((N + G - 1) / G);
    const int TB = blockDim.x;
    const int t = threadIdx.x;
    int total = 0;
    if (part == 0) {
        // exclusive scan of group counts: thread t owns groups [t*chunk, (t+1)*chunk); wave shuffles + per-wave totals
        const int chunk = (nw + TB - 1) / TB;
        int local = 0;
        for (int w = t * chunk; w < min((t + 1) * chunk, nw); ++w) local += __builtin_nontemporal_load(&sc.wave_cnt[w]);
        int incl = local;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_scan[wv] = incl;
        __syncthreads();
        int wave_base = 0;
        for (int w = 0; w < NW; ++w) {
            if (w < wv) wave_base += s_scan[w];
            total += s_scan[w];
        }
        if (t == 0) {
            Bf.counters[0] = total;  // number of reset envs
            // the runner's ep_infos sum (imx_buffers.log_accum): this step's extras["log"] -- refreshed below when something was reset,
            // the entries of the last refresh otherwise -- added to the running sum by the lane that owns the entry
            if (Bf.log_accum) {
                const int kc = P.nrew_all + P.nterm;
                Bf.log_accum[kc] += total > 0 ? (float)total : Bf.log_out[kc];
            }
        }
        int off = wave_base + incl - local;
        for (int w = t * chunk; w < min((t + 1) * chunk, nw); ++w) {
            const int c = __builtin_nontemporal_load(&sc.wave_cnt[w]);
            for (int j = 0; j < c; ++j)
                Bf.reset_env_ids[off + j] = (int64_t)w * G + __builtin_nontemporal_load(&sc.ids_local[w * 64 + j]);
            off += c;
        }
        if (total > 0 && t == 0) Bf.log_out[P.nrew_all + P.nterm] = (float)total;  // (after the read of the old value above: same lane)
        if (nparts > 1) return;
    } else {
        for (int w = lane; w < nw; w += 64) total += __builtin_nontemporal_load(&sc.wave_cnt[w]);
        total = wave_sum_i(total);
    }
    // reference only refreshes extras["log"] when something was reset (:216)
    // one wave per log entry: lanes stride over the groups, fixed-shape shuffle tree -> deterministic
    const int nlog = P.nrew_all + P.nterm;
    const int first = nparts > 1 ? (part - 1) * NW + wv : wv, stride = nparts > 1 ? (nparts - 1) * NW : NW;
    if (total > 0) {
        for (int k = first; k < nlog; k += stride) {
            float v;
            if (k < P.nrew_all) {
                float s = 0.0f;
                for (int w = lane; w < nw; w += 64) s += __builtin_nontemporal_load(&sc.log_part[(size_t)w * P.nrew_all + k]);
                s = wave_sum(s);
                v = s / (float)total / P.max_ep_len_s;
            } else {
                const int kt = k - P.nrew_all;
                int s = 0;
                for (int w = lane; w < nw; w += 64) s += __builtin_nontemporal_load(&sc.term_part[(size_t)w * P.nterm + kt]);
                s = wave_sum_i(s);
                v = (float)s;
            }
            if (lane == 0) {
                Bf.log_out[k] = v;
                if (Bf.log_accum) Bf.log_accum[k] += v;
            }
        }
    } else if (Bf.log_accum) {
        for (int k = first; k < nlog; k += stride)
            if (lane == 0) Bf.log_accum[k] += Bf.log_out[k];
    }
    // the orchestration's entries (imx_reset_orchestrate ran between the step kernel and this tail): Metrics/<command>/error_vel_xy|yaw =
    // mean over the reset envs of the metric before its reset (command_manager.py:123-149), Curriculum/terrain_levels = mean level over ALL
    // envs (curriculums.py:55, curriculum_manager.py:95-118); slots behind the reset count
    if (Bf.ev_part) {
        const int ng = (int)((N + 63) / 64);
        for (int j = first; j < 3; j += stride) {
            if (!((Bf.ev_flags >> (j < 2 ? 0 : 1)) & 1)) continue;
            const int slot = nlog + 1 + j;
            if (total > 0) {
                float s = 0.0f;
                for (int w = lane; w < ng; w += 64) s += __builtin_nontemporal_load(&Bf.ev_part[(size_t)w * 4 + j]);
                s = wave_sum(s);
                const float v = j < 2 ? s / (float)total : s / (float)N;
                if (lane == 0) {
                    Bf.log_out[slot] = v;
                    if (Bf.log_accum) Bf.log_accum[slot] += v;
                }
            } else if (Bf.log_accum && lane == 0) {
                Bf.log_accum[slot] += Bf.log_out[slot];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- terminations + rewards
// Block = G consecutive envs x NW waves (NW <= 16).  Lane l of every wave owns env G*blockIdx + l ("env per lane").  The work items --
// nterm termination terms, then nrew reward terms -- are dealt round-robin to the waves, so that the state loads of ALL terms of an
// env are in flight together and the kernel is two memory round trips deep, not one chain per term:
//   phase 0  root state (and the episodic sum of the wave's first reward item) -- no table needed, issued first;
//   phase 1  each wave evaluates its items: record and id list through the scalar cache (wave-uniform, L2-resident), state loads,
//            a termination's bit into an LDS mask, a reward's RAW function value f and the env's running episodic sum into LDS;
//   phase 2  with every termination known (is_alive / is_terminated / the reset flag need them), each wave finishes its reward
//            items: value = f * weight * dt, episodic sum, step_reward, reset-log partial;
//   phase 3  wave 0 adds the values IN TERM ORDER (bit-identical to the reference's sequential `+=`), writes the env outputs and
//            the ordered reset ids of the group; the other waves store term_dones and the termination-log counts.
// What the per-wave timeline (tools/trace_step.py) showed on the way here: a memory round trip costs ~2 us at this size, the previous
// layout (8 waves, two terms per wave back to back, 64-env groups) walked ~6 of them in a row (24 us); with one item per wave the
// critical path became the SLOWEST item's instruction count -- the force-history terms evaluated 8 padded slots x 4 history slots
// with a square root each (9.7 us for undesired_contacts against 2 us for a joint sum) -- hence exact trip counts and one square
// root per body (max_hist_force), and the end of the step moved out of the kernel (step_tail: 4.9 us of fence + ticket).
// CLASSIC: the plan has reward ops of classic/humanoid/mdp (classic_reward, progress_reward's term_state).  Their code lives in this
// instantiation only: k_term_rew sits at 128 VGPRs, and any further code in the one shared kernel made it spill (36 to 84 bytes per
// lane at compile time, one extra case alone enough) -- so every other plan runs the kernel exactly as it was.
// REACH: the plan has reward ops of manipulation/reach/mdp (reach_reward), evaluated in a third instantiation for the same reason.
// LIFT: the plan has terms that read the scene's rigid object (manipulation/lift/mdp, root_height_below_minimum on the object), next to
// the reach ops in a kernel of its own, k_term_rew_lift -- the reach instantiation went from 16 to 108 bytes of scratch with them inline.
// Both kernels include the one body, term_rew_body.inc.
template <bool CLASSIC, bool REACH>
__global__ void __launch_bounds__(64 * IMX_TR_MAX_WAVES)
k_term_rew(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, StepScratch sc, float* __restrict__ frame, int G, int defer_tail,
           imx_rollout_slot_t ro) {
#include "term_rew_body.inc"
}
__global__ void __launch_bounds__(64 * IMX_TR_MAX_WAVES)
k_term_rew_lift(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, StepScratch sc, float* __restrict__ frame, int G, int defer_tail,
                imx_rollout_slot_t ro) {
    constexpr bool CLASSIC = false;  // (with IMX_TR_LIFT the body runs the reach and the lift ops unconditionally)
#define IMX_TR_LIFT
#include "term_rew_body.inc"
#undef IMX_TR_LIFT
}

// NAV: the navigation task's two reward ops, in a kernel of their own like the lift ops (the shared instantiations stay as they were).
__global__ void __launch_bounds__(64 * IMX_TR_MAX_WAVES)
k_term_rew_nav(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, StepScratch sc, float* __restrict__ frame, int G, int defer_tail,
               imx_rollout_slot_t ro) {
    constexpr bool CLASSIC = false, REACH = false;
#define IMX_TR_NAV
#include "term_rew_body.inc"
#undef IMX_TR_NAV
}

// INHAND: the in-hand task's three reward and three termination ops (manipulation/inhand/mdp), in a kernel of their own for the same
// reason.  need_dtheta: a reward of the plan reads the orientation error (the host looks at the ops): it is then computed once per env.
__global__ void __launch_bounds__(64 * IMX_TR_MAX_WAVES)
k_term_rew_inhand(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, StepScratch sc, float* __restrict__ frame, int G, int defer_tail,
                  imx_rollout_slot_t ro, int need_dtheta, imx_object_state_t X) {
    constexpr bool CLASSIC = false, REACH = false;
#define IMX_TR_INHAND
#include "term_rew_body.inc"
#undef IMX_TR_INHAND
}

// CABINET: the Open-Drawer task's seven reward ops (manipulation/cabinet/mdp/rewards.py), in a kernel of their own for the same reason.
// X = the second articulation's tensors (the cabinet), ft_off = the plan's frame table, fingers: a reward of the plan reads the
// fingertip frames (the host looks at the ops).  The env's frames are computed once, by the last wave, into 20 more rows of LDS.
__global__ void __launch_bounds__(64 * IMX_TR_MAX_WAVES)
k_term_rew_cabinet(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, StepScratch sc, float* __restrict__ frame, int G, int defer_tail,
                   imx_rollout_slot_t ro, int ft_off, int fingers, imx_articulation_state_t X) {
    constexpr bool CLASSIC = false, REACH = false;
#define IMX_TR_CABINET
#include "term_rew_body.inc"
#undef IMX_TR_CABINET
}

// ------------------------------------------------------------------------------------------------- observations
// One WAVE = one environment (4 envs per 256-thread block).  Every lane first derives the env's root-frame vectors
// and scanner yaw from the same 13 root-state floats (wave-uniform loads: one transaction, no LDS, no barrier);
// then lane l produces the output columns xcol[l], xcol[l+64], ... (ray columns first) and stores obs[e*D + c]:
// within a term the 64 lanes of a wave write 64 consecutive floats.
//
// xcol is the per-column expansion of the observation records built once by imx_plan_create (16 words per column:
// everything a lane needs arrives with four 16-byte loads instead of a chain order -> column -> record -> id table).
// Height-scanner rays (yaw-only frame, vertical direction) take a fast path that keeps up to four rays of a lane
// in flight: cell-table loads of all four, then the 48-byte triangle records of all four, then the Woop tests.
#define IMX_OBS_ENVS_PER_BLOCK 4

// ObservationTermCfg.modifiers (observation_manager.py:310-312; utils/modifiers/modifier.py): the term's modifier program,
// run on the raw value of ONE element; filter / integrator state of that element lives in the env's mod_state row at
// st[(soff + k) * d] (element-minor, so the lanes of a term touch consecutive floats).  `zero`: the env was reset this step
// (ObservationManager.reset zeroes the state before the next compute) -- old state is ignored, new state is written.
IMX_DEV float apply_modifiers(const int32_t* __restrict__ W, int xmod, float v, float* __restrict__ row, bool zero) {
    const int4 m = *reinterpret_cast<const int4*>(W + xmod);
    const int po = m.x, pn = m.y, d = m.w;
    float* st = row + m.z;
    for (int q = 0; q < pn; q += 4) {
        const int op = W[po + q];
        const float a = f_of(W[po + q + 1]), b = f_of(W[po + q + 2]);
        const int soff = W[po + q + 3];
        switch (op) {
            case IMX_M_SCALE: v = v * a; break;
            case IMX_M_BIAS: v = v + a; break;
            case IMX_M_CLIP: v = clip_keep_nan(v, a, b); break;
            case IMX_M_INTEGRATOR: {  // integral += (data + y_prev) / 2 * dt; y_prev = data (modifier.py:247-259)
                float* s = st + soff * d;
                const float yp = zero ? 0.0f : s[d];
                const float integ = (zero ? 0.0f : s[0]) + (v + yp) / 2.0f * a;
                s[0] = integ; s[d] = v;
                v = integ;
            } break;
            case IMX_M_DIGITAL_FILTER: {  // y = x_n . B - y_n . A with both windows rolled by one (modifier.py:160-176)
                const int na = W[po + q + 1], nb = W[po + q + 2];
                float* xs = st + soff * d;
                float* ys = xs + nb * d;
                const int32_t* A = W + po + q + 4;
                const int32_t* B = A + na;
                float accx = 0.0f, accy = 0.0f, carry = v;
                for (int k = 0; k < nb; ++k) {
                    const float old = zero ? 0.0f : xs[k * d];
                    xs[k * d] = carry;
                    accx += carry * f_of(B[k]);
                    carry = old;
                }
                for (int k = 0; k < na; ++k) accy += (zero ? 0.0f : ys[k * d]) * f_of(A[k]);
                const float y = accx - accy;
                carry = y;
                for (int k = 0; k < na; ++k) {
                    const float old = zero ? 0.0f : ys[k * d];
                    ys[k * d] = carry;
                    carry = old;
                }
                v = y;
                q += na + nb;
            } break;
            default: break;
        }
    }
    return v;
}

// k_frame: one lane per env -- root-frame vectors (ArticulationData.root_lin_vel_b / root_ang_vel_b /
// projected_gravity_b), sensor position and the yaw-only sensor quaternion (yaw_quat, utils/math.py:521-542), once per
// env per step instead of once per wave of k_obs (PMC: the transcendental prologue was ~40 % of k_obs's VALU work).
__global__ void __launch_bounds__(64)
k_frame(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, float* __restrict__ frame, int fill_all) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const float4 q4 = reinterpret_cast<const float4*>(S.root_quat_w)[e];
    float4 o[5];
    quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, S.root_lin_vel_w[e * 3], S.root_lin_vel_w[e * 3 + 1],
                        S.root_lin_vel_w[e * 3 + 2], o[0].x, o[0].y, o[0].z);
    quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, S.root_ang_vel_w[e * 3], S.root_ang_vel_w[e * 3 + 1],
                        S.root_ang_vel_w[e * 3 + 2], o[0].w, o[1].x, o[1].y);
    quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, P.gx, P.gy, P.gz, o[1].z, o[1].w, o[2].x);
    o[2].y = S.root_pos_w[e * 3]; o[2].z = S.root_pos_w[e * 3 + 1]; o[2].w = S.root_pos_w[e * 3 + 2];
    o[3] = q4;
    o[4] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    if (P.R > 0 && P.ray_yaw_only) yaw_quat_wz(q4.x, q4.y, q4.z, q4.w, o[4].x, o[4].y);
    float4* dst = reinterpret_cast<float4*>(frame) + e * 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) dst[k] = o[k];
    if (P.R > 0)
        dst[5] = scanner_step(P, Bf, e, (uint32_t)Bf.counters[2], fill_all || (Bf.reset_buf && Bf.reset_buf[e]), o[2].y, o[2].z, o[2].w);
}


// k_obs: one BLOCK = one environment, one lane = one output column (ray columns first in xcol).  No prologue, no
// barrier: the env's 20-float frame is read with wave-uniform loads (scalar cache), then every lane is an independent,
// register-light stream: xcol (four 16-byte loads) -> value -> noise/clip/scale -> obs[e*D + c]; consecutive lanes
// write consecutive floats of one obs row.  The ray path is cast_ray_vertical (imx_raycast.h): cell descriptor and
// the four shared lattice corners are loaded together -- one dependent memory level per ray on height-field terrain.

// modifiers -> noise -> clip -> scale -> history window -> obs[e][c] for computed column i (observation_manager.py:305-335)
// LEAN: the plan has one observation group, no modifiers and no history windows (every task config of BASELINE.json) -- the code for
// those features is compiled out, which is worth registers (= resident waves) to every launch that does not need them.
template <bool LEAN>
IMX_DEV void obs_finish(const PlanView& P, const imx_buffers_t& Bf, const XCol& x, int i, float v, int64_t e, int corrupt,
                        bool fill_all, const float* __restrict__ noise_u, uint64_t seed, uint32_t step) {
    const int c = x.a.x;
    if (LEAN) {
        Bf.obs[e * P.gD[0] + c] = obs_post<false>(x, v, corrupt & P.gcorrupt, noise_u, seed, step, e, P.D, 0);
        return;
    }
    const int g = (x.a.w >> 8) & 3;  // observation group of this column (ObservationManager.compute loops over the groups)
    const int gD = g == 0 ? P.gD[0] : (g == 1 ? P.gD[1] : (g == 2 ? P.gD[2] : P.gD[3]));
    const int gb = g == 0 ? 0 : (g == 1 ? P.gbase[1] : (g == 2 ? P.gbase[2] : P.gbase[3]));
    float* grow = g == 0 ? Bf.obs : (g == 1 ? Bf.obs_extra1 : (g == 2 ? Bf.obs_extra2 : Bf.obs_extra3));
    if (x.a.w & IMX_F_MODIFIERS)
        v = apply_modifiers(P.w, P.xmod_off + 4 * i, v, Bf.mod_state + e * P.MS, fill_all || Bf.reset_buf[e]);
    const float vp = obs_post<true>(x, v, corrupt & (P.gcorrupt >> g), noise_u, seed, step, e, P.D, gb);
    float* o = grow + e * gD + c;  // newest slot
    const int hist = x.d.z;
    if (hist > 1) {
        // CircularBuffer.append (utils/buffers/circular_buffer.py:107-135) on the window kept in the obs row itself: this
        // lane owns element j of every slot.  Envs reset this step (or all, at env.reset) have zero pushes: every slot
        // takes the first value; otherwise the window slides by one.
        const int hs = x.d.w;
        if (fill_all || Bf.reset_buf[e]) {
            for (int h = 1; h < hist; ++h) o[-h * hs] = vp;
        } else {
            for (int h = hist - 1; h >= 1; --h) o[-h * hs] = o[-(h - 1) * hs];
        }
    }
    *o = vp;
}


// One ray of the scanner: RayCaster._update_buffers_impl (ray_caster.py:242-260) -> hit height (+inf on a miss, ops.py:70)
template <bool GENERAL_RAYS>
IMX_DEV float scan_ray(const PlanView& P, const MeshView& M, const float* __restrict__ es, const float* __restrict__ ray_local, int j,
                       float px, float py, float pz, float yw, float yz, float* __restrict__ ray_hits_out, int64_t e) {
    const float3 l3 = reinterpret_cast<const float3*>(ray_local)[j];  // one 12-byte load
    const float lx = l3.x, ly = l3.y, lz = l3.z;
    float sx, sy, sz, dx = P.rdx, dy = P.rdy, dz = P.rdz;
    if (!GENERAL_RAYS || P.ray_yaw_only) {  // (the vertical-ray variant is only launched for a yaw-aligned sensor)
        quat_apply_yaw_only(yw, yz, lx, ly, lz, sx, sy, sz);
    } else {  // ray_caster.py:249-252: full orientation for starts and directions
        quat_apply(es[12], es[13], es[14], es[15], lx, ly, lz, sx, sy, sz);
        quat_apply(es[12], es[13], es[14], es[15], P.rdx, P.rdy, P.rdz, dx, dy, dz);
    }
    sx += px; sy += py; sz += pz;
    float t;
    int32_t face;
    const bool hit = GENERAL_RAYS ? cast_ray(M, sx, sy, sz, dx, dy, dz, P.ray_max_dist, t, face)
                                  : cast_ray_vertical(M, sx, sy, sz, dz, P.rinv_dz, P.ray_max_dist, t, face);
    const float hz = hit ? sz + t * dz : __builtin_huge_valf();  // kernels.py:69
    if (ray_hits_out) {
        float* o = ray_hits_out + ((size_t)e * P.R + j) * 3;
        o[0] = hit ? sx + t * dx : __builtin_huge_valf();
        o[1] = hit ? sy + t * dy : __builtin_huge_valf();
        o[2] = hz;
    }
    return hz;
}

// The observation kernel of a LEAN plan with a height scanner (one observation group, no modifier programs, no history windows: every
// rough-terrain task config of BASELINE.json).  Workgroup = ONE WAVE: wave `role` of env e casts rays 64*role .. 64*role+63 and finishes
// THEIR height_scan columns on the spot -- the term's offset / noise / clip / scale are the same for all R columns, so they travel in
// scalar registers (one record, scalar loads) instead of a 16-word column record per lane; the env's last wave fills its other columns
// (base velocity, joints, actions ...).  No LDS, no barrier: the sensor's per-step decision (cast? where? keep the hits?) sits in the
// frame row, put there by the kernel that produced the row.  Single-wave workgroups because what bounds this kernel is how fast the
// chip re-fills wave slots after the first residency round (tools/trace_kobs.py): a one-wave workgroup fits any free slot, a four-wave
// one needs four on one CU.
template <bool GENERAL_RAYS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(IMX_LEAN_SGPRS)))
k_obs_lean(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, MeshView M, const float* __restrict__ frame,
           const float* __restrict__ noise_u, uint64_t seed, int corrupt, float* __restrict__ ray_hits_out, StepScratch sc, int tail_G,
           int tail_parts, int scan_rec, int waves_per_env, uint32_t div_magic, int div_shift, const int32_t* __restrict__ W) {
    // (W = P.w once more, as a kernel argument of its own: `noalias` there is what lets the compiler read the term record through the
    // scalar cache instead of four vector loads + v_readfirstlane per wave)
    if ((int)blockIdx.x < tail_parts) {  // extra workgroups, first in the grid: the step tail k_term_rew deferred (kernel boundary = its partials are complete)
        step_tail(P, N, Bf, sc, tail_G, (int)blockIdx.x, tail_parts);
        return;
    }
    const bool role_major = waves_per_env < 0;
    if (role_major) waves_per_env = -waves_per_env;
    const uint32_t step = (uint32_t)Bf.counters[2];
    const bool fill_all = (corrupt & 2) != 0;
    const bool keep_all_hits = (corrupt & 8) != 0;
    corrupt &= 1;
    const int D = P.gD[0];
    // One wave per work item (env, role).  (Persistent waves -- as many as the chip holds, each walking the items with the grid's
    // stride -- were measured: 265 us against 204 at 65 536 envs, 21.5 against 19.7 at 4096; more resident waves only made each slower.)
    const unsigned b = blockIdx.x - (unsigned)tail_parts;
    int64_t e;
    int role;
    // b / divisor by multiply-high with the host's magic number (two scalar instructions instead of the ~25 of a 32-bit division)
    const uint32_t q = (uint32_t)(((uint64_t)b * div_magic) >> 32) >> div_shift;
    if (!role_major) {
        e = q;
        role = (int)(b - q * (unsigned)waves_per_env);
    } else {  // role-major order (the host's choice for small grids)
        role = (int)q;
        e = b - q * (unsigned)N;
    }
    const float* __restrict__ es = frame + e * IMX_ES_WORDS;  // wave-uniform address
    if (role < waves_per_env - 1) {
        // the ray's local start depends on the lane only: requested before the first answer of the frame row is looked at (one round
        // trip of the wave's life less: frame row and ray table travel together)
        const int j0 = role * 64 + (int)threadIdx.x;
        const float3 l3_early = reinterpret_cast<const float3*>(W + P.ray_off)[j0 < P.R ? j0 : P.R - 1];
        // height_scan (observations.py:165-173): sensor.data.pos_w z - hit z - offset, then noise -> clip -> scale (observation_manager.py:313-318)
        const int sflags = (int)es[20];
        const bool cast = (sflags & 1) != 0, cache_z = P.scan_stateful && ((sflags & 2) || keep_all_hits);
        const float px = es[21], py = es[22], pz = es[23];
        const int32_t* r = W + P.obs_off + scan_rec * IMX_REC_WORDS;
        const int out = r[IMX_R_OUT], flags = r[IMX_R_FLAGS];
        const float off = f_of(r[IMX_R_P0]), nlo = f_of(r[IMX_R_NOISE_LO]), nhi = f_of(r[IMX_R_NOISE_HI]);
        const float clo = f_of(r[IMX_R_CLIP_LO]), chi = f_of(r[IMX_R_CLIP_HI]), scale = f_of(r[IMX_R_SCALE]);
        const bool noisy = (corrupt & P.gcorrupt) && (flags & (IMX_F_NOISE_ADD | IMX_F_NOISE_SCALE | IMX_F_NOISE_ABS));
        const float* __restrict__ ray_local = reinterpret_cast<const float*>(W + P.ray_off);
        const float yw = es[16], yz = es[17];
        const int j = role * 64 + (int)threadIdx.x;  // one ray per lane
        const bool has = j < P.R;  // (no early exit: the wave casts together, see cast_ray_vertical_wave)
        // per-env bases are wave-uniform (scalar); the lane adds a 32-bit column offset
        float* __restrict__ obs_row = Bf.obs + e * D;
        float* __restrict__ hitz_row = P.scan_stateful ? Bf.scan_hit_z + (size_t)e * P.R : nullptr;
        float hz = 0.0f;
        if (cast && !GENERAL_RAYS) {
            // RayCaster._update_buffers_impl (ray_caster.py:242-260), yaw-aligned sensor, vertical rays: start = yaw(q) * local + sensor pos
            const float3 l3 = l3_early;
            float sx, sy, sz, t = 0.0f;
            quat_apply_yaw_only(yw, yz, l3.x, l3.y, l3.z, sx, sy, sz);
            sx += px; sy += py; sz += pz;
            const bool hit = cast_ray_vertical_wave(M, has, sx, sy, sz, P.rdz, P.rinv_dz, P.ray_max_dist, t);
            hz = hit ? sz + t * P.rdz : __builtin_huge_valf();  // kernels.py:69
            if (ray_hits_out && has) {
                float* o = ray_hits_out + ((size_t)e * P.R + j) * 3;
                o[0] = hit ? sx + t * P.rdx : __builtin_huge_valf();
                o[1] = hit ? sy + t * P.rdy : __builtin_huge_valf();
                o[2] = hz;
            }
        } else if (cast && has) {
            hz = scan_ray<GENERAL_RAYS>(P, M, es, ray_local, j, px, py, pz, yw, yz, ray_hits_out, e);
        }
        if (!has) return;
        if (cast) {
            if (cache_z) hitz_row[(unsigned)j] = hz;
        } else {
            hz = hitz_row[(unsigned)j];  // data.ray_hits_w of the last update
        }
        float v = pz - hz - off;
        const int c = out + j;
        if (noisy) {
            const float nz = noise_sample<false>(flags, nlo, nhi, noise_u, seed, step, e, P.D, c);
            v = (flags & IMX_F_NOISE_ADD) ? v + nz : ((flags & IMX_F_NOISE_SCALE) ? v * nz : nz);
        }
        if (flags & IMX_F_CLIP) v = clip_keep_nan(v, clo, chi);
        if (flags & IMX_F_SCALE) v = v * scale;
        obs_row[(unsigned)c] = v;
    } else {
        if (e == 0 && threadIdx.x == 0) Bf.counters[3] = (int32_t)step;  // the shadow the next step kernel counts on from
        for (int i = P.n_ray_cols + (int)threadIdx.x; i < P.DC; i += 64) {  // xcol lists the ray columns first
            const XCol x = load_xcol(W, P.xcol_off, i);
            obs_finish<true>(P, Bf, x, i, obs_plain_value<false>(P, S, Bf, es, e, x), e, corrupt, fill_all, noise_u, seed, step);
        }
    }
}

template <bool GENERAL_RAYS, bool LEAN>
__global__ void __launch_bounds__(256)
k_obs(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, MeshView M, const float* __restrict__ frame,
      const float* __restrict__ noise_u, uint64_t seed, int corrupt, float* __restrict__ ray_hits_out, StepScratch sc, int tail_G,
      int tail_parts) {
#include "obs_body.inc"
}

// INHAND: a plan whose observations read the rigid object's root state (root_pos_w / root_quat_w / root_lin_vel_w / root_ang_vel_w with
// asset word 1) or goal_quat_diff (Isaac-Repose-Cube-Allegro-v0) runs the same body in a kernel of its own, with the general ray path
// (a plan without a height scanner casts nothing): k_obs<...> and k_obs_lean<...> stay the instruction streams they were.
template <bool LEAN>
__global__ void __launch_bounds__(256)
k_obs_inhand(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, MeshView M, const float* __restrict__ frame,
             const float* __restrict__ noise_u, uint64_t seed, int corrupt, float* __restrict__ ray_hits_out, StepScratch sc, int tail_G,
             int tail_parts, imx_object_state_t X) {
    constexpr bool GENERAL_RAYS = true;
#define IMX_OBS_INHAND
#include "obs_body.inc"
#undef IMX_OBS_INHAND
}

// CABINET: a plan whose observations read FrameTransformer frames (manipulation/cabinet/mdp/observations.py) or the second
// articulation's joints (Isaac-Open-Drawer-Franka-v0) runs the same body in a kernel of its own, like the in-hand plans.
template <bool LEAN>
__global__ void __launch_bounds__(256)
k_obs_cabinet(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, MeshView M, const float* __restrict__ frame,
              const float* __restrict__ noise_u, uint64_t seed, int corrupt, float* __restrict__ ray_hits_out, StepScratch sc, int tail_G,
              int tail_parts, imx_articulation_state_t X) {
    constexpr bool GENERAL_RAYS = true;
#define IMX_OBS_CABINET
#include "obs_body.inc"
#undef IMX_OBS_CABINET
}

// IMU: a plan whose observations read an Imu sensor's data (imu_orientation / imu_ang_vel / imu_lin_acc, envs/mdp/observations.py:188-231;
// X = the tensors imx_plan_bind_imu bound) runs the same body in a kernel of its own, like the in-hand and cabinet plans.
template <bool LEAN>
__global__ void __launch_bounds__(256)
k_obs_imu(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, MeshView M, const float* __restrict__ frame,
          const float* __restrict__ noise_u, uint64_t seed, int corrupt, float* __restrict__ ray_hits_out, StepScratch sc, int tail_G,
          int tail_parts, ImuObsView X) {
    constexpr bool GENERAL_RAYS = true;
#define IMX_OBS_IMU
#include "obs_body.inc"
#undef IMX_OBS_IMU
}

// ------------------------------------------------------------------------------------------------- root frame
__global__ void k_root_frame(int64_t N, const float* __restrict__ q, const float* __restrict__ lv,
                             const float* __restrict__ av, float gx, float gy, float gz, float* __restrict__ olv,
                             float* __restrict__ oav, float* __restrict__ opg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const float w = q[e * 4], x = q[e * 4 + 1], y = q[e * 4 + 2], z = q[e * 4 + 3];
    float a, b, c;
    if (olv) { quat_rotate_inverse(w, x, y, z, lv[e * 3], lv[e * 3 + 1], lv[e * 3 + 2], a, b, c); olv[e * 3] = a; olv[e * 3 + 1] = b; olv[e * 3 + 2] = c; }
    if (oav) { quat_rotate_inverse(w, x, y, z, av[e * 3], av[e * 3 + 1], av[e * 3 + 2], a, b, c); oav[e * 3] = a; oav[e * 3 + 1] = b; oav[e * 3 + 2] = c; }
    if (opg) { quat_rotate_inverse(w, x, y, z, gx, gy, gz, a, b, c); opg[e * 3] = a; opg[e * 3 + 1] = b; opg[e * 3 + 2] = c; }
}

// ------------------------------------------------------------------------------------------------- raycast_mesh
__global__ void k_raycast(MeshView M, const float* __restrict__ starts, const float* __restrict__ dirs, int64_t n,
                          float max_dist, float* __restrict__ hits, float* __restrict__ dist, int32_t* __restrict__ faces) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float ox = starts[i * 3], oy = starts[i * 3 + 1], oz = starts[i * 3 + 2];
    const float dx = dirs[i * 3], dy = dirs[i * 3 + 1], dz = dirs[i * 3 + 2];
    float t;
    int32_t f;
    const float inf = __builtin_huge_valf();
    if (cast_ray(M, ox, oy, oz, dx, dy, dz, max_dist, t, f)) {
        hits[i * 3] = ox + t * dx; hits[i * 3 + 1] = oy + t * dy; hits[i * 3 + 2] = oz + t * dz;
        if (dist) dist[i] = t;
        if (faces) faces[i] = f;
    } else {
        hits[i * 3] = inf; hits[i * 3 + 1] = inf; hits[i * 3 + 2] = inf;
        if (dist) dist[i] = inf;
        if (faces) faces[i] = -1;
    }
}

// ------------------------------------------------------------------------------------------------- C ABI
// Magic number for floor(b / d), 0 <= b < 2^31, d >= 2: q = mulhi(b, magic) >> shift.  With l = ceil(log2 d) and magic =
// floor(2^(31+l) / d) + 1 (< 2^32 because d > 2^(l-1)), b * magic / 2^(31+l) = b/d + eps with eps < 2^31 * d / (d * 2^(31+l)) <= 1/d:
// never enough to carry frac(b/d) <= (d-1)/d over the next integer.
static void imx_magic_u31(uint32_t d, uint32_t& magic, int& shift) {
    int l = 1;
    while ((1ull << l) < d) ++l;
    magic = (uint32_t)(((1ull << (31 + l)) / d) + 1);
    shift = l - 1;
}

static int check_common(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf) {
    IMX_REQUIRE(plan && st && bf, "null plan/state/buffers");
    IMX_REQUIRE(plan->dev, "plan has no device copy (no GPU visible when it was created)");
    IMX_REQUIRE(N > 0 && N < (1ll << 31), "num_envs out of range: %lld", (long long)N);
    return 0;
}

int imx_check_action_inputs(const imx_plan_t* plan, const imx_state_t* st, const imx_buffers_t* bf, const char* who) {
    IMX_REQUIRE(bf->action && bf->prev_action && bf->processed_action, "%s: null action buffer", who);
    IMX_REQUIRE(plan->A > 0, "%s: plan has no action columns", who);
    for (int k = 0; k < plan->nact; ++k) {
        const int flags = plan->host[plan->act_off + k * IMX_REC_WORDS + IMX_R_FLAGS];
        if (flags & IMX_F_ACT_DEFAULT_POS_OFFSET) IMX_REQUIRE(st->default_joint_pos, "%s: default_joint_pos missing", who);
        if (flags & IMX_F_ACT_DEFAULT_VEL_OFFSET) IMX_REQUIRE(st->default_joint_vel, "%s: default_joint_vel missing", who);
        if (flags & (IMX_F_ACT_TO_LIMITS | IMX_F_ACT_EMA)) IMX_REQUIRE(st->soft_joint_pos_limits, "%s: soft_joint_pos_limits missing", who);
        if (flags & IMX_F_ACT_EMA) IMX_REQUIRE(st->joint_pos, "%s: joint_pos missing", who);
    }
    return 0;
}

// The body poses frame `index` of the plan's frame table reads (0 = the ee_frame's source, 1.. its targets, then the cabinet_frame's
// source and targets): the robot's in the state struct or the second articulation's bound to the plan, by the frame's asset word.
// who = "a term" | "an observation term".
static int need_frame_inputs(const imx_plan_t* plan, const imx_state_t* st, int index, const char* who) {
    const int32_t* fr = &plan->host[plan->ft_off + IMX_FT_HEADER_WORDS + index * IMX_FRAME_WORDS];
    const float* pos = fr[1] ? plan->articulation_state.body_pos_w : st->body_pos_w;
    const float* quat = fr[1] ? plan->articulation_state.body_quat_w : st->body_quat_w;
    IMX_REQUIRE(pos, "state tensor '%s' is required by %s but missing", fr[1] ? "articulation_state.body_pos_w" : "body_pos_w", who);
    IMX_REQUIRE(quat, "state tensor '%s' is required by %s but missing", fr[1] ? "articulation_state.body_quat_w" : "body_quat_w", who);
    return 0;
}

extern "C" int imx_action_process(const imx_plan_t* plan, int64_t N, const float* actions_d, float pre_clip,
                                  const imx_state_t* st, const imx_buffers_t* bf, imx_stream_t stream) {
    if (check_common(plan, N, st, bf)) return 1;
    IMX_REQUIRE(actions_d, "imx_action_process: null actions");
    if (imx_check_action_inputs(plan, st, bf, "imx_action_process")) return 1;
    const int64_t n = N * plan->A;
    const int bs = 256;
    bool binary = plan->PA != plan->A;
    for (int k = 0; k < plan->nact; ++k) binary = binary || plan->host[plan->act_off + k * IMX_REC_WORDS + IMX_R_OP] == IMX_A_BINARY_JOINT;
    hipLaunchKernelGGL(binary ? k_action_binary : k_action, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, (hipStream_t)stream,
                       imx_plan_view(plan), N, actions_d, pre_clip, *st, *bf);
    IMX_HIP(hipGetLastError());
    return 0;
}

extern "C" int imx_terminations_rewards(const imx_plan_t* plan, int64_t N, const imx_state_t* st,
                                        const imx_buffers_t* bf, int flags, imx_stream_t stream) {
    return imx_terminations_rewards_rollout(plan, N, st, bf, flags, nullptr, stream);
}

extern "C" int imx_terminations_rewards_rollout(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                                                int flags, const imx_rollout_slot_t* slot, imx_stream_t stream) {
    if (check_common(plan, N, st, bf)) return 1;
    imx_rollout_slot_t ro{};
    if (slot) {
        ro = *slot;
        IMX_REQUIRE(ro.value_t && ro.rewards_out && ro.dones_out, "imx_terminations_rewards_rollout: value_t, rewards_out and dones_out are required");
        IMX_REQUIRE((ro.cur_reward_sum == nullptr) == (ro.cur_ep_len == nullptr), "imx_terminations_rewards_rollout: episode buffers come together");
        IMX_REQUIRE(!ro.ep_stats3 || ro.cur_reward_sum, "imx_terminations_rewards_rollout: ep_stats3 needs the episode buffers");
    }
    IMX_REQUIRE(st->root_quat_w && st->root_lin_vel_w && st->root_ang_vel_w, "root state missing");
    IMX_REQUIRE(bf->episode_length_buf && bf->reward_buf && bf->episode_sums && bf->step_reward && bf->term_dones &&
                    bf->terminated && bf->truncated && bf->reset_buf && bf->reset_env_ids && bf->counters &&
                    bf->log_out && bf->scratch && bf->action && bf->prev_action,
                "imx_terminations_rewards: null buffer");
    // inputs each op dereferences must be present
    const auto& w = plan->host;
    auto need = [&](const void* p, const char* name) -> int {
        IMX_REQUIRE(p, "state tensor '%s' is required by a term but missing", name);
        return 0;
    };
    for (int k = 0; k < plan->nterm; ++k) {
        switch (w[plan->term_off + k * IMX_REC_WORDS + IMX_R_OP]) {
            case IMX_T_ILLEGAL_CONTACT: if (need(st->net_forces_w_history, "net_forces_w_history")) return 1; break;
            case IMX_T_JOINT_POS_MANUAL_LIMIT: if (need(st->joint_pos, "joint_pos")) return 1; break;
            case IMX_T_ROOT_HEIGHT_BELOW_MIN:
                if (w[plan->term_off + k * IMX_REC_WORDS + IMX_R_AUX0] ? need(st->object_root_pos_w, "object_root_pos_w") : need(st->root_pos_w, "root_pos_w")) return 1;
                break;
            case IMX_T_TERRAIN_OUT_OF_BOUNDS: if (need(st->root_pos_w, "root_pos_w")) return 1; break;
            case IMX_T_OBJECT_REACHED_GOAL:
                if (need(st->command, "command") || need(st->root_pos_w, "root_pos_w") || need(st->object_root_pos_w, "object_root_pos_w")) return 1;
                break;
            case IMX_T_MAX_CONSECUTIVE_SUCCESS: if (need(plan->object_state.command_consecutive_success, "command_consecutive_success")) return 1; break;
            case IMX_T_OBJECT_AWAY_FROM_GOAL:
                if (need(st->command, "command") || need(st->env_origins, "env_origins") || need(st->object_root_pos_w, "object_root_pos_w")) return 1;
                break;
            case IMX_T_OBJECT_AWAY_FROM_ROBOT: if (need(st->root_pos_w, "root_pos_w") || need(st->object_root_pos_w, "object_root_pos_w")) return 1; break;
            case IMX_T_JOINT_VEL_LIMIT: if (need(st->joint_vel, "joint_vel") || need(st->soft_joint_vel_limits, "soft_joint_vel_limits")) return 1; break;
            case IMX_T_JOINT_VEL_MANUAL_LIMIT: if (need(st->joint_vel, "joint_vel")) return 1; break;
            case IMX_T_JOINT_EFFORT_LIMIT: if (need(st->computed_torque, "computed_torque") || need(st->applied_torque, "applied_torque")) return 1; break;
            case IMX_T_EXTERNAL: if (need(st->ext_term, "ext_term")) return 1; break;
            case IMX_T_COMMAND_RESAMPLE: if (need(st->command_time_left, "command_time_left") || need(st->command_counter, "command_counter")) return 1; break;
            default: break;
        }
    }
    for (int k = 0; k < plan->nrew; ++k) {
        // (zero-weight terms too: imx_plan_update / set_term_cfg can wake one in place while a captured graph keeps replaying this
        //  launch with the state pointers it was captured with -- a NULL tensor would then be a device fault, not an error return)
        switch (w[plan->rew_off + k * IMX_REC_WORDS + IMX_R_OP]) {
            case IMX_W_BASE_HEIGHT_L2: if (need(st->root_pos_w, "root_pos_w")) return 1; break;
            case IMX_W_JOINT_TORQUES_L2: if (need(st->applied_torque, "applied_torque")) return 1; break;
            case IMX_W_JOINT_VEL_L1: case IMX_W_JOINT_VEL_L2: if (need(st->joint_vel, "joint_vel")) return 1; break;
            case IMX_W_JOINT_ACC_L2: if (need(st->joint_acc, "joint_acc")) return 1; break;
            case IMX_W_JOINT_DEVIATION_L1: if (need(st->joint_pos, "joint_pos") || need(st->default_joint_pos, "default_joint_pos")) return 1; break;
            case IMX_W_JOINT_POS_LIMITS: if (need(st->joint_pos, "joint_pos") || need(st->soft_joint_pos_limits, "soft_joint_pos_limits")) return 1; break;
            case IMX_W_JOINT_VEL_LIMITS: if (need(st->joint_vel, "joint_vel") || need(st->soft_joint_vel_limits, "soft_joint_vel_limits")) return 1; break;
            case IMX_W_APPLIED_TORQUE_LIMITS: if (need(st->applied_torque, "applied_torque") || need(st->computed_torque, "computed_torque")) return 1; break;
            case IMX_W_UNDESIRED_CONTACTS: case IMX_W_CONTACT_FORCES: if (need(st->net_forces_w_history, "net_forces_w_history")) return 1; break;
            case IMX_W_TRACK_LIN_VEL_XY_EXP: case IMX_W_TRACK_ANG_VEL_Z_EXP: case IMX_W_TRACK_LIN_VEL_XY_YAW_FRAME_EXP:
            case IMX_W_TRACK_ANG_VEL_Z_WORLD_EXP: if (need(st->command, "command")) return 1; break;
            case IMX_W_FEET_AIR_TIME: if (need(st->command, "command") || need(st->current_contact_time, "current_contact_time") || need(st->last_air_time, "last_air_time")) return 1; break;
            case IMX_W_FEET_AIR_TIME_POSITIVE_BIPED: if (need(st->command, "command") || need(st->current_contact_time, "current_contact_time") || need(st->current_air_time, "current_air_time")) return 1; break;
            case IMX_W_FEET_SLIDE: if (need(st->net_forces_w_history, "net_forces_w_history") || need(st->body_lin_vel_w, "body_lin_vel_w")) return 1; break;
            case IMX_W_JOINT_POS_TARGET_L2: if (need(st->joint_pos, "joint_pos")) return 1; break;
            case IMX_W_EXTERNAL: if (need(st->ext_reward, "ext_reward")) return 1; break;
            case IMX_W_BODY_LIN_ACC_L2: if (need(st->body_lin_acc_w, "body_lin_acc_w")) return 1; break;
            case IMX_W_AIR_TIME_REWARD: case IMX_W_GAIT_REWARD:
                if (need(st->command, "command") || need(st->current_air_time, "current_air_time") ||
                    need(st->current_contact_time, "current_contact_time")) return 1;
                break;
            case IMX_W_BASE_ANGULAR_VELOCITY_REWARD: case IMX_W_BASE_LINEAR_VELOCITY_REWARD: if (need(st->command, "command")) return 1; break;
            case IMX_W_FOOT_CLEARANCE_REWARD: if (need(st->body_pos_w, "body_pos_w") || need(st->body_lin_vel_w, "body_lin_vel_w")) return 1; break;
            case IMX_W_AIR_TIME_VARIANCE_PENALTY: if (need(st->last_air_time, "last_air_time") || need(st->last_contact_time, "last_contact_time")) return 1; break;
            case IMX_W_FOOT_SLIP_PENALTY: if (need(st->net_forces_w_history, "net_forces_w_history") || need(st->body_lin_vel_w, "body_lin_vel_w")) return 1; break;
            case IMX_W_JOINT_ACCELERATION_PENALTY: if (need(st->joint_acc, "joint_acc")) return 1; break;
            case IMX_W_JOINT_POSITION_PENALTY:
                if (need(st->command, "command") || need(st->joint_pos, "joint_pos") || need(st->default_joint_pos, "default_joint_pos")) return 1;
                break;
            case IMX_W_JOINT_TORQUES_PENALTY: if (need(st->applied_torque, "applied_torque")) return 1; break;
            case IMX_W_JOINT_VELOCITY_PENALTY: if (need(st->joint_vel, "joint_vel")) return 1; break;
            case IMX_W_MOVE_TO_TARGET_BONUS: case IMX_W_PROGRESS_REWARD: if (need(st->root_pos_w, "root_pos_w")) return 1; break;
            case IMX_W_JOINT_POS_LIMITS_PENALTY_RATIO: if (need(st->joint_pos, "joint_pos") || need(st->soft_joint_pos_limits, "soft_joint_pos_limits")) return 1; break;
            case IMX_W_POWER_CONSUMPTION: if (need(st->joint_vel, "joint_vel")) return 1; break;
            case IMX_W_POSITION_COMMAND_ERROR: case IMX_W_POSITION_COMMAND_ERROR_TANH:
                if (need(st->command, "command") || need(st->root_pos_w, "root_pos_w") || need(st->body_pos_w, "body_pos_w")) return 1;
                break;
            case IMX_W_ORIENTATION_COMMAND_ERROR: if (need(st->command, "command") || need(st->body_quat_w, "body_quat_w")) return 1; break;
            case IMX_W_OBJECT_IS_LIFTED: if (need(st->object_root_pos_w, "object_root_pos_w")) return 1; break;
            case IMX_W_OBJECT_EE_DISTANCE:
                if (need(st->object_root_pos_w, "object_root_pos_w") || need(st->body_pos_w, "body_pos_w") || need(st->body_quat_w, "body_quat_w")) return 1;
                break;
            case IMX_W_OBJECT_GOAL_DISTANCE:
                if (need(st->command, "command") || need(st->root_pos_w, "root_pos_w") || need(st->object_root_pos_w, "object_root_pos_w")) return 1;
                break;
            case IMX_W_NAV_POSITION_COMMAND_ERROR_TANH: case IMX_W_NAV_HEADING_COMMAND_ERROR_ABS: if (need(st->command, "command")) return 1; break;
            case IMX_W_TRACK_ORIENTATION_INV_L2: case IMX_W_SUCCESS_BONUS:
                if (need(st->command, "command") || need(plan->object_state.object_root_quat_w, "object_root_quat_w")) return 1;
                break;
            case IMX_W_TRACK_POS_L2:
                if (need(st->command, "command") || need(st->env_origins, "env_origins") || need(st->object_root_pos_w, "object_root_pos_w")) return 1;
                break;
            default: break;
        }
        // manipulation/cabinet: the frames the kernel computes once per env (tcp, handle; the fingertips for the ops that read them),
        // the gripper joints, the drawer joint
        const int cop = w[plan->rew_off + k * IMX_REC_WORDS + IMX_R_OP];
        if (cop >= IMX_W_APPROACH_EE_HANDLE) {
            if (need_frame_inputs(plan, st, 1, "a term") || need_frame_inputs(plan, st, 2 + plan->ft_n_ee, "a term")) return 1;
            if (cop == IMX_W_ALIGN_GRASP_AROUND_HANDLE || cop == IMX_W_APPROACH_GRIPPER_HANDLE || cop >= IMX_W_OPEN_DRAWER_BONUS)
                if (need_frame_inputs(plan, st, 2, "a term") || need_frame_inputs(plan, st, 3, "a term")) return 1;
            if (cop == IMX_W_GRASP_HANDLE && need(st->joint_pos, "joint_pos")) return 1;
            if (cop >= IMX_W_OPEN_DRAWER_BONUS) {
                if (w[plan->rew_off + k * IMX_REC_WORDS + IMX_R_AUX1] ? need(plan->articulation_state.joint_pos, "articulation_state.joint_pos")
                                                                      : need(st->joint_pos, "joint_pos")) return 1;
            }
        }
    }
    if (plan->CMD > 0 && !st->command) IMX_FAIL("command tensor missing");
    IMX_REQUIRE(plan->term_slots == 0 || bf->term_state,
                "imx_terminations_rewards: the plan has %d stateful reward terms (progress_reward): term_state (%d, N) is required",
                plan->term_slots, plan->term_slots);
    IMX_REQUIRE(!plan->scan_stateful || !st->root_pos_w || bf->scan_state,
                "imx_terminations_rewards: the height scanner has an update period / drift range: scan_state (N,8) is required");
    const int G = step_group_size(N);
    const unsigned grid = (unsigned)((N + G - 1) / G);
    StepScratch sc = carve(bf->scratch, N, plan->nrew_all > 0 ? plan->nrew_all : 1, plan->nterm > 0 ? plan->nterm : 1);
    // one wave per work item (termination or reward term) up to 16 waves; more items go round-robin
    const int items = plan->nterm + plan->nrew;
    const int NW = items < 2 ? 2 : (items > IMX_TR_MAX_WAVES ? IMX_TR_MAX_WAVES : items);
    size_t lds = ((size_t)(plan->nterm > 0 ? plan->nterm : 1) * 64 + 3 * (size_t)(plan->nrew > 0 ? plan->nrew : 1) * 64) * 4;
    // with the root position at hand the kernel also leaves the frame table imx_observations needs (flag 4 there skips k_frame)
    float* frame = st->root_pos_w ? reinterpret_cast<float*>(reinterpret_cast<char*>(bf->scratch) + frame_offset_bytes(plan, N)) : nullptr;
    bool classic = false, reach = false, lift = false, nav = false, inhand = false, need_dtheta = false, object_height = false;
    bool cabinet = false, fingers = false;
    for (int k = 0; k < plan->nrew; ++k) {
        const int op = w[plan->rew_off + k * IMX_REC_WORDS + IMX_R_OP];
        cabinet = cabinet || op >= IMX_W_APPROACH_EE_HANDLE;
        fingers = fingers || op == IMX_W_ALIGN_GRASP_AROUND_HANDLE || op == IMX_W_APPROACH_GRIPPER_HANDLE || op >= IMX_W_OPEN_DRAWER_BONUS;
        classic = classic || (op >= IMX_W_UPRIGHT_POSTURE_BONUS && op <= IMX_W_POWER_CONSUMPTION);
        reach = reach || (op >= IMX_W_POSITION_COMMAND_ERROR && op <= IMX_W_OBJECT_GOAL_DISTANCE);
        lift = lift || (op >= IMX_W_OBJECT_IS_LIFTED && op <= IMX_W_OBJECT_GOAL_DISTANCE);
        nav = nav || (op >= IMX_W_NAV_POSITION_COMMAND_ERROR_TANH && op <= IMX_W_NAV_HEADING_COMMAND_ERROR_ABS);
        inhand = inhand || (op >= IMX_W_TRACK_ORIENTATION_INV_L2 && op <= IMX_W_TRACK_POS_L2);
        need_dtheta = need_dtheta || op == IMX_W_TRACK_ORIENTATION_INV_L2 || op == IMX_W_SUCCESS_BONUS;
    }
    for (int k = 0; k < plan->nterm; ++k) {  // the terminations on the object
        const int32_t* r = &w[plan->term_off + k * IMX_REC_WORDS];
        lift = lift || r[IMX_R_OP] == IMX_T_OBJECT_REACHED_GOAL;
        object_height = object_height || (r[IMX_R_OP] == IMX_T_ROOT_HEIGHT_BELOW_MIN && r[IMX_R_AUX0]);
        inhand = inhand || (r[IMX_R_OP] >= IMX_T_MAX_CONSECUTIVE_SUCCESS && r[IMX_R_OP] <= IMX_T_OBJECT_AWAY_FROM_ROBOT);
    }
    lift = lift || (object_height && !inhand);  // root_height_below_minimum on the object: the lift kernel, or the in-hand one beside its ops
    reach = reach || lift;
    IMX_REQUIRE(!(inhand && (classic || reach || nav)),
                "imx_terminations_rewards: a plan with in-hand (manipulation/inhand) ops beside classic/humanoid, reach, lift or navigation ops is not supported");
    IMX_REQUIRE(!(classic && reach), "imx_terminations_rewards: a plan with both classic/humanoid and manipulation/reach or lift ops is not supported");
    IMX_REQUIRE(!(nav && (classic || reach)), "imx_terminations_rewards: a plan with navigation reward ops beside classic/humanoid, reach or lift ops is not supported");
    IMX_REQUIRE(!(cabinet && (classic || reach || nav || inhand)),
                "imx_terminations_rewards: a plan with cabinet (manipulation/cabinet) ops beside classic/humanoid, reach, lift, navigation or in-hand ops is not supported");
    if (cabinet) {
        lds += 20 * 64 * 4;  // the env's frames
        hipLaunchKernelGGL(k_term_rew_cabinet, dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc, frame, G,
                           flags & 1, ro, plan->ft_off, fingers ? 1 : 0, plan->articulation_state);
    } else if (inhand) {
        lds += 64 * 4;  // the env's orientation error
        hipLaunchKernelGGL(k_term_rew_inhand, dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc, frame, G,
                           flags & 1, ro, need_dtheta ? 1 : 0, plan->object_state);
    } else if (nav)
        hipLaunchKernelGGL(k_term_rew_nav, dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc, frame, G,
                           flags & 1, ro);
    else if (lift)
        hipLaunchKernelGGL(k_term_rew_lift, dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc, frame, G,
                           flags & 1, ro);
    else if (classic)
        hipLaunchKernelGGL((k_term_rew<true, false>), dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc,
                           frame, G, flags & 1, ro);
    else if (reach)
        hipLaunchKernelGGL((k_term_rew<false, true>), dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc,
                           frame, G, flags & 1, ro);
    else
        hipLaunchKernelGGL((k_term_rew<false, false>), dim3(grid), dim3(64 * NW), lds, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf, sc,
                           frame, G, flags & 1, ro);
    IMX_HIP(hipGetLastError());
    return 0;
}

// RewardManager.reset(env_ids) of the stateful reward terms outside a step (env.reset()): progress_reward.reset (rewards.py:54-60), the
// reset branch of k_term_rew's phase 2 -- same device function, same inputs.  One lane per env, the reward records through the scalar cache.
__global__ void k_term_state_reset(PlanView P, int64_t N, imx_state_t S, imx_buffers_t Bf, const uint8_t* __restrict__ mask) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N || (mask && !mask[e])) return;
    for (int k = 0; k < P.nrew; ++k) {
        const int32_t* r = P.w + P.rew_off + k * IMX_REC_WORDS;
        if (r[IMX_R_OP] != IMX_W_PROGRESS_REWARD) continue;
        Bf.term_state[(size_t)r[IMX_R_AUX0] * N + e] = progress_potential(f_of(r[IMX_R_P0]), f_of(r[IMX_R_P1]), f_of(r[IMX_R_P2]), S.root_pos_w[e * 3],
                                                                          S.root_pos_w[e * 3 + 1], S.root_pos_w[e * 3 + 2], P.step_dt, true);
    }
}

extern "C" int imx_term_state_reset(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf, const uint8_t* mask_d,
                                    imx_stream_t stream) {
    IMX_REQUIRE(plan && st && bf && N > 0, "imx_term_state_reset: null argument");
    if (plan->term_slots == 0) return 0;
    IMX_REQUIRE(bf->term_state, "imx_term_state_reset: term_state (%d, N) is required", plan->term_slots);
    IMX_REQUIRE(st->root_pos_w, "imx_term_state_reset: state tensor 'root_pos_w' is required by progress_reward but missing");
    hipLaunchKernelGGL(k_term_state_reset, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, imx_plan_view(plan), N, *st, *bf,
                       mask_d);
    IMX_HIP(hipGetLastError());
    return 0;
}

// Which observation kernel a plan gets (imx_observations below; imx_observations_kernel_name reports it to benchmarks).
struct ObsKernelChoice {
    bool lean;         // one group, no modifier programs, no history windows, no gaussian noise (DC == D also rules out twin scan columns)
    bool vertical;     // height-scanner frame yaw-only + vertical direction (the reference cfg): register-lean single-cell ray path
    bool single_wave;  // k_obs_lean: one single-wave workgroup per 64 rays + one for the env's other columns
    bool inhand;       // k_obs_inhand: a root observation on the rigid object (asset word 1) or goal_quat_diff
    bool cabinet;      // k_obs_cabinet: a FrameTransformer frame observation or a joint observation on the second articulation
    bool imu;          // k_obs_imu: an observation of an Imu sensor's data
    int scan_rec;
};
static ObsKernelChoice choose_obs_kernel(const imx_plan_t* plan) {
    const auto& w = plan->host;
    const PlanView pv = imx_plan_view(plan);
    ObsKernelChoice c;
    c.lean = plan->ngroups == 1 && plan->MS == 0 && plan->DC == plan->D && plan->DX == plan->DC;
    for (int k = 0; k < plan->nobs && c.lean; ++k) c.lean = !(w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_FLAGS] & (IMX_F_MODIFIERS | IMX_F_NOISE_GAUSS));
    c.vertical = pv.R == 0 || (pv.ray_yaw_only && pv.rdx == 0.0f && pv.rdy == 0.0f && pv.rdz != 0.0f);
    c.scan_rec = -1;
    c.inhand = false;
    c.cabinet = false;
    c.imu = false;
    bool object_op = false;  // (k_obs_lean is compiled without it)
    for (int k = 0; k < plan->nobs; ++k) {
        if (w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_OP] == IMX_O_HEIGHT_SCAN) c.scan_rec = k;
        const int op = w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_OP];
        object_op = object_op || op == IMX_O_OBJECT_POSITION_IN_ROBOT_ROOT_FRAME;
        c.inhand = c.inhand || op == IMX_O_GOAL_QUAT_DIFF ||
                   (op >= IMX_O_ROOT_POS_W && op <= IMX_O_ROOT_ANG_VEL_W && w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_AUX0]);
        c.cabinet = c.cabinet || (op >= IMX_O_REL_EE_DRAWER_DISTANCE && op <= IMX_O_ARTICULATION_JOINT_VEL_REL);
        c.imu = c.imu || (op >= IMX_O_IMU_ORIENTATION && op <= IMX_O_IMU_LIN_ACC);
    }
    c.single_wave = c.lean && c.scan_rec >= 0 && pv.R > 0 && pv.R <= 64 * 15 && !object_op && !c.inhand && !c.cabinet && !c.imu;
    return c;
}

extern "C" const char* imx_observations_kernel_name(const imx_plan_t* plan) {
    if (!plan) return "";
    const ObsKernelChoice c = choose_obs_kernel(plan);
    if (c.single_wave) return c.vertical ? "k_obs_lean<false>" : "k_obs_lean<true>";
    if (c.cabinet) return c.lean ? "k_obs_cabinet<true>" : "k_obs_cabinet<false>";
    if (c.imu) return c.lean ? "k_obs_imu<true>" : "k_obs_imu<false>";
    if (c.inhand) return c.lean ? "k_obs_inhand<true>" : "k_obs_inhand<false>";
    if (c.vertical) return c.lean ? "k_obs<false,true>" : "k_obs<false,false>";
    return c.lean ? "k_obs<true,true>" : "k_obs<true,false>";
}

extern "C" int imx_observations(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                                const imx_mesh_t* mesh, const float* noise_u_d, uint64_t seed, int enable_corruption,
                                float* ray_hits_out_d, imx_stream_t stream) {
    if (check_common(plan, N, st, bf)) return 1;
    IMX_REQUIRE(bf->obs && bf->counters, "imx_observations: null obs/counters buffer");
    IMX_REQUIRE(st->root_quat_w && st->root_lin_vel_w && st->root_ang_vel_w && st->root_pos_w, "root state missing");
    IMX_REQUIRE(!plan->needs_mesh || mesh, "plan has a height_scan term but no mesh was given");
    IMX_REQUIRE(plan->DC == plan->D || bf->reset_buf, "imx_observations: observation history needs the reset mask (reset_buf)");
    {
        const float* extra[3] = {bf->obs_extra1, bf->obs_extra2, bf->obs_extra3};
        for (int g = 1; g < plan->ngroups; ++g)
            IMX_REQUIRE(extra[g - 1], "imx_observations: the plan has %d observation groups but obs_extra%d is NULL", plan->ngroups, g);
    }
    IMX_REQUIRE(!plan->scan_stateful || (bf->scan_state && bf->scan_hit_z && bf->reset_buf),
                "imx_observations: the height scanner has an update period / drift range: scan_state (N,8), scan_hit_z (N,R) and reset_buf are required");
    IMX_REQUIRE(plan->MS == 0 || (bf->mod_state && bf->reset_buf),
                "imx_observations: the plan has stateful observation modifiers: mod_state (N x %d floats) and reset_buf are required", plan->MS);
    const auto& w = plan->host;
    for (int k = 0; k < plan->nobs; ++k) {
        const int op = w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_OP];
        const void* p = (const void*)1;
        const char* name = "";
        const bool on_object = w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_AUX0] != 0;  // (read for the four root ops only)
        switch (op) {
            case IMX_O_ROOT_POS_W:
                p = st->env_origins; name = "env_origins";
                if (p && on_object) { p = st->object_root_pos_w; name = "object_root_pos_w"; }
                break;
            case IMX_O_ROOT_QUAT_W: if (on_object) { p = plan->object_state.object_root_quat_w; name = "object_root_quat_w"; } break;
            case IMX_O_ROOT_LIN_VEL_W: if (on_object) { p = plan->object_state.object_root_lin_vel_w; name = "object_root_lin_vel_w"; } break;
            case IMX_O_ROOT_ANG_VEL_W: if (on_object) { p = plan->object_state.object_root_ang_vel_w; name = "object_root_ang_vel_w"; } break;
            case IMX_O_GOAL_QUAT_DIFF:
                p = plan->object_state.object_root_quat_w; name = "object_root_quat_w";
                if (p && !st->command) { p = nullptr; name = "command"; }
                break;
            case IMX_O_JOINT_POS: p = st->joint_pos; name = "joint_pos"; break;
            case IMX_O_JOINT_POS_REL: p = (st->joint_pos && st->default_joint_pos) ? (const void*)1 : nullptr; name = "joint_pos/default_joint_pos"; break;
            case IMX_O_JOINT_POS_LIMIT_NORMALIZED: p = (st->joint_pos && st->soft_joint_pos_limits) ? (const void*)1 : nullptr; name = "joint_pos/soft_joint_pos_limits"; break;
            case IMX_O_JOINT_VEL: p = st->joint_vel; name = "joint_vel"; break;
            case IMX_O_JOINT_VEL_REL: p = (st->joint_vel && st->default_joint_vel) ? (const void*)1 : nullptr; name = "joint_vel/default_joint_vel"; break;
            case IMX_O_LAST_ACTION: p = bf->action; name = "action"; break;
            case IMX_O_GENERATED_COMMANDS: p = st->command; name = "command"; break;
            case IMX_O_EXTERNAL: p = st->ext_obs; name = "ext_obs"; break;
            case IMX_O_BODY_INCOMING_WRENCH: p = st->link_incoming_joint_force; name = "link_incoming_joint_force"; break;
            case IMX_O_BASE_HEADING_PROJ: case IMX_O_BASE_ANGLE_TO_TARGET: p = st->root_pos_w; name = "root_pos_w"; break;
            case IMX_O_OBJECT_POSITION_IN_ROBOT_ROOT_FRAME:  // (and the frame row's root position, filled from root_pos_w)
                p = st->object_root_pos_w; name = "object_root_pos_w";
                if (p && !st->root_pos_w) { p = nullptr; name = "root_pos_w"; }
                break;
            case IMX_O_ARTICULATION_JOINT_POS_REL: p = plan->articulation_state.joint_pos; name = "articulation_state.joint_pos"; break;
            case IMX_O_ARTICULATION_JOINT_VEL_REL: p = plan->articulation_state.joint_vel; name = "articulation_state.joint_vel"; break;
            case IMX_O_EE_POS: case IMX_O_FINGERTIPS_POS: p = st->env_origins; name = "env_origins"; break;
            case IMX_O_IMU_ORIENTATION: case IMX_O_IMU_ANG_VEL: case IMX_O_IMU_LIN_ACC: {  // (AUX0 < IMX_MAX_IMU: parse_plan)
                const int si = w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_AUX0];
                p = si < plan->n_imu ? (const void*)1 : nullptr; name = "imu data (imx_plan_bind_imu)";
                break;
            }
            default: break;
        }
        IMX_REQUIRE(p, "state tensor '%s' is required by an observation term but missing", name);
        if (op >= IMX_O_REL_EE_DRAWER_DISTANCE && op <= IMX_O_FINGERTIPS_POS) {  // the frames the term reads (frame table indices)
            const int first = op == IMX_O_FINGERTIPS_POS ? 2 : 1, last = op == IMX_O_FINGERTIPS_POS ? plan->ft_n_ee : 1;
            for (int f = first; f <= last; ++f)
                if (need_frame_inputs(plan, st, f, "an observation term")) return 1;
            if (op == IMX_O_REL_EE_DRAWER_DISTANCE && need_frame_inputs(plan, st, 2 + plan->ft_n_ee, "an observation term")) return 1;
        }
    }
    MeshView mv{};
    if (mesh) mv = mesh->v;
    // one block per env; lanes take column i, i + blockDim, ...  Ray columns come first and are the long ones: when they
    // fit in three waves the remaining (cheap) columns ride as a second trip of the first lanes instead of a fourth wave
    int bs = plan->DC <= 64 ? 64 : (plan->DC <= 128 ? 128 : (plan->DC <= 192 ? 192 : 256));
    if (plan->DC > 192 && plan->n_ray_cols > 0 && plan->n_ray_cols <= 192 && plan->DC <= 2 * 192) bs = 192;
    const PlanView pv = imx_plan_view(plan);
    IMX_REQUIRE(bf->scratch, "imx_observations: scratch buffer missing");
    float* frame = reinterpret_cast<float*>(reinterpret_cast<char*>(bf->scratch) + frame_offset_bytes(plan, N));
    if (!(enable_corruption & 4))  // bit 2: imx_terminations_rewards ran on this very state and left the frame table behind
        hipLaunchKernelGGL(k_frame, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pv, N, *st, *bf, frame, (enable_corruption >> 1) & 1);
    const ObsKernelChoice ch = choose_obs_kernel(plan);
    const bool vertical = ch.vertical;
    // bit 4: finish the step tail imx_terminations_rewards (flags bit 0) left to this call -- one extra workgroup
    const bool tail = (enable_corruption & 16) != 0;
    StepScratch sc{};
    int tail_G = 0, tail_parts = 0;
    if (tail) {
        IMX_REQUIRE(bf->reset_env_ids && bf->log_out, "imx_observations: finishing the step tail needs reset_env_ids and log_out");
        sc = carve(bf->scratch, N, plan->nrew_all > 0 ? plan->nrew_all : 1, plan->nterm > 0 ? plan->nterm : 1);
        tail_G = step_group_size(N);
    }
    const size_t lds = (size_t)(pv.R > 0 ? pv.R : 1) * 4;
    const int nlog = plan->nrew_all + plan->nterm;
    const bool lean = ch.lean;
#define IMX_LAUNCH_OBS(G, L)                                                                                                     \
    hipLaunchKernelGGL((k_obs<G, L>), dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed, \
                       enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts)
    const int scan_rec = ch.scan_rec;
    if (ch.single_wave) {
        // one single-wave workgroup per 64 rays + one for the env's other columns
        const int wpe = (pv.R + 63) / 64 + 1;
        IMX_REQUIRE((uint64_t)N * wpe + 1 < (1ull << 31), "imx_observations: %lld envs x %d waves exceed the grid", (long long)N, wpe);
        if (tail) tail_parts = 1 + (nlog < 16 ? nlog : 16);  // one wave orders the reset ids, one per log entry (<= 16)
        // Up to ~2 residency rounds the waves go out role by role (all envs' first 64 rays, ..., the short column waves last: a
        // shorter drain, 17.2 us against 18.6 at 4096 envs); beyond that env by env (an env's rays share mesh lines: 173 us against
        // 191 at 65536 envs).
        const bool role_major = N <= 8192 && N >= 2;
        const uint32_t divisor = role_major ? (uint32_t)N : (uint32_t)wpe;
        uint32_t div_magic = 0;
        int div_shift = 0;
        imx_magic_u31(divisor, div_magic, div_shift);
        const unsigned lgrid = (unsigned)(N * wpe) + (unsigned)tail_parts;
        if (vertical)
            hipLaunchKernelGGL(k_obs_lean<false>, dim3(lgrid), dim3(64), 0, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                               enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, scan_rec, role_major ? -wpe : wpe, div_magic, div_shift, pv.w);
        else
            hipLaunchKernelGGL(k_obs_lean<true>, dim3(lgrid), dim3(64), 0, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                               enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, scan_rec, role_major ? -wpe : wpe, div_magic, div_shift, pv.w);
    } else {
        if (tail) tail_parts = 1 + ((nlog < 16 ? nlog : 16) * 64 + bs - 1) / bs;
        const unsigned grid = (unsigned)N + (unsigned)tail_parts;
        IMX_REQUIRE(!(ch.cabinet && ch.inhand), "imx_observations: a plan with cabinet (manipulation/cabinet) observations beside observations on the "
                                                "scene's rigid object (manipulation/inhand) is not supported");
        IMX_REQUIRE(!(ch.imu && (ch.cabinet || ch.inhand)), "imx_observations: a plan with Imu observations beside cabinet or rigid-object "
                                                            "observations is not supported");
        if (ch.imu) {
            if (lean)
                hipLaunchKernelGGL(k_obs_imu<true>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->imu);
            else
                hipLaunchKernelGGL(k_obs_imu<false>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->imu);
        } else if (ch.cabinet) {
            if (lean)
                hipLaunchKernelGGL(k_obs_cabinet<true>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->articulation_state);
            else
                hipLaunchKernelGGL(k_obs_cabinet<false>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->articulation_state);
        } else if (ch.inhand) {
            if (lean)
                hipLaunchKernelGGL(k_obs_inhand<true>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->object_state);
            else
                hipLaunchKernelGGL(k_obs_inhand<false>, dim3(grid), dim3(bs), lds, (hipStream_t)stream, pv, N, *st, *bf, mv, frame, noise_u_d, seed,
                                   enable_corruption, ray_hits_out_d, sc, tail_G, tail_parts, plan->object_state);
        } else if (vertical) { if (lean) IMX_LAUNCH_OBS(false, true); else IMX_LAUNCH_OBS(false, false); }
        else { if (lean) IMX_LAUNCH_OBS(true, true); else IMX_LAUNCH_OBS(true, false); }
    }
#undef IMX_LAUNCH_OBS
    IMX_HIP(hipGetLastError());
    return 0;
}

extern "C" int imx_root_frame(int64_t N, const float* q, const float* lv, const float* av, float gx, float gy, float gz,
                              float* olv, float* oav, float* opg, imx_stream_t stream) {
    IMX_REQUIRE(N > 0 && q, "imx_root_frame: bad arguments");
    IMX_REQUIRE((!olv || lv) && (!oav || av), "imx_root_frame: output requested without its input");
    hipLaunchKernelGGL(k_root_frame, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, q, lv, av,
                       gx, gy, gz, olv, oav, opg);
    IMX_HIP(hipGetLastError());
    return 0;
}

extern "C" int imx_raycast(const imx_mesh_t* mesh, const float* starts, const float* dirs, int64_t n, float max_dist,
                           float* hits, float* dist, int32_t* faces, imx_stream_t stream) {
    if (n == 0) return 0;
    IMX_REQUIRE(mesh && starts && dirs && hits, "imx_raycast: null argument");
    IMX_REQUIRE(n > 0, "imx_raycast: negative ray count");
    hipLaunchKernelGGL(k_raycast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mesh->v, starts,
                       dirs, n, max_dist, hits, dist, faces);
    IMX_HIP(hipGetLastError());
    return 0;
}
