// Device functions of the observation path shared by the observation kernels (step.hip) and the fused low-level policy step
// (pretrained_policy.hip): one column's value, its noise / clip / scale, and the per-column record they read.  Moved here from step.hip
// unchanged: every kernel that used them compiles to the instruction stream it had ("Low-level policy step").
#pragma once

#include "imx_internal.h"
#include "imx_frame_transformer.h"

// torch.clamp / Tensor.clip of an observation: NaN stays NaN (fminf / fmaxf alone return the bound).  A height-scan ray that misses
// (+inf hit) through a DigitalFilter gives -inf - -inf = NaN, and the reference's observation is NaN, not the clip bound.
IMX_DEV float clip_keep_nan(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

// one angle of euler_xyz_from_quat (utils/math.py:414-444) `% (2 pi)`: atan2 lies in [-pi, pi], where torch.remainder by fp32(2 pi) is
// x + 2 pi for x < 0 and x itself otherwise (-0 included)
IMX_DEV float euler_mod_2pi(float s, float c) {
    const float a = atan2f(s, c);
    return a < 0.0f ? a + 6.28318530717958647692f : a;
}
// atan2(sin(a), cos(a)) of observations.py:26-28,75 for a in (-3 pi, 2 pi): a wrapped into (-pi, pi] without sinf / cosf (exact math;
// within a few ulps of pi the reference's rounding can land on the other side -- a known deviation, compared modulo 2 pi)
IMX_DEV float wrap_atan2(float a) {
    const float PI = 3.14159265358979323846f, TWO_PI = 6.28318530717958647692f;
    return a > PI ? a - TWO_PI : (a <= -PI ? a + TWO_PI : a);
}
// base_heading_proj (observations.py:43-58): quat_rotate(q, FORWARD_VEC_B = (1, 0, 0)) (utils/math.py:583-602, a + b + c; with v = x the
// cross and dot products reduce to single factors exactly) . normalize(target - pos, z = 0) (math.py:82-92: x / max(||x||, 1e-9))
IMX_DEV float heading_proj(float qw, float qx, float qy, float qz, float tx, float ty, float px, float py) {
    const float dx = tx - px, dy = ty - py;
    const float n = fmaxf(sqrtf(dx * dx + dy * dy), 1.0e-9f);
    const float ux = dx / n, uy = dy / n;
    const float hx = (2.0f * (qw * qw) - 1.0f) + (qx * qx) * 2.0f;
    const float hy = (qz * qw) * 2.0f + (qy * qx) * 2.0f;
    return hx * ux + hy * uy;  // + hz * 0
}
// base_angle_to_target (observations.py:61-77): atan2(to_target y, x) - yaw, wrapped
IMX_DEV float angle_to_target(float qw, float qx, float qy, float qz, float tx, float ty, float px, float py) {
    const float walk = atan2f(ty - py, tx - px);
    const float yaw = euler_mod_2pi(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
    return wrap_atan2(walk - yaw);
}

#define IMX_XCOL_WORDS 16
enum { XC_COL = 0, XC_OP, XC_J, XC_FLAGS, XC_P0, XC_NLO, XC_NHI, XC_CLO, XC_CHI, XC_SCALE, XC_AUX, XC_RX, XC_RY, XC_RZ, XC_HIST, XC_HSTRIDE };

struct XCol {
    int4 a, b, c, d;
};
IMX_DEV XCol load_xcol(const int32_t* __restrict__ W, int off, int i) {
    const int4* p = reinterpret_cast<const int4*>(W + off) + (size_t)i * 4;
    XCol x;
    x.a = p[0]; x.b = p[1]; x.c = p[2]; x.d = p[3];
    return x;
}

// The noise term of one element: uniform_noise u * (n_max - n_min) + n_min (noise_model.py:62-66; constant_noise is the case n_min == n_max)
// or gaussian_noise mean + std * z (:87-92).  The sample is the fed one (the reference's recorded rand_like / randn_like draw) or comes
// from the counter-based generator (Box-Muller on two of its uniforms for z).
// GAUSS = false: plans without a gaussian term (the LEAN kernels: logf / cosf / sqrtf in their instruction stream cost 2 % at 4096 envs
// and 7 % at 65 536, taken or not; a plan with gaussian noise runs the general kernels).
template <bool GAUSS>
IMX_DEV float noise_sample(int flags, float lo, float hi, const float* __restrict__ noise_u, uint64_t seed, uint32_t step, int64_t e, int D, int c) {
    if (GAUSS && (flags & IMX_F_NOISE_GAUSS)) {
        float z;
        if (noise_u) {
            z = noise_u[e * D + c];
        } else {
            const float u1 = uniform01(seed, step, (uint64_t)e * D + c), u2 = uniform01(seed ^ 0x6A09E667F3BCC909ull, step, (uint64_t)e * D + c);
            z = sqrtf(-2.0f * logf(1.0f - u1)) * cosf(6.28318530717958647692f * u2);  // 1 - u1 in (0, 1]: no log(0)
        }
        return lo + hi * z;
    }
    const float u = noise_u ? noise_u[e * D + c] : uniform01(seed, step, (uint64_t)e * D + c);
    return u * (hi - lo) + lo;
}

// D = width of the whole column space (all groups side by side), gbase = first column of this entry's group in it: the parity-mode
// uniforms are one (N, D) array, group after group
template <bool GAUSS>
IMX_DEV float obs_post(const XCol& x, float v, int corrupt, const float* __restrict__ noise_u, uint64_t seed, uint32_t step,
                       int64_t e, int D, int gbase) {
    const int flags = x.a.w;
    if (corrupt && (flags & (IMX_F_NOISE_ADD | IMX_F_NOISE_SCALE | IMX_F_NOISE_ABS))) {
        // a term with a history window draws for its first (oldest-slot) columns, like rand_like on the (N, d) term value
        const int c = gbase + x.a.x - (x.d.z - 1) * x.d.w;
        const float lo = f_of(x.b.y), hi = f_of(x.b.z);
        const float nz = noise_sample<GAUSS>(flags, lo, hi, noise_u, seed, step, e, D, c);
        v = (flags & IMX_F_NOISE_ADD) ? v + nz : ((flags & IMX_F_NOISE_SCALE) ? v * nz : nz);
    }
    if (flags & IMX_F_CLIP) v = clip_keep_nan(v, f_of(x.b.w), f_of(x.c.x));
    if (flags & IMX_F_SCALE) v = v * f_of(x.c.y);
    return v;
}

// object_position_in_robot_root_frame (manipulation/lift/mdp/observations.py:19-31), component j: subtract_frame_transforms (utils/math.py:
// 785-816) = quat_apply(quat_inv(q), object - root), the subtraction inside the rotation; quat_inv = normalize(conjugate(q)) (:239-248,
// normalize :82-92 = x / max(||x||, 1e-9)).  es = the env's frame row: root position 9..11, root quaternion 12..15
IMX_DEV float object_pos_in_root_frame(const float* __restrict__ es, const float* __restrict__ obj, int j) {
    const float w = es[12], x = es[13], y = es[14], z = es[15];
    const float n = fmaxf(sqrtf(((w * w + x * x) + y * y) + z * z), 1.0e-9f);
    float ox, oy, oz;
    quat_apply(w / n, -x / n, -y / n, -z / n, obj[0] - es[9], obj[1] - es[10], obj[2] - es[11], ox, oy, oz);
    return j == 0 ? ox : (j == 1 ? oy : oz);
}

// goal_quat_diff (manipulation/inhand/mdp/observations.py:20-38), component j: quat_mul(object_quat_w, quat_conjugate(goal_quat_w)), then
// quat_unique (utils/math.py:251-263: -q where w < 0) when make_quat_unique
IMX_DEV float goal_quat_diff(const float* __restrict__ obj_quat, const float* __restrict__ cmd, bool unique, int j) {
    const float4 q = quat_mul_ref(make_float4(obj_quat[0], obj_quat[1], obj_quat[2], obj_quat[3]), make_float4(cmd[3], -cmd[4], -cmd[5], -cmd[6]));
    const float v = j == 0 ? q.x : (j == 1 ? q.y : (j == 2 ? q.z : q.w));
    return (unique && q.x < 0.0f) ? -v : v;
}

// value of one non-ray observation column (every op but HEIGHT_SCAN); es = the env's frame (k_frame).  OBJECT: with the op that reads the
// scene's rigid object -- k_obs only; k_obs_lean, tuned to its SGPR budget, is not chosen for a plan that has it (choose_obs_kernel)
template <bool OBJECT>
IMX_DEV float obs_plain_value(const PlanView& P, const imx_state_t& S, const imx_buffers_t& Bf, const float* __restrict__ es,
                              int64_t e, const XCol& x) {
    const int32_t* __restrict__ W = P.w;
    const int op = x.a.y, j = x.a.z, flags = x.a.w, aux = x.c.z, J = P.J;
    switch (op) {
        case IMX_O_BASE_POS_Z: return es[11];
        case IMX_O_BASE_LIN_VEL: return es[0 + j];
        case IMX_O_BASE_ANG_VEL: return es[3 + j];
        case IMX_O_PROJECTED_GRAVITY: return es[6 + j];
        case IMX_O_ROOT_POS_W: return es[9 + j] - S.env_origins[e * 3 + j];
        case IMX_O_ROOT_QUAT_W: return ((flags & IMX_F_QUAT_UNIQUE) && es[12] < 0.0f) ? -es[12 + j] : es[12 + j];
        case IMX_O_ROOT_LIN_VEL_W: return S.root_lin_vel_w[e * 3 + j];
        case IMX_O_ROOT_ANG_VEL_W: return S.root_ang_vel_w[e * 3 + j];
        case IMX_O_JOINT_POS: return S.joint_pos[e * J + aux];
        case IMX_O_JOINT_POS_REL: return S.joint_pos[e * J + aux] - S.default_joint_pos[e * J + aux];
        case IMX_O_JOINT_POS_LIMIT_NORMALIZED: {  // scale_transform (utils/math.py:22-40)
            const float2 lim = reinterpret_cast<const float2*>(S.soft_joint_pos_limits)[e * J + aux];
            const float offset = (lim.x + lim.y) * 0.5f;
            return 2.0f * (S.joint_pos[e * J + aux] - offset) / (lim.y - lim.x);
        }
        case IMX_O_JOINT_VEL: return S.joint_vel[e * J + aux];
        case IMX_O_JOINT_VEL_REL: return S.joint_vel[e * J + aux] - S.default_joint_vel[e * J + aux];
        case IMX_O_LAST_ACTION: return Bf.action[e * P.A + j];
        case IMX_O_GENERATED_COMMANDS: return S.command[e * P.CMD + j];
        case IMX_O_EXTERNAL: return S.ext_obs[e * (int64_t)W[IMX_H_NEXT_OBS] + aux + j];
        // classic/humanoid/mdp/observations.py; target_pos x, y in XC_P0, XC_RX
        case IMX_O_BASE_YAW_ROLL: {  // :19-30: yaw, roll
            const float qw = es[12], qx = es[13], qy = es[14], qz = es[15];
            return wrap_atan2(j == 0 ? euler_mod_2pi(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz))
                                     : euler_mod_2pi(2.0f * (qw * qx + qy * qz), 1.0f - 2.0f * (qx * qx + qy * qy)));
        }
        case IMX_O_BASE_UP_PROJ: return -es[8];  // :33-40
        case IMX_O_BASE_HEADING_PROJ: return heading_proj(es[12], es[13], es[14], es[15], f_of(x.b.x), f_of(x.c.w), es[9], es[10]);
        case IMX_O_BASE_ANGLE_TO_TARGET: return angle_to_target(es[12], es[13], es[14], es[15], f_of(x.b.x), f_of(x.c.w), es[9], es[10]);
        case IMX_O_BODY_INCOMING_WRENCH: return S.link_incoming_joint_force[e * (int64_t)P.NB * 6 + aux];  // envs/mdp/observations.py:176-185
        case IMX_O_OBJECT_POSITION_IN_ROBOT_ROOT_FRAME: return OBJECT ? object_pos_in_root_frame(es, S.object_root_pos_w + e * 3, j) : 0.0f;
        default: return 0.0f;
    }
}

// k_obs_inhand's column value: the root observations on the scene's rigid object (XC_AUX = 1; X = the bound imx_object_state_t) and
// goal_quat_diff; every other column is obs_plain_value's.  In a function of its own, so that every other kernel keeps the instruction
// stream it had
IMX_DEV float obs_inhand_value(const PlanView& P, const imx_state_t& S, const imx_object_state_t& X, const imx_buffers_t& Bf,
                               const float* __restrict__ es, int64_t e, const XCol& x) {
    const int op = x.a.y, j = x.a.z, flags = x.a.w, aux = x.c.z;
    if (op == IMX_O_GOAL_QUAT_DIFF) return goal_quat_diff(X.object_root_quat_w + e * 4, S.command + e * P.CMD, (flags & IMX_F_QUAT_UNIQUE) != 0, j);
    if (aux && op >= IMX_O_ROOT_POS_W && op <= IMX_O_ROOT_ANG_VEL_W) {
        if (op == IMX_O_ROOT_POS_W) return S.object_root_pos_w[e * 3 + j] - S.env_origins[e * 3 + j];
        if (op == IMX_O_ROOT_LIN_VEL_W) return X.object_root_lin_vel_w[e * 3 + j];
        if (op == IMX_O_ROOT_ANG_VEL_W) return X.object_root_ang_vel_w[e * 3 + j];
        const float* __restrict__ q = X.object_root_quat_w + e * 4;
        return ((flags & IMX_F_QUAT_UNIQUE) && q[0] < 0.0f) ? -q[j] : q[j];
    }
    return obs_plain_value<true>(P, S, Bf, es, e, x);
}

// k_obs_imu's column value: imu_orientation / imu_ang_vel / imu_lin_acc (envs/mdp/observations.py:188-231) = the sensor's data.quat_w /
// ang_vel_b / lin_acc_b as the refresh launch (imx_imu) left them, XC_AUX = the sensor's index; every other column is obs_plain_value's
IMX_DEV float obs_imu_value(const PlanView& P, const imx_state_t& S, const ImuObsView& X, const imx_buffers_t& Bf,
                            const float* __restrict__ es, int64_t e, const XCol& x) {
    const int op = x.a.y, j = x.a.z, aux = x.c.z;
    if (op == IMX_O_IMU_ORIENTATION) return X.quat_w[aux][e * 4 + j];
    if (op == IMX_O_IMU_ANG_VEL) return X.ang_vel_b[aux][e * 3 + j];
    if (op == IMX_O_IMU_LIN_ACC) return X.lin_acc_b[aux][e * 3 + j];
    return obs_plain_value<true>(P, S, Bf, es, e, x);
}

// ---- manipulation/cabinet (Isaac-Open-Drawer-Franka-v0): FrameTransformer frames out of the plan's frame table (include/imx.h IMX_FT_*)
// The pose of the frame whose words start at P.w + fo for env e: its body's pose -- of the robot (S) or of the second articulation
// (X, B2 bodies per env) by the frame's asset word -- combined with its offset (imx_frame_pose, imx_frame_transformer.h).
IMX_DEV ImxFramePose cabinet_frame_pose(const PlanView& P, const imx_state_t& S, const imx_articulation_state_t& X, int fo, int B2, int64_t e) {
    const int32_t* __restrict__ fr = P.w + fo;
    const bool second = fr[1] != 0;
    const int64_t b = e * (second ? B2 : P.NB) + fr[0];
    return imx_frame_pose((second ? X.body_pos_w : S.body_pos_w) + b * 3, (second ? X.body_quat_w : S.body_quat_w) + b * 4, fr);
}
// word offset of a frame inside the table at ft: the ee_frame's target t, the cabinet_frame's target t (n_ee = the ee_frame's target count)
IMX_DEV int ft_ee_target(int ft, int t) { return ft + IMX_FT_HEADER_WORDS + (1 + t) * IMX_FRAME_WORDS; }
IMX_DEV int ft_cabinet_target(int ft, int n_ee, int t) { return ft + IMX_FT_HEADER_WORDS + (2 + n_ee + t) * IMX_FRAME_WORDS; }

// k_obs_cabinet's column value: the four frame observations of manipulation/cabinet/mdp/observations.py (XC_AUX = the frame table) and
// joint_pos_rel / joint_vel_rel on the second articulation (XC_AUX = the joint, XC_RX = its default, XC_RY = the row width J2); every
// other column is obs_plain_value's.  One lane per column: a lane derives the frame it reads itself.
IMX_DEV float obs_cabinet_value(const PlanView& P, const imx_state_t& S, const imx_articulation_state_t& X, const imx_buffers_t& Bf,
                                const float* __restrict__ es, int64_t e, const XCol& x) {
    const int op = x.a.y, j = x.a.z, flags = x.a.w, aux = x.c.z;
    if (op >= IMX_O_ARTICULATION_JOINT_POS_REL)
        return (op == IMX_O_ARTICULATION_JOINT_POS_REL ? X.joint_pos : X.joint_vel)[e * x.d.x + aux] - f_of(x.c.w);
    if (op >= IMX_O_REL_EE_DRAWER_DISTANCE) {
        const int B2 = P.w[aux + 1], n_ee = P.w[aux + 2];
        const int t = op == IMX_O_FINGERTIPS_POS ? 1 + j / 3 : 0, c = op == IMX_O_FINGERTIPS_POS ? j % 3 : j;
        const ImxFramePose tp = cabinet_frame_pose(P, S, X, ft_ee_target(aux, t), B2, e);
        if (op == IMX_O_EE_QUAT) {  // ee_quat :51-59: quat_unique (utils/math.py:448-461: -q where w < 0) when make_quat_unique
            const float v = c == 0 ? tp.q.x : (c == 1 ? tp.q.y : (c == 2 ? tp.q.z : tp.q.w));
            return ((flags & IMX_F_QUAT_UNIQUE) && tp.q.x < 0.0f) ? -v : v;
        }
        const float pc = c == 0 ? tp.px : (c == 1 ? tp.py : tp.pz);
        if (op == IMX_O_REL_EE_DRAWER_DISTANCE) {  // :27-32: handle - tcp
            const ImxFramePose hd = cabinet_frame_pose(P, S, X, ft_cabinet_target(aux, n_ee, 0), B2, e);
            return (c == 0 ? hd.px : (c == 1 ? hd.py : hd.pz)) - pc;
        }
        return pc - S.env_origins[e * 3 + c];  // ee_pos :43-48, fingertips_pos :35-40
    }
    return obs_plain_value<true>(P, S, Bf, es, e, x);
}
