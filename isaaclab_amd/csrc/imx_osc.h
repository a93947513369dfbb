// OperationalSpaceControllerAction for ONE env (envs/mdp/actions/task_space_actions.py:416-462, 568-649 with
// controllers/operational_space.py:173-343, 345-548).  Shared by the kernel (osc.hip) and by the host program tools/osc_host.cpp: this
// file compiles as gfx950 device code and as plain host C++.
//
// Only the identity task frame is built (the term compiler refuses task_frame_rel_path): R_task_b is the identity, so the gains, the
// selection matrices and the wrench in the root frame are the task-frame ones, exactly; the desired rotation still passes through the
// reference's quat_mul with the identity (combine_frame_transforms), which rounds.
//
// No value can move an access: every index comes from the cfg (checked on the host, imx_osc_check) and the env index.  NaN inputs, a
// zero quaternion or a singular mass matrix give NaN / inf in the env's own outputs.
#pragma once
#include "../../include/imx.h"
#include "imx_task_space.h"

struct OscIO {
    const float* processed_action;  // (N, PA)
    int64_t PA;
    const float* root_pos;          // (N,3)
    const float* root_quat;         // (N,4)
    const float* root_lin_vel;      // (N,3)
    const float* root_ang_vel;      // (N,3)
    const float* body_pos;          // (N, num_bodies, 3)
    const float* body_quat;         // (N, num_bodies, 4)
    const float* body_lin_vel;      // (N, num_bodies, 3)
    const float* body_ang_vel;      // (N, num_bodies, 3)
    int64_t num_bodies;
    const float* jacobians;         // (N, NB, 6, ND)
    int64_t NB, ND;
    const float* mass;              // (N, NM, NM)
    const float* gravity;           // (N, NM)
    int64_t NM;
    const float* joint_pos;         // (N, J)
    const float* joint_vel;         // (N, J)
    int64_t J;
    const float* nullspace_target;  // (N, num_joints)
    float* command_state;           // (N, ld_cmd): pose 7, Kp 6, Kd 6, wrench 6
    int64_t ld_cmd;
    float* joint_efforts;           // (N, ld_eff)
    int64_t ld_eff;
};

#define IMX_OSC_NJ IMX_IK_MAX_JOINTS

// R^T R z = b for an upper-triangular 6 x 6 factor.  PARTIAL: R is block diagonal (two 3 x 3 blocks); the zero entries are skipped.
template <bool PARTIAL>
IMX_HD void osc_rtr_solve(const float (&R)[6][6], float (&b)[6]) {
IMX_UNROLL
    for (int i = 0; i < 6; ++i) {  // R^T y = b
        float s = b[i];
IMX_UNROLL
        for (int k = 0; k < i; ++k)
            if (!PARTIAL || (i < 3) == (k < 3)) s -= R[k][i] * b[k];
        b[i] = s / R[i][i];
    }
IMX_UNROLL
    for (int i = 5; i >= 0; --i) {  // R z = y
        float s = b[i];
IMX_UNROLL
        for (int k = i + 1; k < 6; ++k)
            if (!PARTIAL || (i < 3) == (k < 3)) s -= R[i][k] * b[k];
        b[i] = s / R[i][i];
    }
}

// DEC: imx_osc_decoupling of the cfg; NULLSP: cfg.nullspace_position (with DEC == full only).  Compile-time, so that an instantiation
// holds only the matrices its cfg needs.
template <int DEC, bool NULLSP>
IMX_HD void osc_env(const imx_osc_t& c, int64_t e, int mode, const OscIO& io) {
    // ---- _compute_ee_pose (task_space_actions.py:597-615).  task_frame, apply_delta_pose and frame_jacobian of imx_task_space.h are
    // written out in this function: through the helpers the same arithmetic is scheduled and allocated differently (225 / 180 / 169 /
    // 114 VGPRs against 233 / 173 / 174 / 116), and the shipped cfg's mode 2 replayed from a graph measured 0.02 to 0.05 us slower (NOTES.md)
    const float4 rq = make_float4(io.root_quat[e * 4], io.root_quat[e * 4 + 1], io.root_quat[e * 4 + 2], io.root_quat[e * 4 + 3]);
    const float4 q10 = quat_inv(rq);
    const int64_t b = e * io.num_bodies + c.body_idx;
    const float4 bq = make_float4(io.body_quat[b * 4], io.body_quat[b * 4 + 1], io.body_quat[b * 4 + 2], io.body_quat[b * 4 + 3]);
    // subtract_frame_transforms (utils/math.py:785-816)
    const float4 eq0 = quat_mul_ref(q10, bq);  // (without the offset: _ee_pose_b_no_offset)
    float4 eq = eq0;
    float ex, ey, ez;
    quat_apply(q10.x, q10.y, q10.z, q10.w, io.body_pos[b * 3] - io.root_pos[e * 3], io.body_pos[b * 3 + 1] - io.root_pos[e * 3 + 1],
               io.body_pos[b * 3 + 2] - io.root_pos[e * 3 + 2], ex, ey, ez);
    if (c.has_offset) {  // combine_frame_transforms (:750-781)
        float ox, oy, oz;
        quat_apply(eq.x, eq.y, eq.z, eq.w, c.offset_pos[0], c.offset_pos[1], c.offset_pos[2], ox, oy, oz);
        ex += ox; ey += oy; ez += oz;
        eq = quat_mul_ref(eq, make_float4(c.offset_rot[0], c.offset_rot[1], c.offset_rot[2], c.offset_rot[3]));
    }

    float px, py, pz;  // desired_ee_pose_b
    float4 qd;
    float kp[6], kd[6], fw[6];
    float* cs = io.command_state + e * io.ld_cmd;
    if (mode & 1) {  // ---- OperationalSpaceController.set_command (operational_space.py:173-343)
        const float* a = io.processed_action + e * io.PA;
IMX_UNROLL
        for (int i = 0; i < 6; ++i) {
            float k = c.motion_stiffness[i], ratio = c.motion_damping_ratio[i];
            if (c.impedance_mode != IMX_OSC_FIXED)  // stiffness.clip_(min, max) (:224-226, 242-244)
                k = fminf(fmaxf(a[c.stiffness_col + i], c.stiffness_limits[0]), c.stiffness_limits[1]);
            if (c.impedance_mode == IMX_OSC_VARIABLE)
                ratio = fminf(fmaxf(a[c.damping_ratio_col + i], c.damping_ratio_limits[0]), c.damping_ratio_limits[1]);
            kp[i] = c.motion_axes[i] * k;              // S_motion @ diag(stiffness) (:96, 230, 251)
            kd[i] = 2.0f * sqrtf(kp[i]) * ratio;       // (:97-101, 231-237, 252-254)
            fw[i] = c.has_wrench ? a[c.wrench_col + i] : 0.0f;  // R_task_b = I, task frame at the root's origin (:337-343)
        }
        const float* t = a + c.pose_col;
        const float4 ident = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        float4 qt;  // desired_ee_pose_task
        if (c.pose_type == IMX_OSC_POSE_REL) {
            // subtract_frame_transforms with the identity task frame (:271-276): quat_inv(identity) * q, the position as it is
            const float4 cur = quat_mul_ref(make_float4(1.0f, -0.0f, -0.0f, -0.0f), eq);
            // apply_delta_pose (utils/math.py:873-910)
            px = ex + t[0]; py = ey + t[1]; pz = ez + t[2];
            const float rx = t[3], ry = t[4], rz = t[5];
            const float angle = sqrtf((rx * rx + ry * ry) + rz * rz);
            const float axx = rx / angle, axy = ry / angle, axz = rz / angle;
            // quat_from_angle_axis (:629-642): normalize(axis) * sin(angle / 2), cos(angle / 2), normalize
            const float an = fmaxf(sqrtf((axx * axx + axy * axy) + axz * axz), 1.0e-9f);
            const float th = angle / 2.0f, sn = sinf(th), w = cosf(th);
            const float x = axx / an * sn, y = axy / an * sn, z = axz / an * sn;
            const float qn = fmaxf(sqrtf((w * w + x * x) + (y * y + z * z)), 1.0e-9f);
            const bool on = angle > 1.0e-6f;  // (NaN: identity, as torch.where picks)
            const float4 dq4 = make_float4(on ? w / qn : 1.0f, on ? x / qn : 0.0f, on ? y / qn : 0.0f, on ? z / qn : 0.0f);
            qt = quat_mul_ref(dq4, cur);
        } else {  // pose_abs: the seven values as they are (:282-284)
            px = t[0]; py = t[1]; pz = t[2];
            qt = make_float4(t[3], t[4], t[5], t[6]);
        }
        qd = quat_mul_ref(ident, qt);  // combine_frame_transforms with the identity task frame (:328-335)
        cs[0] = px; cs[1] = py; cs[2] = pz; cs[3] = qd.x; cs[4] = qd.y; cs[5] = qd.z; cs[6] = qd.w;
IMX_UNROLL
        for (int i = 0; i < 6; ++i) {
            cs[7 + i] = kp[i];
            cs[13 + i] = kd[i];
            cs[19 + i] = fw[i];
        }
    } else {
        px = cs[0]; py = cs[1]; pz = cs[2];
        qd = make_float4(cs[3], cs[4], cs[5], cs[6]);
IMX_UNROLL
        for (int i = 0; i < 6; ++i) {
            kp[i] = cs[7 + i];
            kd[i] = cs[13 + i];
            fw[i] = cs[19 + i];
        }
    }
    if (!(mode & 2)) return;

    // ---- apply_actions (:440-462)
    // _compute_ee_velocity (:617-634)
    float vel[6];
    {
        const float lx = io.body_lin_vel[b * 3] - io.root_lin_vel[e * 3], ly = io.body_lin_vel[b * 3 + 1] - io.root_lin_vel[e * 3 + 1],
                    lz = io.body_lin_vel[b * 3 + 2] - io.root_lin_vel[e * 3 + 2];
        const float wx = io.body_ang_vel[b * 3] - io.root_ang_vel[e * 3], wy = io.body_ang_vel[b * 3 + 1] - io.root_ang_vel[e * 3 + 1],
                    wz = io.body_ang_vel[b * 3 + 2] - io.root_ang_vel[e * 3 + 2];
        quat_rotate_ref(rq, -1.0f, lx, ly, lz, vel[0], vel[1], vel[2]);
        quat_rotate_ref(rq, -1.0f, wx, wy, wz, vel[3], vel[4], vel[5]);
        if (c.has_offset) {  // v += w x r, r = quat_rotate(ee_quat_b_no_offset, offset_pos)
            float r0, r1, r2;
            quat_rotate_ref(eq0, 1.0f, c.offset_pos[0], c.offset_pos[1], c.offset_pos[2], r0, r1, r2);
            vel[0] += vel[4] * r2 - vel[5] * r1;
            vel[1] += vel[5] * r0 - vel[3] * r2;
            vel[2] += vel[3] * r1 - vel[4] * r0;
        }
    }
    // compute_pose_error (utils/math.py:820-867, "axis_angle"), des_ee_acc_b = Kp e + Kd (-v) (operational_space.py:408-423)
    float acc[6];
    {
        float er[6];
        pose_error(ex, ey, ez, eq, px, py, pz, qd, true, er);
IMX_UNROLL
        for (int i = 0; i < 6; ++i) acc[i] = kp[i] * er[i] + kd[i] * (-vel[i]);
    }

    // jacobian_b (:403-410) and _compute_ee_jacobian (:576-595); columns past num_joints hold zeros
    float Jm[6][IMX_OSC_NJ];
    {
        float R[3][3], Ro[3][3];
        matrix_from_quat(q10.x, q10.y, q10.z, q10.w, R);
        matrix_from_quat(c.offset_rot[0], c.offset_rot[1], c.offset_rot[2], c.offset_rot[3], Ro);
        const float ox = c.offset_pos[0], oy = c.offset_pos[1], oz = c.offset_pos[2];
        const float* jrow = io.jacobians + (e * io.NB + c.jacobi_body_idx) * 6 * io.ND;
IMX_UNROLL
        for (int j = 0; j < IMX_OSC_NJ; ++j) {
            const bool on = j < c.num_joints;
            const int64_t col = on ? c.jacobi_joint_ids[j] : c.jacobi_joint_ids[0];  // (a valid column; the value is dropped)
            float v[3], w[3], bv[3], bw[3];
IMX_UNROLL
            for (int r = 0; r < 3; ++r) {
                v[r] = jrow[r * io.ND + col];
                w[r] = jrow[(3 + r) * io.ND + col];
            }
IMX_UNROLL
            for (int r = 0; r < 3; ++r) {  // bmm: sequential dot
                bv[r] = (R[r][0] * v[0] + R[r][1] * v[1]) + R[r][2] * v[2];
                bw[r] = (R[r][0] * w[0] + R[r][1] * w[1]) + R[r][2] * w[2];
            }
            if (c.has_offset) {  // J_v += -[r]x J_w, then J_w = R(offset_rot) J_w
                bv[0] += (0.0f * bw[0] + oz * bw[1]) + (-oy) * bw[2];
                bv[1] += ((-oz) * bw[0] + 0.0f * bw[1]) + ox * bw[2];
                bv[2] += (oy * bw[0] + (-ox) * bw[1]) + 0.0f * bw[2];
                const float t0 = bw[0], t1 = bw[1], t2 = bw[2];
IMX_UNROLL
                for (int r = 0; r < 3; ++r) bw[r] = (Ro[r][0] * t0 + Ro[r][1] * t1) + Ro[r][2] * t2;
            }
IMX_UNROLL
            for (int r = 0; r < 3; ++r) {
                Jm[r][j] = on ? bv[r] : 0.0f;
                Jm[3 + r][j] = on ? bw[r] : 0.0f;
            }
        }
    }

    float tau[IMX_OSC_NJ];
IMX_UNROLL
    for (int j = 0; j < IMX_OSC_NJ; ++j) tau[j] = 0.0f;
    float force[6];  // os_command_forces_b, then S_m F (+ S_f F_wrench - the null-space multiplier)
    if (DEC == IMX_OSC_DECOUPLING_NONE) {
IMX_UNROLL
        for (int i = 0; i < 6; ++i) force[i] = acc[i];
    } else {
        // _compute_dynamic_quantities (:568-574): M[joint_ids][:, joint_ids], lower triangle; rows past num_joints are the identity's
        float L[IMX_OSC_NJ][IMX_OSC_NJ];
        const float* mrow = io.mass + e * io.NM * io.NM;
IMX_UNROLL
        for (int i = 0; i < IMX_OSC_NJ; ++i) {
IMX_UNROLL
            for (int k = 0; k <= i; ++k) {
                const bool on = i < c.num_joints;  // (k <= i)
                const float v = mrow[(int64_t)(on ? c.joint_ids[i] : c.joint_ids[0]) * io.NM + (on ? c.joint_ids[k] : c.joint_ids[0])];
                L[i][k] = on ? v : (i == k ? 1.0f : 0.0f);
            }
        }
        float u[6];  // J qdd of the null-space task
        if (NULLSP) {  // joint_acc_nullspace = kp_n (q* - q) + kd_n (-qd) (operational_space.py:527-534); M qdd before M is factored
            float qdd[IMX_OSC_NJ];
IMX_UNROLL
            for (int j = 0; j < IMX_OSC_NJ; ++j) {
                const bool on = j < c.num_joints;
                const int64_t col = on ? c.joint_ids[j] : c.joint_ids[0];
                const float tq = io.nullspace_target[e * c.num_joints + (on ? j : 0)];
                const float v = c.nullspace_kp * (tq - io.joint_pos[e * io.J + col]) + c.nullspace_kd * (-io.joint_vel[e * io.J + col]);
                qdd[j] = on ? v : 0.0f;
            }
IMX_UNROLL
            for (int i = 0; i < IMX_OSC_NJ; ++i) {
                float s = 0.0f;
IMX_UNROLL
                for (int k = 0; k < IMX_OSC_NJ; ++k) s += (k <= i ? L[i][k] : L[k][i]) * qdd[k];
                tau[i] = i < c.num_joints ? s : 0.0f;
            }
IMX_UNROLL
            for (int r = 0; r < 6; ++r) {
                float s = 0.0f;
IMX_UNROLL
                for (int k = 0; k < IMX_OSC_NJ; ++k) s += Jm[r][k] * qdd[k];
                u[r] = s;
            }
        }
        chol<IMX_OSC_NJ>(L);
        // Y = L^-1 J^T (n x 6): J M^-1 J^T = Y^T Y.  Its Cholesky factor R (Y^T Y = R^T R) is taken from Y by a Gram-Schmidt sweep, column
        // by column, instead of from the product: the product squares Y's condition number, and on a near-singular task space a pivot of
        // the squared matrix drowns in its rounding (a negative square root); R[i][i] = ||column|| cannot.  Partial decoupling factors
        // the translational and the rotational 3 x 3 block on their own (:431-438): columns 3-5 are not swept against columns 0-2.
        float R[6][6];
        {
            constexpr bool PART = DEC == IMX_OSC_DECOUPLING_PARTIAL;
            float Y[IMX_OSC_NJ][6];
IMX_UNROLL
            for (int i = 0; i < IMX_OSC_NJ; ++i) {
                const float inv = 1.0f / L[i][i];
IMX_UNROLL
                for (int r = 0; r < 6; ++r) {
                    float s = Jm[r][i];
IMX_UNROLL
                    for (int k = 0; k < i; ++k) s -= L[i][k] * Y[k][r];
                    Y[i][r] = s * inv;
                }
            }
IMX_UNROLL
            for (int i = 0; i < 6; ++i) {
IMX_UNROLL
                for (int k = 0; k < 6; ++k) {
                    if (k >= i || (PART && (i < 3) != (k < 3))) {
                        if (k != i) R[k][i] = 0.0f;
                        continue;
                    }
                    float r = 0.0f;
IMX_UNROLL
                    for (int j = 0; j < IMX_OSC_NJ; ++j) r += Y[j][k] * Y[j][i];
                    R[k][i] = r;
IMX_UNROLL
                    for (int j = 0; j < IMX_OSC_NJ; ++j) Y[j][i] -= r * Y[j][k];
                }
                float d = 0.0f;
IMX_UNROLL
                for (int j = 0; j < IMX_OSC_NJ; ++j) d += Y[j][i] * Y[j][i];
                d = sqrtf(d);
                R[i][i] = d;
                const float inv = 1.0f / d;
IMX_UNROLL
                for (int j = 0; j < IMX_OSC_NJ; ++j) Y[j][i] *= inv;
            }
        }
IMX_UNROLL
        for (int i = 0; i < 6; ++i) force[i] = acc[i];
        // Lambda a (operational_space.py:441-444) and, for the null space, Lambda (J qdd) (:496-508, 536-538 with M^-1 M = I), solved
        osc_rtr_solve<DEC == IMX_OSC_DECOUPLING_PARTIAL>(R, force);
        if (NULLSP) osc_rtr_solve<false>(R, u);
        if (NULLSP) {
IMX_UNROLL
            for (int i = 0; i < 6; ++i) u[i] = -u[i];
IMX_UNROLL
            for (int j = 0; j < IMX_OSC_NJ; ++j) {  // tau_null = M qdd - J^T Lambda J qdd
                float s = 0.0f;
IMX_UNROLL
                for (int i = 0; i < 6; ++i) s += Jm[i][j] * u[i];
                tau[j] += s;
            }
        }
    }
    // joint_efforts = J^T S_m F + J^T S_f F_wrench (+ g) + tau_null (operational_space.py:452, 475, 483, 543)
IMX_UNROLL
    for (int j = 0; j < IMX_OSC_NJ; ++j) {
        float s = 0.0f;
IMX_UNROLL
        for (int i = 0; i < 6; ++i) s += Jm[i][j] * (c.motion_axes[i] * force[i]);
        float t = s;
        if (c.has_wrench) {
            float sw = 0.0f;
IMX_UNROLL
            for (int i = 0; i < 6; ++i) sw += Jm[i][j] * (c.wrench_axes[i] * fw[i]);
            t += sw;
        }
        if (c.gravity_compensation) t += io.gravity[e * io.NM + (j < c.num_joints ? c.joint_ids[j] : c.joint_ids[0])];
        tau[j] = t + tau[j];
    }
IMX_UNROLL
    for (int j = 0; j < IMX_OSC_NJ; ++j)
        if (j < c.num_joints) io.joint_efforts[e * io.ld_eff + j] = tau[j];
}

// The instantiation of a cfg (the combinations imx_osc_check lets through)
IMX_HD void osc_env_dispatch(const imx_osc_t& c, int64_t e, int mode, const OscIO& io) {
    if (c.decoupling == IMX_OSC_DECOUPLING_FULL) {
        if (c.nullspace_position) osc_env<IMX_OSC_DECOUPLING_FULL, true>(c, e, mode, io);
        else osc_env<IMX_OSC_DECOUPLING_FULL, false>(c, e, mode, io);
    } else if (c.decoupling == IMX_OSC_DECOUPLING_PARTIAL) {
        osc_env<IMX_OSC_DECOUPLING_PARTIAL, false>(c, e, mode, io);
    } else {
        osc_env<IMX_OSC_DECOUPLING_NONE, false>(c, e, mode, io);
    }
}

// What osc_env dereferences, checked before any launch (or host call).  Returns NULL when all is in range, else the reason.
static inline const char* imx_osc_check(const imx_osc_t* c, int64_t N, int mode, const OscIO& io) {
    const int64_t lim = 1ll << 20;
    if (!c) return "null cfg";
    if (N <= 0 || N >= (1ll << 31)) return "num_envs outside [1, 2^31)";
    if (mode < 1 || mode > 3) return "mode must be 1, 2 or 3";
    if (c->pose_type != IMX_OSC_POSE_ABS && c->pose_type != IMX_OSC_POSE_REL) return "unknown pose type";
    if (c->impedance_mode < IMX_OSC_FIXED || c->impedance_mode > IMX_OSC_VARIABLE) return "unknown impedance mode";
    if (c->decoupling < IMX_OSC_DECOUPLING_NONE || c->decoupling > IMX_OSC_DECOUPLING_PARTIAL) return "unknown decoupling";
    if (const char* why = task_space_check(*c, mode, io.num_bodies, io.NB, io.ND, c->nullspace_position ? io.J : 0)) return why;
    if (c->nullspace_position && c->decoupling != IMX_OSC_DECOUPLING_FULL) return "null-space control without full decoupling (it needs an SVD)";
    if (c->nullspace_position && c->num_joints <= 6) return "null-space control on six joints or fewer";
    if (!io.root_pos || !io.root_quat || !io.body_pos || !io.body_quat || !io.command_state) return "null argument";
    if (io.ld_cmd < IMX_OSC_CMD_WIDTH || io.ld_cmd >= lim) return "ld_cmd smaller than 25";
    if (mode & 1) {
        if (!io.processed_action) return "null processed action";
        if (!processed_cols_ok(io.PA, c->pose_col, c->pose_type == IMX_OSC_POSE_ABS ? 7 : 6) || (c->has_wrench && !processed_cols_ok(io.PA, c->wrench_col, 6)) ||
            (c->impedance_mode != IMX_OSC_FIXED && !processed_cols_ok(io.PA, c->stiffness_col, 6)) ||
            (c->impedance_mode == IMX_OSC_VARIABLE && !processed_cols_ok(io.PA, c->damping_ratio_col, 6)))
            return "processed columns outside [0, PA)";
    }
    if (mode & 2) {
        if (!io.jacobians || !io.joint_efforts || !io.root_lin_vel || !io.root_ang_vel || !io.body_lin_vel || !io.body_ang_vel) return "null argument";
        if (io.ND <= 0 || io.ND >= lim) return "bad ND";
        if (io.ld_eff < c->num_joints || io.ld_eff >= lim) return "ld_eff smaller than num_joints";
        const bool dyn = c->decoupling != IMX_OSC_DECOUPLING_NONE, jnt = c->nullspace_position != 0;
        if (dyn && !io.mass) return "null mass matrices";
        if (c->gravity_compensation && !io.gravity) return "null gravity";
        if ((dyn || c->gravity_compensation) && (io.NM <= 0 || io.NM >= 32768)) return "bad NM";
        if (jnt && (!io.joint_pos || !io.joint_vel || !io.nullspace_target)) return "null joint state or null-space target";
        if (jnt && (io.J <= 0 || io.J >= lim)) return "bad J";
        for (int j = 0; j < c->num_joints; ++j)
            if ((dyn || c->gravity_compensation) && c->joint_ids[j] >= io.NM) return "mass-matrix row outside [0, NM)";
    }
    return nullptr;
}
