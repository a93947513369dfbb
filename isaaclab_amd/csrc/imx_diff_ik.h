// DifferentialInverseKinematicsAction for ONE env (envs/mdp/actions/task_space_actions.py:155-229 with
// controllers/differential_ik.py:98-240).  Shared by the kernel (diff_ik.hip) and by the host program tools/diff_ik_host.cpp: this file
// compiles as gfx950 device code and as plain host C++.
//
// The reference's global test `ee_quat_curr.norm() != 0` (task_space_actions.py:173) is one host sync over all envs and is false only
// before the simulation has produced a pose; it is not reproduced: apply_actions always computes.
//
// No value can move an access: every index comes from the cfg (checked on the host, imx_diff_ik_check) and the env index.  NaN or zero
// quaternions and lambda = 0 give NaN / inf in the outputs.
#pragma once
#include "../../include/imx.h"
#include "imx_quat.h"

struct DiffIkIO {
    const float* processed_action;  // (N, PA)
    int64_t PA;
    const float* root_pos;          // (N,3)
    const float* root_quat;         // (N,4)
    const float* body_pos;          // (N, num_bodies, 3)
    const float* body_quat;         // (N, num_bodies, 4)
    int64_t num_bodies;
    const float* jacobians;         // (N, NB, 6, ND)
    int64_t NB, ND;
    const float* joint_pos;         // (N, J)
    int64_t J;
    float* ee_pos_des;              // (N,3)
    float* ee_quat_des;             // (N,4)
    float* joint_pos_des;           // (N, ld_des)
    int64_t ld_des;
};

// Solve (A) z = b for a symmetric positive definite M x M matrix held in registers: A = L L^T, L y = b, L^T z = y.  Only the lower
// triangle of A is read.  A matrix that is not positive definite (lambda = 0 on a rank-deficient Jacobian) gives NaN / inf.
template <int M>
IMX_HD void chol_solve(float (&A)[M][M], float (&b)[M]) {
IMX_UNROLL
    for (int j = 0; j < M; ++j) {
        float d = A[j][j];
IMX_UNROLL
        for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
        d = sqrtf(d);
        A[j][j] = d;
        const float inv = 1.0f / d;
IMX_UNROLL
        for (int i = j + 1; i < M; ++i) {
            float s = A[i][j];
IMX_UNROLL
            for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
            A[i][j] = s * inv;
        }
    }
IMX_UNROLL
    for (int i = 0; i < M; ++i) {  // L y = b
        float s = b[i];
IMX_UNROLL
        for (int k = 0; k < i; ++k) s -= A[i][k] * b[k];
        b[i] = s / A[i][i];
    }
IMX_UNROLL
    for (int i = M - 1; i >= 0; --i) {  // L^T z = y
        float s = b[i];
IMX_UNROLL
        for (int k = i + 1; k < M; ++k) s -= A[k][i] * b[k];
        b[i] = s / A[i][i];
    }
}

// dq = J^T (J J^T + lambda^2 I)^-1 dx (dls) or k J^T dx (trans) over the first M rows of Jm (differential_ik.py:180-240)
template <int M>
IMX_HD void diff_ik_delta(const imx_diff_ik_t& c, const float (&Jm)[6][IMX_IK_MAX_JOINTS], const float (&dx6)[6], float (&dq)[IMX_IK_MAX_JOINTS]) {
    float z[M];
IMX_UNROLL
    for (int i = 0; i < M; ++i) z[i] = dx6[i];
    float scale = c.k_val;
    if (c.ik_method == IMX_IK_DLS) {
        float A[M][M];
        const float l2 = c.lambda_val * c.lambda_val;
IMX_UNROLL
        for (int i = 0; i < M; ++i) {
IMX_UNROLL
            for (int k = 0; k <= i; ++k) {
                float s = 0.0f;
IMX_UNROLL
                for (int j = 0; j < IMX_IK_MAX_JOINTS; ++j) s += Jm[i][j] * Jm[k][j];  // (columns past num_joints hold zeros)
                A[i][k] = (i == k) ? s + l2 : s;
            }
        }
        chol_solve<M>(A, z);
        scale = 1.0f;
    }
IMX_UNROLL
    for (int j = 0; j < IMX_IK_MAX_JOINTS; ++j) {
        float s = 0.0f;
IMX_UNROLL
        for (int i = 0; i < M; ++i) s += (scale * Jm[i][j]) * z[i];
        dq[j] = s;
    }
}

// jrow: the env's own 6 x ND block of the selected body (global memory, or a staged copy); element (r, c) at jrow[r * ND + c].
IMX_HD void diff_ik_env(const imx_diff_ik_t& c, int64_t e, int mode, const DiffIkIO& io, const float* jrow) {
    // ---- _compute_frame_pose (task_space_actions.py:188-207)
    const float4 rq = make_float4(io.root_quat[e * 4], io.root_quat[e * 4 + 1], io.root_quat[e * 4 + 2], io.root_quat[e * 4 + 3]);
    // quat_inv = normalize(conjugate) (utils/math.py:239-248, 82-92: x / norm.clamp(min=1e-9))
    const float rn = fmaxf(sqrtf((rq.x * rq.x + rq.y * rq.y) + (rq.z * rq.z + rq.w * rq.w)), 1.0e-9f);
    const float4 q10 = make_float4(rq.x / rn, -rq.y / rn, -rq.z / rn, -rq.w / rn);
    const int64_t b = e * io.num_bodies + c.body_idx;
    const float4 bq = make_float4(io.body_quat[b * 4], io.body_quat[b * 4 + 1], io.body_quat[b * 4 + 2], io.body_quat[b * 4 + 3]);
    // subtract_frame_transforms (utils/math.py:785-816)
    float4 eq = quat_mul_ref(q10, bq);
    float ex, ey, ez;
    quat_apply(q10.x, q10.y, q10.z, q10.w, io.body_pos[b * 3] - io.root_pos[e * 3], io.body_pos[b * 3 + 1] - io.root_pos[e * 3 + 1],
               io.body_pos[b * 3 + 2] - io.root_pos[e * 3 + 2], ex, ey, ez);
    if (c.has_offset) {  // combine_frame_transforms (:750-781)
        float ox, oy, oz;
        quat_apply(eq.x, eq.y, eq.z, eq.w, c.offset_pos[0], c.offset_pos[1], c.offset_pos[2], ox, oy, oz);
        ex += ox; ey += oy; ez += oz;
        eq = quat_mul_ref(eq, make_float4(c.offset_rot[0], c.offset_rot[1], c.offset_rot[2], c.offset_rot[3]));
    }

    float px, py, pz;  // ee_pos_des
    float4 qd;         // ee_quat_des
    if (mode & 1) {    // ---- DifferentialIKController.set_command (differential_ik.py:98-146)
        const float* a = io.processed_action + e * io.PA + c.processed_col;
        if (c.command_type == IMX_IK_POSITION) {
            px = a[0]; py = a[1]; pz = a[2];
            if (c.use_relative_mode) { px = ex + px; py = ey + py; pz = ez + pz; }
            qd = eq;
        } else if (c.use_relative_mode) {  // apply_delta_pose (utils/math.py:873-910)
            px = ex + a[0]; py = ey + a[1]; pz = ez + a[2];
            const float rx = a[3], ry = a[4], rz = a[5];
            const float angle = sqrtf((rx * rx + ry * ry) + rz * rz);
            const float axx = rx / angle, axy = ry / angle, axz = rz / angle;
            // quat_from_angle_axis (:629-642): normalize(axis) * sin(angle / 2), cos(angle / 2), normalize
            const float an = fmaxf(sqrtf((axx * axx + axy * axy) + axz * axz), 1.0e-9f);
            const float th = angle / 2.0f, sn = sinf(th), w = cosf(th);
            const float x = axx / an * sn, y = axy / an * sn, z = axz / an * sn;
            const float qn = fmaxf(sqrtf((w * w + x * x) + (y * y + z * z)), 1.0e-9f);
            const bool on = angle > 1.0e-6f;  // (NaN: identity, as torch.where picks)
            const float4 dq4 = make_float4(on ? w / qn : 1.0f, on ? x / qn : 0.0f, on ? y / qn : 0.0f, on ? z / qn : 0.0f);
            qd = quat_mul_ref(dq4, eq);
        } else {
            px = a[0]; py = a[1]; pz = a[2];
            qd = make_float4(a[3], a[4], a[5], a[6]);
        }
        io.ee_pos_des[e * 3] = px; io.ee_pos_des[e * 3 + 1] = py; io.ee_pos_des[e * 3 + 2] = pz;
        io.ee_quat_des[e * 4] = qd.x; io.ee_quat_des[e * 4 + 1] = qd.y; io.ee_quat_des[e * 4 + 2] = qd.z; io.ee_quat_des[e * 4 + 3] = qd.w;
    } else {
        px = io.ee_pos_des[e * 3]; py = io.ee_pos_des[e * 3 + 1]; pz = io.ee_pos_des[e * 3 + 2];
        qd = make_float4(io.ee_quat_des[e * 4], io.ee_quat_des[e * 4 + 1], io.ee_quat_des[e * 4 + 2], io.ee_quat_des[e * 4 + 3]);
    }
    if (!(mode & 2)) return;

    // ---- apply_actions (:168-179)
    float dx[6] = {px - ex, py - ey, pz - ez, 0.0f, 0.0f, 0.0f};
    if (c.command_type == IMX_IK_POSE) {  // compute_pose_error (utils/math.py:820-867): target * conj(source) / (source * conj(source)).w
        const float4 conj = make_float4(eq.x, -eq.y, -eq.z, -eq.w);
        const float nrm = quat_mul_ref(eq, conj).x;
        const float4 inv = make_float4(conj.x / nrm, conj.y / nrm, conj.z / nrm, conj.w / nrm);
        axis_angle_from_quat_ref(quat_mul_ref(qd, inv), dx[3], dx[4], dx[5]);
    }
    // jacobian_b (:142-149): R = matrix_from_quat(quat_inv(root_quat)) (utils/math.py:144-174) on both 3-row blocks
    float R[3][3];
    {
        const float r = q10.x, i = q10.y, j = q10.z, k = q10.w;
        const float two_s = 2.0f / ((r * r + i * i) + (j * j + k * k));
        R[0][0] = 1.0f - two_s * (j * j + k * k); R[0][1] = two_s * (i * j - k * r); R[0][2] = two_s * (i * k + j * r);
        R[1][0] = two_s * (i * j + k * r); R[1][1] = 1.0f - two_s * (i * i + k * k); R[1][2] = two_s * (j * k - i * r);
        R[2][0] = two_s * (i * k - j * r); R[2][1] = two_s * (j * k + i * r); R[2][2] = 1.0f - two_s * (i * i + j * j);
    }
    float Ro[3][3];  // matrix_from_quat(offset_rot)
    {
        const float r = c.offset_rot[0], i = c.offset_rot[1], j = c.offset_rot[2], k = c.offset_rot[3];
        const float two_s = 2.0f / ((r * r + i * i) + (j * j + k * k));
        Ro[0][0] = 1.0f - two_s * (j * j + k * k); Ro[0][1] = two_s * (i * j - k * r); Ro[0][2] = two_s * (i * k + j * r);
        Ro[1][0] = two_s * (i * j + k * r); Ro[1][1] = 1.0f - two_s * (i * i + k * k); Ro[1][2] = two_s * (j * k - i * r);
        Ro[2][0] = two_s * (i * k - j * r); Ro[2][1] = two_s * (j * k + i * r); Ro[2][2] = 1.0f - two_s * (i * i + j * j);
    }
    const float ox = c.offset_pos[0], oy = c.offset_pos[1], oz = c.offset_pos[2];
    // the angular rows enter a position-only solve through the offset correction alone
    const bool need_w = c.command_type == IMX_IK_POSE || c.has_offset;
    float Jm[6][IMX_IK_MAX_JOINTS];
IMX_UNROLL
    for (int j = 0; j < IMX_IK_MAX_JOINTS; ++j) {
        const bool on = j < c.num_joints;
        const int64_t col = on ? c.jacobi_joint_ids[j] : c.jacobi_joint_ids[0];  // (a valid column; the value is dropped)
        float v[3], w[3] = {0.0f, 0.0f, 0.0f};
IMX_UNROLL
        for (int r = 0; r < 3; ++r) v[r] = jrow[r * io.ND + col];
        if (need_w) {
IMX_UNROLL
            for (int r = 0; r < 3; ++r) w[r] = jrow[(3 + r) * io.ND + col];
        }
        float bv[3], bw[3];
IMX_UNROLL
        for (int r = 0; r < 3; ++r) {  // bmm: sequential dot
            bv[r] = (R[r][0] * v[0] + R[r][1] * v[1]) + R[r][2] * v[2];
            bw[r] = (R[r][0] * w[0] + R[r][1] * w[1]) + R[r][2] * w[2];
        }
        if (c.has_offset) {  // _compute_frame_jacobian (:209-229): J_v += -[r]x J_w, then J_w = R(offset_rot) J_w
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
    float dq[IMX_IK_MAX_JOINTS];
    if (c.command_type == IMX_IK_POSE) diff_ik_delta<6>(c, Jm, dx, dq);
    else diff_ik_delta<3>(c, Jm, dx, dq);
IMX_UNROLL
    for (int j = 0; j < IMX_IK_MAX_JOINTS; ++j)
        if (j < c.num_joints) io.joint_pos_des[e * io.ld_des + j] = io.joint_pos[e * io.J + c.joint_ids[j]] + dq[j];
}

// What diff_ik_env dereferences, checked before any launch (or host call).  Returns NULL when all is in range, else the reason.
static inline const char* imx_diff_ik_check(const imx_diff_ik_t* c, int64_t N, int mode, const DiffIkIO& io) {
    if (!c) return "null cfg";
    if (N <= 0 || N >= (1ll << 31)) return "num_envs outside [1, 2^31)";
    if (mode < 1 || mode > 3) return "mode must be 1, 2 or 3";
    if (c->command_type != IMX_IK_POSITION && c->command_type != IMX_IK_POSE) return "unknown command type";
    if (c->ik_method != IMX_IK_DLS && c->ik_method != IMX_IK_TRANS) return "unknown ik method (dls and trans are built)";
    if (c->num_joints < 1 || c->num_joints > IMX_IK_MAX_JOINTS) return "num_joints outside [1, 8]";
    if (!io.root_pos || !io.root_quat || !io.body_pos || !io.body_quat || !io.ee_pos_des || !io.ee_quat_des) return "null argument";
    if (io.num_bodies <= 0 || io.num_bodies >= (1ll << 20) || c->body_idx < 0 || c->body_idx >= io.num_bodies) return "body_idx outside [0, num_bodies)";
    if (mode & 1) {
        const int width = c->command_type == IMX_IK_POSITION ? 3 : (c->use_relative_mode ? 6 : 7);
        if (!io.processed_action) return "null processed action";
        if (io.PA <= 0 || io.PA >= (1ll << 20) || c->processed_col < 0 || c->processed_col + width > io.PA) return "processed columns outside [0, PA)";
    }
    if (mode & 2) {
        if (!io.jacobians || !io.joint_pos || !io.joint_pos_des) return "null argument";
        if (io.NB <= 0 || io.NB >= (1ll << 20) || c->jacobi_body_idx < 0 || c->jacobi_body_idx >= io.NB) return "jacobi_body_idx outside [0, NB)";
        if (io.ND <= 0 || io.ND >= (1ll << 20) || io.J <= 0 || io.J >= (1ll << 20)) return "bad ND or J";
        if (io.ld_des < c->num_joints || io.ld_des >= (1ll << 20)) return "ld_des smaller than num_joints";
        for (int j = 0; j < c->num_joints; ++j) {
            if (c->joint_ids[j] < 0 || c->joint_ids[j] >= io.J) return "joint id outside [0, J)";
            if (c->jacobi_joint_ids[j] < 0 || c->jacobi_joint_ids[j] >= io.ND) return "Jacobian column outside [0, ND)";
        }
    }
    return nullptr;
}
