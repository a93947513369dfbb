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
#include "imx_task_space.h"

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
        chol<M>(A);  // A z = dx: lambda = 0 on a rank-deficient Jacobian gives NaN / inf
        chol_substitute<M>(A, z);
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
    const TaskFrame f = task_frame(c, e, io);  // ---- _compute_frame_pose (task_space_actions.py:188-207)
    const float ex = f.ex, ey = f.ey, ez = f.ez;
    const float4 eq = f.eq;

    float px, py, pz;  // ee_pos_des
    float4 qd;         // ee_quat_des
    if (mode & 1) {    // ---- DifferentialIKController.set_command (differential_ik.py:98-146)
        const float* a = io.processed_action + e * io.PA + c.processed_col;
        if (c.command_type == IMX_IK_POSITION) {
            px = a[0]; py = a[1]; pz = a[2];
            if (c.use_relative_mode) { px = ex + px; py = ey + py; pz = ez + pz; }
            qd = eq;
        } else if (c.use_relative_mode) {
            apply_delta_pose(ex, ey, ez, eq, a, px, py, pz, qd);
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
    float dx[6];
    pose_error(ex, ey, ez, eq, px, py, pz, qd, c.command_type == IMX_IK_POSE, dx);
    // the angular rows enter a position-only solve through the offset correction alone
    float Jm[6][IMX_IK_MAX_JOINTS];
    frame_jacobian(c, f.q10, jrow, io.ND, c.command_type == IMX_IK_POSE || c.has_offset, Jm);
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
    if (const char* why = task_space_check(*c, mode, io.num_bodies, io.NB, io.ND, io.J)) return why;
    if (!io.root_pos || !io.root_quat || !io.body_pos || !io.body_quat || !io.ee_pos_des || !io.ee_quat_des) return "null argument";
    if (mode & 1) {
        const int width = c->command_type == IMX_IK_POSITION ? 3 : (c->use_relative_mode ? 6 : 7);
        if (!io.processed_action) return "null processed action";
        if (!processed_cols_ok(io.PA, c->processed_col, width)) return "processed columns outside [0, PA)";
    }
    if (mode & 2) {
        if (!io.jacobians || !io.joint_pos || !io.joint_pos_des) return "null argument";
        if (io.ND <= 0 || io.ND >= (1ll << 20) || io.J <= 0 || io.J >= (1ll << 20)) return "bad ND or J";
        if (io.ld_des < c->num_joints || io.ld_des >= (1ll << 20)) return "ld_des smaller than num_joints";
    }
    return nullptr;
}
