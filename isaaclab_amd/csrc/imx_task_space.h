// What the task-space action terms share for ONE env: the end-effector frame in the root frame, the pose delta and the pose error, the
// frame Jacobian, and the in-register Cholesky solve (envs/mdp/actions/task_space_actions.py:142-229, 403-410, 576-615 with
// utils/math.py).  Used by imx_diff_ik.h and, for the pieces that leave its kernels as they were, imx_osc.h; like them it compiles as
// gfx950 device code and as plain host C++.
//
// Cfg is imx_diff_ik_t or imx_osc_t (body_idx, has_offset, offset_pos, offset_rot, num_joints, jacobi_joint_ids, ... carry the same
// names in both); IO is the term's own struct of pointers.  Matrices are references to register arrays and every loop over them is
// fully unrolled: a pointer into one would put it in scratch.
#pragma once
#include "../../include/imx.h"
#include "imx_quat.h"

IMX_HD void matrix_from_quat(float r, float i, float j, float k, float (&R)[3][3]) {  // utils/math.py:144-174
    const float two_s = 2.0f / ((r * r + i * i) + (j * j + k * k));
    R[0][0] = 1.0f - two_s * (j * j + k * k); R[0][1] = two_s * (i * j - k * r); R[0][2] = two_s * (i * k + j * r);
    R[1][0] = two_s * (i * j + k * r); R[1][1] = 1.0f - two_s * (i * i + k * k); R[1][2] = two_s * (j * k - i * r);
    R[2][0] = two_s * (i * k - j * r); R[2][1] = two_s * (j * k + i * r); R[2][2] = 1.0f - two_s * (i * i + j * j);
}

// quat_inv = normalize(conjugate) (utils/math.py:239-248, 82-92: x / norm.clamp(min=1e-9))
IMX_HD float4 quat_inv(float4 q) {
    const float n = fmaxf(sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w)), 1.0e-9f);
    return make_float4(q.x / n, -q.y / n, -q.z / n, -q.w / n);
}

struct TaskFrame {
    float4 rq, q10;    // the root's quaternion and its quat_inv
    int64_t b;         // the body's row: e * num_bodies + body_idx
    float ex, ey, ez;  // the body's pose in the root frame, with the offset
    float4 eq;
    float4 eq0;        // its rotation without the offset (_ee_pose_b_no_offset)
};

// _compute_frame_pose (task_space_actions.py:188-207) / _compute_ee_pose (:597-615)
template <class Cfg, class IO>
IMX_HD TaskFrame task_frame(const Cfg& c, int64_t e, const IO& io) {
    TaskFrame f;
    f.rq = make_float4(io.root_quat[e * 4], io.root_quat[e * 4 + 1], io.root_quat[e * 4 + 2], io.root_quat[e * 4 + 3]);
    f.q10 = quat_inv(f.rq);
    const int64_t b = f.b = e * io.num_bodies + c.body_idx;
    const float4 bq = make_float4(io.body_quat[b * 4], io.body_quat[b * 4 + 1], io.body_quat[b * 4 + 2], io.body_quat[b * 4 + 3]);
    // subtract_frame_transforms (utils/math.py:785-816)
    f.eq = f.eq0 = quat_mul_ref(f.q10, bq);
    quat_apply(f.q10.x, f.q10.y, f.q10.z, f.q10.w, io.body_pos[b * 3] - io.root_pos[e * 3], io.body_pos[b * 3 + 1] - io.root_pos[e * 3 + 1],
               io.body_pos[b * 3 + 2] - io.root_pos[e * 3 + 2], f.ex, f.ey, f.ez);
    if (c.has_offset) {  // combine_frame_transforms (:750-781)
        float ox, oy, oz;
        quat_apply(f.eq.x, f.eq.y, f.eq.z, f.eq.w, c.offset_pos[0], c.offset_pos[1], c.offset_pos[2], ox, oy, oz);
        f.ex += ox; f.ey += oy; f.ez += oz;
        f.eq = quat_mul_ref(f.eq, make_float4(c.offset_rot[0], c.offset_rot[1], c.offset_rot[2], c.offset_rot[3]));
    }
    return f;
}

// apply_delta_pose (utils/math.py:873-910) of the six values at `a` on the pose (ex, ey, ez, q)
IMX_HD void apply_delta_pose(float ex, float ey, float ez, float4 q, const float* a, float& px, float& py, float& pz, float4& qd) {
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
    qd = quat_mul_ref(dq4, q);
}

// compute_pose_error (utils/math.py:820-867, "axis_angle") of the pose (ex, ey, ez, eq) against (px, py, pz, qd); rot: the rotation rows too
IMX_HD void pose_error(float ex, float ey, float ez, float4 eq, float px, float py, float pz, float4 qd, bool rot, float (&er)[6]) {
    er[0] = px - ex; er[1] = py - ey; er[2] = pz - ez;
    er[3] = 0.0f; er[4] = 0.0f; er[5] = 0.0f;
    if (rot) axis_angle_from_quat_ref(quat_error_ref(qd, eq), er[3], er[4], er[5]);
}

// jacobian_b (:142-149, 403-410): R = matrix_from_quat(quat_inv(root_quat)) on both 3-row blocks, then _compute_frame_jacobian
// (:209-229, 576-595) for the offset; columns past num_joints hold zeros.  jrow: the env's own 6 x ND block of the selected body
// (global memory, or a staged copy), element (r, c) at jrow[r * ND + c].  need_w = false leaves the angular rows unread (as zeros).
template <class Cfg>
IMX_HD void frame_jacobian(const Cfg& c, float4 q10, const float* jrow, int64_t ND, bool need_w, float (&Jm)[6][IMX_IK_MAX_JOINTS]) {
    float R[3][3], Ro[3][3];
    matrix_from_quat(q10.x, q10.y, q10.z, q10.w, R);
    matrix_from_quat(c.offset_rot[0], c.offset_rot[1], c.offset_rot[2], c.offset_rot[3], Ro);
    const float ox = c.offset_pos[0], oy = c.offset_pos[1], oz = c.offset_pos[2];
IMX_UNROLL
    for (int j = 0; j < IMX_IK_MAX_JOINTS; ++j) {
        const bool on = j < c.num_joints;
        const int64_t col = on ? c.jacobi_joint_ids[j] : c.jacobi_joint_ids[0];  // (a valid column; the value is dropped)
        float v[3], w[3] = {0.0f, 0.0f, 0.0f};
IMX_UNROLL
        for (int r = 0; r < 3; ++r) v[r] = jrow[r * ND + col];
        if (need_w) {
IMX_UNROLL
            for (int r = 0; r < 3; ++r) w[r] = jrow[(3 + r) * ND + col];
        }
        float bv[3], bw[3];
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

// A = L L^T in place (lower triangle; only the lower triangle is read), for a symmetric positive definite M x M matrix held in
// registers.  A matrix that is not positive definite gives NaN / inf.
template <int M>
IMX_HD void chol(float (&A)[M][M]) {
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
}

// L L^T z = b in place of b, L the factor chol left in A: L y = b, L^T z = y
template <int M>
IMX_HD void chol_substitute(const float (&A)[M][M], float (&b)[M]) {
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

static inline bool processed_cols_ok(int64_t PA, int col, int width) {
    return PA > 0 && PA < (1ll << 20) && col >= 0 && col + width <= PA;
}

// The cfg indices both terms dereference through, checked on the host before any launch: returns NULL or the reason.  `mode & 2`
// adds what the Jacobian needs.  J: the joint count joint_ids must stay below, 0 where the term reads no joint array.  A count
// outside its range (ND, J <= 0) is left to the term's own message.
template <class Cfg>
static inline const char* task_space_check(const Cfg& c, int mode, int64_t num_bodies, int64_t NB, int64_t ND, int64_t J) {
    const int64_t lim = 1ll << 20;
    if (c.num_joints < 1 || c.num_joints > IMX_IK_MAX_JOINTS) return "num_joints outside [1, 8]";
    if (num_bodies <= 0 || num_bodies >= lim || c.body_idx < 0 || c.body_idx >= num_bodies) return "body_idx outside [0, num_bodies)";
    if (!(mode & 2)) return nullptr;
    if (NB <= 0 || NB >= lim || c.jacobi_body_idx < 0 || c.jacobi_body_idx >= NB) return "jacobi_body_idx outside [0, NB)";
    for (int j = 0; j < c.num_joints; ++j) {
        if (c.joint_ids[j] < 0 || (J > 0 && c.joint_ids[j] >= J)) return "joint id outside [0, J)";
        if (c.jacobi_joint_ids[j] < 0 || (ND > 0 && c.jacobi_joint_ids[j] >= ND)) return "Jacobian column outside [0, ND)";
    }
    return nullptr;
}
