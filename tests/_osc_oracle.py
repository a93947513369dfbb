"""TEST INFRASTRUCTURE -- a torch restatement of ``OperationalSpaceControllerAction`` (reference
``isaaclab/envs/mdp/actions/task_space_actions.py:232-700``) with ``OperationalSpaceController`` (``controllers/operational_space.py:34-548``)
and the ``utils/math.py`` helpers they call, written for this repository.  It works in the dtype of the tensors it is given (fp32 in the
tests).  Deliberate departures, the same as the kernel's: only the identity task frame (so gains, selection matrices and wrench are
diagonal / unrotated), linear systems are solved instead of inverses being formed (M by a Cholesky factor, J M^-1 J^T by the QR
factor of L^-1 J^T), the null-space term is ``M qdd - J^T Lambda (J qdd)`` (M^-1 M = I), and only the open-loop wrench exists.

The term is a ``plan.OscTerm`` (``resolve_osc_term``).  ``s`` is a dict of the state tensors under the state feed's names.
"""

from __future__ import annotations

import torch

from _diff_ik_oracle import apply_delta_pose, axis_angle_from_quat, matrix_from_quat, normalize, quat_apply, quat_conjugate, quat_mul


def quat_rotate(q, v, sign=1.0):  # utils/math.py:583-625 (sign -1: quat_rotate_inverse)
    w, xyz = q[:, 0:1], q[:, 1:]
    a = v * (2.0 * w ** 2 - 1.0)
    b = torch.linalg.cross(xyz, v, dim=-1) * w * 2.0
    c = xyz * (xyz * v).sum(-1, keepdim=True) * 2.0
    return a + sign * b + c


class OscOracle:
    def __init__(self, osc, num_envs: int, nullspace_target=None, dtype=torch.float32):
        self.osc, self.N, self.dtype = osc, num_envs, dtype
        t = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
        self.raw_actions = torch.zeros(num_envs, osc.width, dtype=dtype)
        self.processed_actions = torch.zeros(num_envs, osc.width, dtype=dtype)
        self.scale, self.clip = t(osc.scale), t(osc.clip)
        self.offset_pos = None if osc.offset_pos is None else t(osc.offset_pos).repeat(num_envs, 1)
        self.offset_rot = None if osc.offset_rot is None else t(osc.offset_rot).repeat(num_envs, 1)
        self.s_motion, self.s_force = t(osc.motion_control_axes), t(osc.contact_wrench_control_axes)
        self.kp = (self.s_motion * t(osc.motion_stiffness)).repeat(num_envs, 1)  # operational_space.py:90-101
        self.kd = 2 * self.kp.sqrt() * t(osc.motion_damping_ratio)
        self.pose_des = torch.zeros(num_envs, 7, dtype=dtype)
        self.wrench = torch.zeros(num_envs, 6, dtype=dtype)
        self.null_kp = t(osc.nullspace_stiffness)
        self.null_kd = 2 * torch.sqrt(self.null_kp) * t(osc.nullspace_damping_ratio)
        self.nullspace_target = nullspace_target
        self.joint_efforts = torch.zeros(num_envs, len(osc.joint_ids), dtype=dtype)

    @property
    def command_state(self):
        return torch.cat([self.pose_des, self.kp, self.kd, self.wrench], dim=1)

    def reset(self, env_ids):  # :464-474
        self.raw_actions[env_ids] = 0.0

    def ee_pose(self, s):  # _compute_ee_pose :597-615
        b = self.osc.body_idx
        q10 = normalize(quat_conjugate(s["root_quat_w"]))
        quat0 = quat_mul(q10, s["body_quat_w"][:, b])
        pos = quat_apply(q10, s["body_pos_w"][:, b] - s["root_pos_w"])
        quat = quat0
        if self.offset_pos is not None:
            pos, quat = pos + quat_apply(quat0, self.offset_pos), quat_mul(quat0, self.offset_rot)
        return pos, quat, quat0

    def process_actions(self, raw):  # _preprocess_actions :664-700
        self.raw_actions[:] = raw
        self.processed_actions = torch.clamp(self.raw_actions * self.scale, min=self.clip[:, 0], max=self.clip[:, 1])

    def set_command(self, s):  # operational_space.py:173-343 with the identity task frame
        o, cmd = self.osc, self.processed_actions
        lim = o.motion_stiffness_limits
        if o.impedance_mode != "fixed":
            k = cmd[:, o.stiffness_idx:o.stiffness_idx + 6].clamp(lim[0], lim[1])
            self.kp = self.s_motion * k
            ratio = torch.tensor(o.motion_damping_ratio, dtype=self.dtype)
            if o.impedance_mode == "variable":
                ratio = cmd[:, o.damping_ratio_idx:o.damping_ratio_idx + 6].clamp(*o.motion_damping_ratio_limits)
            self.kd = 2 * self.kp.sqrt() * ratio
        ident = torch.zeros(self.N, 4, dtype=self.dtype)
        ident[:, 0] = 1.0
        if o.pose_type == "pose_rel":
            pos, quat, _ = self.ee_pose(s)
            cur = quat_mul(normalize(quat_conjugate(ident)), quat)
            p, q = apply_delta_pose(pos, cur, cmd[:, o.pose_idx:o.pose_idx + 6])
        else:
            p, q = cmd[:, o.pose_idx:o.pose_idx + 3], cmd[:, o.pose_idx + 3:o.pose_idx + 7]
        self.pose_des = torch.cat([p, quat_mul(ident, q)], dim=1)
        if o.wrench_idx is not None:
            self.wrench = cmd[:, o.wrench_idx:o.wrench_idx + 6].clone()

    def ee_jacobian(self, s):  # jacobian_b :403-410, _compute_ee_jacobian :576-595
        o = self.osc
        jac = s["jacobians"][:, o.jacobi_body_idx][:, :, o.jacobi_joint_ids].clone()
        R = matrix_from_quat(normalize(quat_conjugate(s["root_quat_w"])))
        jac[:, :3] = torch.bmm(R, jac[:, :3])
        jac[:, 3:] = torch.bmm(R, jac[:, 3:])
        if self.offset_pos is not None:
            r = self.offset_pos
            skew = torch.zeros(self.N, 3, 3, dtype=self.dtype)
            skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -r[:, 2], r[:, 1], -r[:, 0]
            skew[:, 1, 0], skew[:, 2, 0], skew[:, 2, 1] = r[:, 2], -r[:, 1], r[:, 0]
            jac[:, 0:3] += torch.bmm(-skew, jac[:, 3:])
            jac[:, 3:] = torch.bmm(matrix_from_quat(self.offset_rot), jac[:, 3:])
        return jac

    def ee_velocity(self, s, quat0):  # _compute_ee_velocity :617-634
        b = self.osc.body_idx
        lin = quat_rotate(s["root_quat_w"], s["body_lin_vel_w"][:, b] - s["root_lin_vel_w"], -1.0)
        ang = quat_rotate(s["root_quat_w"], s["body_ang_vel_w"][:, b] - s["root_ang_vel_w"], -1.0)
        if self.offset_pos is not None:
            lin = lin + torch.linalg.cross(ang, quat_rotate(quat0, self.offset_pos), dim=-1)
        return torch.cat([lin, ang], dim=1)

    def apply_actions(self, s):  # :440-462, operational_space.py:345-548
        o = self.osc
        pos, quat, quat0 = self.ee_pose(s)
        jac = self.ee_jacobian(s)
        vel = self.ee_velocity(s, quat0)
        conj = quat_conjugate(quat)
        inv = conj / quat_mul(quat, conj)[:, 0:1]
        err = torch.cat([self.pose_des[:, :3] - pos, axis_angle_from_quat(quat_mul(self.pose_des[:, 3:], inv))], dim=1)
        force = self.kp * err + self.kd * (-vel)
        jt = jac.transpose(1, 2)
        ids = o.joint_ids
        if o.decoupling != "none":
            # J M^-1 J^T = Y^T Y with Y = L^-1 J^T, M = L L^T; its factor R comes from a QR of Y, not from the product (which squares the
            # condition number): Lambda b = R^-1 R^-T b.  Partial decoupling: the two 3-column halves of Y on their own
            M = s["mass_matrices"][:, ids][:, :, ids]
            M = torch.tril(M) + torch.tril(M, -1).transpose(1, 2)  # (the lower triangle is what is read)
            Y = torch.linalg.solve_triangular(torch.linalg.cholesky(M), jt, upper=False)
            blocks = [(0, 3), (3, 6)] if o.decoupling == "partial" else [(0, 6)]
            Rs = [torch.linalg.qr(Y[:, :, lo:hi]).R for lo, hi in blocks]

            def lam(b):  # (N, 6, 1)
                out = []
                for (lo, hi), R in zip(blocks, Rs):
                    y = torch.linalg.solve_triangular(R.transpose(1, 2), b[:, lo:hi], upper=False)
                    out.append(torch.linalg.solve_triangular(R, y, upper=True))
                return torch.cat(out, dim=1)

            force = lam(force.unsqueeze(-1)).squeeze(-1)
        tau = (jt @ (self.s_motion * force).unsqueeze(-1)).squeeze(-1)
        if o.wrench_idx is not None:
            tau = tau + (jt @ (self.s_force * self.wrench).unsqueeze(-1)).squeeze(-1)
        if o.gravity_compensation:
            tau = tau + s["gravity_compensation_forces"][:, ids]
        if o.nullspace_control == "position":
            target = self.nullspace_target if self.nullspace_target is not None else torch.zeros(self.N, len(ids), dtype=self.dtype)
            qdd = (self.null_kp * (target - s["joint_pos"][:, ids]) + self.null_kd * (-s["joint_vel"][:, ids])).unsqueeze(-1)
            tau = tau + (M @ qdd - jt @ lam(jac @ qdd)).squeeze(-1)
        self.joint_efforts = tau
        return tau
