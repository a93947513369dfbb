"""TEST INFRASTRUCTURE -- a torch restatement of ``DifferentialInverseKinematicsAction`` (reference
``isaaclab/envs/mdp/actions/task_space_actions.py:30-229``) with ``DifferentialIKController`` (``controllers/differential_ik.py:98-240``)
and the ``utils/math.py`` helpers they call, written for this repository.  It works in the dtype of the tensors it is given (fp32 in the
tests).  Two deliberate departures, the same as the kernel's: the damped least-squares step solves ``(J J^T + lambda^2 I) z = dx``
instead of forming the inverse, and the global ``ee_quat_curr.norm() != 0`` test (:173) is not made.

The term is a ``plan.IkTerm`` (``resolve_ik_term``).
"""

from __future__ import annotations

import torch


def quat_mul(a, b):  # utils/math.py:464-500
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                        qq - zz + (z1 + y1) * (w2 - x2)], dim=-1)


def quat_apply(q, v):  # :545-564
    xyz = q[:, 1:]
    t = torch.linalg.cross(xyz, v, dim=-1) * 2
    return v + q[:, 0:1] * t + torch.linalg.cross(xyz, t, dim=-1)


def normalize(x, eps=1.0e-9):  # :82-92
    return x / x.norm(dim=-1, keepdim=True).clamp(min=eps)


def quat_conjugate(q):
    return torch.cat([q[:, 0:1], -q[:, 1:]], dim=-1)


def matrix_from_quat(q):  # :144-174
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return o.reshape(q.shape[:-1] + (3, 3))


def axis_angle_from_quat(q, eps=1.0e-6):  # :646-675
    q = q * (1.0 - 2.0 * (q[:, 0:1] < 0.0))
    mag = q[:, 1:].norm(dim=-1)
    half = torch.atan2(mag, q[:, 0])
    angle = 2.0 * half
    s = torch.where(angle.abs() > eps, torch.sin(half) / angle, 0.5 - angle * angle / 48)
    return q[:, 1:4] / s.unsqueeze(-1)


def apply_delta_pose(pos, rot, delta, eps=1.0e-6):  # :873-910
    target_pos = pos + delta[:, 0:3]
    r = delta[:, 3:6]
    angle = r.norm(dim=-1)
    axis = r / angle.unsqueeze(-1)
    theta = (angle / 2).unsqueeze(-1)
    dq = normalize(torch.cat([theta.cos(), normalize(axis) * theta.sin()], dim=-1))  # quat_from_angle_axis :629-642
    ident = torch.zeros_like(dq)
    ident[:, 0] = 1.0
    dq = torch.where(angle.unsqueeze(-1) > eps, dq, ident)
    return target_pos, quat_mul(dq, rot)


class DiffIKOracle:
    def __init__(self, ik, num_envs: int, dtype=torch.float32):
        self.ik, self.N, self.dtype = ik, num_envs, dtype
        n = len(ik.joint_ids)
        self.raw_actions = torch.zeros(num_envs, ik.width, dtype=dtype)
        self.processed_actions = torch.zeros(num_envs, ik.width, dtype=dtype)
        self.ee_pos_des = torch.zeros(num_envs, 3, dtype=dtype)
        self.ee_quat_des = torch.zeros(num_envs, 4, dtype=dtype)
        self.joint_pos_des = torch.zeros(num_envs, n, dtype=dtype)
        self.scale = torch.tensor(ik.scale, dtype=dtype)
        self.clip = None if ik.clip is None else torch.tensor(ik.clip, dtype=dtype)
        self.offset_pos = None if ik.offset_pos is None else torch.tensor(ik.offset_pos, dtype=dtype).repeat(num_envs, 1)
        self.offset_rot = None if ik.offset_rot is None else torch.tensor(ik.offset_rot, dtype=dtype).repeat(num_envs, 1)

    def reset(self, env_ids):  # :181-182
        self.raw_actions[env_ids] = 0.0

    def frame_pose(self, s):  # _compute_frame_pose :188-207
        b = self.ik.body_idx
        q10 = normalize(quat_conjugate(s["root_quat_w"]))  # subtract_frame_transforms (utils/math.py:785-816)
        quat = quat_mul(q10, s["body_quat_w"][:, b])
        pos = quat_apply(q10, s["body_pos_w"][:, b] - s["root_pos_w"])
        if self.offset_pos is not None:  # combine_frame_transforms (:750-781)
            pos, quat = pos + quat_apply(quat, self.offset_pos), quat_mul(quat, self.offset_rot)
        return pos, quat

    def process_actions(self, raw):  # :155-158
        self.raw_actions[:] = raw
        p = self.raw_actions * self.scale
        if self.clip is not None:
            p = torch.clamp(p, min=self.clip[:, 0], max=self.clip[:, 1])
        self.processed_actions = p

    def set_command(self, s):  # the command half of process_actions :163-166, differential_ik.py:98-146
        ik, cmd = self.ik, self.processed_actions
        pos, quat = self.frame_pose(s)
        if ik.command_type == "position":
            self.ee_pos_des = pos + cmd if ik.use_relative_mode else cmd.clone()
            self.ee_quat_des = quat
        elif ik.use_relative_mode:
            self.ee_pos_des, self.ee_quat_des = apply_delta_pose(pos, quat, cmd)
        else:
            self.ee_pos_des, self.ee_quat_des = cmd[:, 0:3].clone(), cmd[:, 3:7].clone()

    def frame_jacobian(self, s):  # jacobian_b :142-149, _compute_frame_jacobian :209-229
        ik = self.ik
        jac = s["jacobians"][:, ik.jacobi_body_idx][:, :, ik.jacobi_joint_ids].clone()
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

    def apply_actions(self, s):  # :168-179, differential_ik.py:148-240
        ik = self.ik
        pos, quat = self.frame_pose(s)
        jac = self.frame_jacobian(s)
        if ik.command_type == "position":
            dx, jac = self.ee_pos_des - pos, jac[:, 0:3]
        else:  # compute_pose_error (utils/math.py:820-867)
            conj = quat_conjugate(quat)
            inv = conj / quat_mul(quat, conj)[:, 0:1]
            dx = torch.cat([self.ee_pos_des - pos, axis_angle_from_quat(quat_mul(self.ee_quat_des, inv))], dim=1)
        jt = jac.transpose(1, 2)
        if ik.ik_method == "trans":
            dq = (ik.k_val * jt @ dx.unsqueeze(-1)).squeeze(-1)
        else:
            A = jac @ jt + (ik.lambda_val ** 2) * torch.eye(jac.shape[1], dtype=self.dtype)
            dq = (jt @ torch.linalg.solve(A, dx.unsqueeze(-1))).squeeze(-1)
        self.joint_pos_des = s["joint_pos"][:, ik.joint_ids] + dq
        return self.joint_pos_des
