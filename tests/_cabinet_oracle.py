"""The manipulation/cabinet/mdp terms (isaaclab_tasks .../manipulation/cabinet/mdp: observations.py:27-59, rewards.py:18-162) and the
FrameTransformer's update (isaaclab/sensors/frame_transformer/frame_transformer.py:337-384) restated in torch, step by step in the
reference's operation order and in whatever dtype the inputs come: on the fp32 tensors they reproduce the reference's values, on their
float64 copies they are the statement the kernels are measured against.  The helpers restate utils/math.py: quat_mul :464-500, quat_apply
:546-566, quat_inv :239-248, normalize :82-92, combine_frame_transforms :750-781, subtract_frame_transforms :785-816, matrix_from_quat
:144-174, quat_unique :448-461.

A frame is ``(body_id, offset position (3,), offset rotation (4,) w x y z)``; a sensor ``(source frame, [target frames])`` -- what
``frames_of`` makes of a ``robots.FrameTable``."""

from __future__ import annotations

import torch


def quat_mul(q1: torch.Tensor, q2: torch.Tensor) -> torch.Tensor:
    w1, x1, y1, z1 = q1.unbind(-1)
    w2, x2, y2, z2 = q2.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                        qq - zz + (z1 + y1) * (w2 - x2)], dim=-1)


def quat_apply(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    xyz, w = q[..., 1:], q[..., :1]
    t = torch.linalg.cross(xyz, v) * 2
    return v + w * t + torch.linalg.cross(xyz, t)


def quat_inv(q: torch.Tensor) -> torch.Tensor:
    c = torch.cat([q[..., :1], -q[..., 1:]], dim=-1)
    return c / c.norm(p=2, dim=-1, keepdim=True).clamp(min=1.0e-9)


def quat_unique(q: torch.Tensor) -> torch.Tensor:
    return torch.where(q[..., 0:1] < 0, -q, q)


def combine_frame_transforms(t01, q01, t12, q12):
    return t01 + quat_apply(q01, t12), quat_mul(q01, q12)


def subtract_frame_transforms(t01, q01, t02, q02):
    q10 = quat_inv(q01)
    return quat_apply(q10, t02 - t01), quat_mul(q10, q02)


def matrix_from_quat(q: torch.Tensor) -> torch.Tensor:
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return o.reshape(q.shape[:-1] + (3, 3))


def frames_of(table) -> tuple:
    """``(source, targets)`` of a ``robots.FrameTable``."""
    as_frame = lambda f: (f.body_id, tuple(f.pos), tuple(f.rot))  # noqa: E731
    return as_frame(table.source), [as_frame(f) for f in table.targets]


def frame_pose(frame, body_pos_w: torch.Tensor, body_quat_w: torch.Tensor):
    """combine_frame_transforms(body pose, offset) of one frame: (N, 3), (N, 4)."""
    b, pos, rot = frame
    N, kw = body_pos_w.shape[0], dict(dtype=body_pos_w.dtype, device=body_pos_w.device)
    return combine_frame_transforms(body_pos_w[:, b], body_quat_w[:, b], torch.tensor(pos, **kw).expand(N, 3), torch.tensor(rot, **kw).expand(N, 4))


def frame_transformer(sensor, body_pos_w: torch.Tensor, body_quat_w: torch.Tensor) -> dict:
    """The six ``FrameTransformerData`` tensors of ``sensor`` on the body poses of the articulation its frames sit on."""
    source, targets = sensor
    sp, sq = frame_pose(source, body_pos_w, body_quat_w)
    tp, tq = (torch.stack(x, dim=1) for x in zip(*[frame_pose(f, body_pos_w, body_quat_w) for f in targets]))
    T = len(targets)
    rp, rq = subtract_frame_transforms(sp.unsqueeze(1).expand(-1, T, -1), sq.unsqueeze(1).expand(-1, T, -1), tp, tq)
    return {"source_pos_w": sp, "source_quat_w": sq, "target_pos_w": tp, "target_quat_w": tq, "target_pos_source": rp, "target_quat_source": rq}


def terms(s: dict, ee, cabinet, drawer_joint: int, gripper_joints, threshold=0.2, grasp_threshold=0.03, offset=0.04, open_joint_pos=0.04,
          cabinet_defaults=(0.0, 0.0)) -> dict:
    """Every cabinet term's raw value from the tensors ``s`` -- the robot's ``body_pos_w`` / ``body_quat_w`` / ``joint_pos``, the second
    articulation's ``articulation_*`` tensors, ``env_origins`` -- in their dtype.  ``ee`` / ``cabinet``: the two sensors (``frames_of``);
    the scalars are compared in the tensors' dtype (torch compares a float32 tensor with a Python number in float32).
    ``cabinet_defaults``: default position and velocity of the drawer joint."""
    E = frame_transformer(ee, s["body_pos_w"], s["body_quat_w"])
    C = frame_transformer(cabinet, s["articulation_body_pos_w"], s["articulation_body_quat_w"])
    dt = s["body_pos_w"].dtype
    c = lambda x: torch.tensor(x, dtype=torch.float32).to(dt)  # noqa: E731  (the fp32 rounding of the scalar, in either dtype)
    tcp, tcp_q, handle, handle_q = E["target_pos_w"][:, 0], E["target_quat_w"][:, 0], C["target_pos_w"][:, 0], C["target_quat_w"][:, 0]
    lf, rf = E["target_pos_w"][:, 1], E["target_pos_w"][:, 2]
    distance = torch.norm(handle - tcp, dim=-1, p=2)
    r = 1.0 / (1.0 + distance ** 2)
    r = torch.pow(r, 2)
    hm, em = matrix_from_quat(handle_q), matrix_from_quat(tcp_q)
    align_z = torch.bmm(em[..., 2].unsqueeze(1), -hm[..., 0].unsqueeze(-1)).squeeze(-1).squeeze(-1)
    align_x = torch.bmm(em[..., 0].unsqueeze(1), -hm[..., 1].unsqueeze(-1)).squeeze(-1).squeeze(-1)
    graspable = (rf[:, 2] < handle[:, 2]) & (lf[:, 2] > handle[:, 2])
    g = graspable.to(dt)
    lfd, rfd = torch.abs(lf[:, 2] - handle[:, 2]), torch.abs(rf[:, 2] - handle[:, 2])
    drawer = s["articulation_joint_pos"][:, drawer_joint]
    return {
        "distance": distance, "align_z": align_z, "align_x": align_x, "drawer": drawer, "is_graspable": graspable,
        "finger_gaps": torch.stack([lf[:, 2] - handle[:, 2], rf[:, 2] - handle[:, 2]], dim=-1),
        "approach_ee_handle": torch.where(distance <= c(threshold), 2 * r, r),
        "align_ee_handle": 0.5 * (torch.sign(align_z) * align_z ** 2 + torch.sign(align_x) * align_x ** 2),
        "align_grasp_around_handle": g,
        "approach_gripper_handle": g * ((c(offset) - lfd) + (c(offset) - rfd)),
        "grasp_handle": (distance <= c(grasp_threshold)).to(dt) * torch.sum(c(open_joint_pos) - s["joint_pos"][:, list(gripper_joints)], dim=-1),
        "open_drawer_bonus": (g + 1.0) * drawer,
        "multi_stage_open_drawer": (drawer > c(0.01)).to(dt) * 0.5 + (drawer > c(0.2)).to(dt) * g + (drawer > c(0.3)).to(dt) * g,
        "rel_ee_drawer_distance": handle - tcp,
        "ee_pos": tcp - s["env_origins"],
        "ee_quat": tcp_q,
        "fingertips_pos": (E["target_pos_w"][:, 1:] - s["env_origins"].unsqueeze(1)).reshape(tcp.shape[0], -1),
        "cabinet_joint_pos": s["articulation_joint_pos"][:, drawer_joint:drawer_joint + 1] - c(cabinet_defaults[0]),
        "cabinet_joint_vel": s["articulation_joint_vel"][:, drawer_joint:drawer_joint + 1] - c(cabinet_defaults[1]),
    }
