"""fp64 statements of the manipulation/reach/mdp reward terms (isaaclab_tasks .../manipulation/reach/mdp/rewards.py) and a feed tweak that
takes each of their branches -- shared by tests/test_reach_plan.py and tests/test_reach_gpu.py.  The formulas restate the reference's
utils/math.py helpers (quat_apply :546-566, quat_mul :464-500, quat_conjugate :224-236, axis_angle_from_quat :646-675,
quat_error_magnitude :678-690, combine_frame_transforms :750-786) in float64 on the fp32 inputs."""

from __future__ import annotations

import math

import torch

TASKS = {  # task -> (robot name, end-effector body, D, A, the cfg's fixed command pitch)
    "Isaac-Reach-Franka-v0": ("franka_panda", "panda_hand", 32, 7, math.pi),
    "Isaac-Reach-UR10-v0": ("ur10", "ee_link", 25, 6, math.pi / 2),
}
REACH = "isaaclab_tasks.manager_based.manipulation.reach.mdp.rewards"


def quat_apply(q, v):
    xyz = q[..., 1:]
    t = torch.cross(xyz, v, dim=-1) * 2.0
    return v + q[..., :1] * t + torch.cross(xyz, t, dim=-1)


def quat_mul(a, b):
    """The Hamilton product (w, x, y, z): the reference's eight-product form is the same function."""
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def conj(q):
    return torch.cat([q[..., :1], -q[..., 1:]], dim=-1)


def quat_error_magnitude(q1, q2):
    """||axis_angle_from_quat(q1 * conj(q2))|| with the reference's w < 0 flip and |angle| <= 1e-6 Taylor branch."""
    d = quat_mul(q1, conj(q2))
    d = d * (1.0 - 2.0 * (d[..., :1] < 0.0).to(d.dtype))
    mag = d[..., 1:].norm(dim=-1)
    half = torch.atan2(mag, d[..., 0])
    angle = 2.0 * half
    s = torch.where(angle.abs() > 1.0e-6, torch.sin(half) / angle, 0.5 - angle * angle / 48.0)
    return (d[..., 1:] / s[..., None]).norm(dim=-1)


def reach_terms(s: dict, b: int, std: float) -> dict:
    """The three reach rewards' raw values in fp64 from the feed tensors ``s`` (current snapshot) for end-effector body ``b``."""
    d = lambda n: s[n].double()  # noqa: E731
    rp, rq, cmd = d("root_pos_w"), d("root_quat_w"), d("command")
    des_p = rp + quat_apply(rq, cmd[:, :3])
    dist = (d("body_pos_w")[:, b] - des_p).norm(dim=-1)
    des_q = quat_mul(rq, cmd[:, 3:7])
    return {"position_command_error": dist, "position_command_error_tanh": 1.0 - torch.tanh(dist / std),
            "orientation_command_error": quat_error_magnitude(d("body_quat_w")[:, b], des_q)}


def position_rounding(s: dict, b: int) -> torch.Tensor:
    """Per-env allowance for the fp32 rounding of des_pos_w = root_pos_w + R cmd (and of body - des) at world coordinates far from the
    origin: two roundings of the largest coordinate involved, which the fp32 reference has as well (an env 400 m out rounds at 3e-5 m)."""
    big = torch.maximum(s["root_pos_w"].double().abs().amax(-1), s["body_pos_w"][:, b].double().abs().amax(-1)) + 1.0
    return 2.0 * big * 2.0 ** -24 * 2.0


def _quat_from_euler_xyz(roll, pitch, yaw):
    """utils/math.py:252-277 in fp32 (torch's own cos / sin, the reference's products)."""
    cy, sy = torch.cos(yaw * 0.5), torch.sin(yaw * 0.5)
    cr, sr = torch.cos(roll * 0.5), torch.sin(roll * 0.5)
    cp, sp = torch.cos(pitch * 0.5), torch.sin(pitch * 0.5)
    return torch.stack([cy * cr * cp + sy * sr * sp, cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp], -1)


def _quat_from_angle_axis(angle, axis):
    h = angle[:, None] * 0.5
    return torch.cat([torch.cos(h), axis * torch.sin(h)], dim=-1)


def reach_tweak(feed, b: int, pitch: float, gen: torch.Generator) -> None:
    """Every branch of the reach terms on a random feed (all snapshots; the same cases as tools/gen_golden_reach.py): the cfg's own
    command orientation on even envs (pitch pi: w ~ -4.4e-8 cos(yaw / 2), either sign), the end effector at 0, std / 2, std, 2 std or
    U(0, 0.5) m from its target, and its orientation equal to the target (Taylor branch), negated (w < 0), turned by pi - 1e-3, pi or
    1e-3, or the feed's random quaternion."""
    st, N = feed._stack, feed.num_envs
    dev = st["command"].device
    idx = torch.arange(N)
    for k in range(feed.num_snapshots):
        cmd = st["command"][k]
        yaw = (torch.rand(N, generator=gen) * 2.0 - 1.0) * 3.14
        q = _quat_from_euler_xyz(torch.zeros(N), torch.full((N,), pitch), yaw).to(dev)
        even = (idx % 2 == 0).to(dev)
        cmd[even, 3:7] = q[even]
        rp, rq = st["root_pos_w"][k], st["root_quat_w"][k]
        des_p = (rp.double() + quat_apply(rq.double(), cmd[:, :3].double())).float()
        des_q = quat_mul(rq.double(), cmd[:, 3:7].double())
        dirn = torch.randn(N, 3, generator=gen)
        dirn = dirn / dirn.norm(dim=-1, keepdim=True)
        d = torch.rand(N, generator=gen) * 0.5
        for m, v in ((0, 0.0), (1, 0.05), (2, 0.1), (3, 0.2)):
            d[idx % 6 == m] = v
        st["body_pos_w"][k][:, b] = des_p + (dirn * d[:, None]).to(dev)
        axis = torch.randn(N, 3, generator=gen, dtype=torch.float64)
        axis = axis / axis.norm(dim=-1, keepdim=True)
        m8 = idx % 8
        ang = torch.full((N,), 1.0e-3, dtype=torch.float64)
        ang[m8 == 2] = math.pi - 1.0e-3
        ang[m8 == 3] = math.pi
        turned = quat_mul(des_q, _quat_from_angle_axis(ang, axis).to(dev))
        bq = st["body_quat_w"][k][:, b].clone()
        m8 = m8.to(dev)
        bq[m8 == 0] = des_q[m8 == 0].float()
        bq[m8 == 1] = -des_q[m8 == 1].float()
        sel = (m8 >= 2) & (m8 <= 4)
        bq[sel] = turned[sel].float()
        st["body_quat_w"][k][:, b] = bq
