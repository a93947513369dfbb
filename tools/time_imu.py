"""Time the Imu refresh two ways at 4096 envs.

    python tools/time_imu.py [--envs 4096] [--launches 200] [--rounds 5] [--out profiles/imu_timing.txt]

  (a) the reference's torch op sequence of ``Imu._update_buffers_impl`` (isaaclab/sensors/imu/imu.py:141-181) with every env outdated --
      the XYZW split and conversion, quat_rotate, quat_mul, the cross product, both derivatives, four quat_rotate_inverse and the
      indexed stores -- on the same device tensors;
  (b) the one launch of ``producers.Imu`` (``imx_imu``), a refresh of all envs (update_period 0, force_recompute).
The outputs are compared first (largest absolute difference per tensor).  HIP events around ``launches`` back-to-back calls after a
warm-up, ``rounds`` alternated rounds; both series, their spread and the ratio of medians.  Recorded values, not a target."""

from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaaclab_amd.producers import Imu  # noqa: E402

OFFSET_POS, OFFSET_ROT, BIAS, DT = (0.05, -0.02, 0.1), (0.9238795, 0.0, 0.3826834, 0.0), (0.0, 0.0, 9.81), 0.005


def quat_rotate(q, v, sign=1.0):  # isaaclab/utils/math.py:583-625
    q_w, q_vec = q[:, 0], q[:, 1:]
    a = v * (2.0 * q_w ** 2 - 1.0).unsqueeze(-1)
    b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
    c = q_vec * torch.bmm(q_vec.view(q.shape[0], 1, 3), v.view(q.shape[0], 3, 1)).squeeze(-1) * 2.0
    return a + sign * b + c


def quat_mul(q1, q2):  # :464-500
    w1, x1, y1, z1 = q1[:, 0], q1[:, 1], q1[:, 2], q1[:, 3]
    w2, x2, y2, z2 = q2[:, 0], q2[:, 1], q2[:, 2], q2[:, 3]
    ww, yy, zz = (z1 + x1) * (x2 + y2), (w1 - y1) * (w2 + z2), (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                        qq - zz + (z1 + y1) * (w2 - x2)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, dev = a.envs, torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    pos = torch.randn(N, 3, generator=g)
    quat = torch.randn(N, 4, generator=g)
    quat = quat / quat.norm(dim=1, keepdim=True)
    lin, ang = torch.randn(N, 3, generator=g) * 0.5, torch.randn(N, 3, generator=g)
    pos, quat, lin, ang = (t.to(dev).contiguous() for t in (pos, quat, lin, ang))
    transforms = torch.cat([pos, quat[:, 1:], quat[:, :1]], dim=-1).contiguous()  # what the PhysX view returns: XYZW
    velocities = torch.cat([lin, ang], dim=-1).contiguous()
    coms = torch.zeros(N, 7, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    d = {k: z(N, 3) for k in ("pos_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b", "prev_v", "prev_w")}
    d["quat_w"] = z(N, 4)
    off_p = torch.tensor(OFFSET_POS, device=dev).repeat(N, 1)
    off_q = torch.tensor(OFFSET_ROT, device=dev).repeat(N, 1)
    bias = torch.tensor(BIAS, device=dev).repeat(N, 1)
    ids = slice(None)

    def old():
        p, q = transforms[ids].split([3, 4], dim=-1)
        q = q.roll(1, dims=-1)  # convert_quat(to="wxyz")
        d["pos_w"][ids] = p + quat_rotate(q, off_p[ids])
        d["quat_w"][ids] = quat_mul(q, off_q[ids])
        com = coms.split([3, 4], dim=-1)[0]
        v, w = velocities.clone()[ids].split([3, 3], dim=-1)  # (get_velocities returns a fresh tensor)
        v += torch.linalg.cross(w, quat_rotate(q, off_p[ids] - com[ids]), dim=-1)
        la = (v - d["prev_v"][ids]) / DT + bias[ids]
        aa = (w - d["prev_w"][ids]) / DT
        d["lin_vel_b"][ids] = quat_rotate(d["quat_w"][ids], v, -1.0)
        d["ang_vel_b"][ids] = quat_rotate(d["quat_w"][ids], w, -1.0)
        d["lin_acc_b"][ids] = quat_rotate(d["quat_w"][ids], la, -1.0)
        d["ang_acc_b"][ids] = quat_rotate(d["quat_w"][ids], aa, -1.0)
        d["prev_v"][ids] = v
        d["prev_w"][ids] = w

    s = Imu({"offset": {"pos": OFFSET_POS, "rot": OFFSET_ROT}, "gravity_bias": BIAS, "update_period": 0.0}, N, dev)

    def new():
        s.update(DT, pos, quat, lin, ang, force_recompute=True)  # update_period 0: every env is outdated at every update

    old()
    new()
    torch.cuda.synchronize()
    lines = [f"{N} envs, every env refreshed; {a.launches} calls per sample, {a.rounds} alternated rounds; device {torch.cuda.get_device_name(0)}"]
    lines.append("first call, max |(a) - (b)|: " + ", ".join(f"{k} {float((d[k] - getattr(s._data, k)).abs().max()):.2e}"
                                                              for k in ("pos_w", "quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b")))
    series = {"a": [], "b": []}
    for fn in (old, new):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for key, fn in (("a", old), ("b", new)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            series[key].append(e0.elapsed_time(e1) * 1000.0 / a.launches)
    for key, what in (("a", "(a) the reference's torch op sequence"), ("b", "(b) imx_imu")):
        x = series[key]
        lines.append(f"  {what}: us per call {[round(u, 1) for u in x]}  min {min(x):.1f} median {statistics.median(x):.1f} max {max(x):.1f}")
    lines.append(f"  ratio of medians (a) / (b): {statistics.median(series['a']) / statistics.median(series['b']):.2f} (both include the host's launch work: "
                 "back-to-back calls from Python)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
