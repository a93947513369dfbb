"""The Imu sensor restated in torch, parameterised on dtype: ``SensorBase`` (isaaclab/sensors/sensor_base.py:182-205,287-296) around
``Imu.reset`` / ``update`` / ``_update_buffers_impl`` (isaaclab/sensors/imu/imu.py:92-181), with the formulas of ``isaaclab.utils.math``
(quat_rotate / quat_rotate_inverse :583-625, quat_mul :464-500) written out.  The clocks are ALWAYS fp32, sequential additions, as in
the reference -- so the fp64 oracle refreshes exactly the envs the fp32 one does; only the float tensors follow ``dtype``.

Also the fixture's loader and replay (``tests/golden/imu_sensor.json``, written by tools/gen_golden_imu.py from the real class) and the
tolerance rule the tests share."""

from __future__ import annotations

import json
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSOR_JSON = os.path.join(ROOT, "tests", "golden", "imu_sensor.json")
TASK_JSON = os.path.join(ROOT, "tests", "golden", "Isaac-Velocity-Flat-Anymal-C-v0-imu.json")
DATA = ("pos_w", "quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b")
PREV = ("prev_lin_vel_w", "prev_ang_vel_w")
CLOCKS = ("timestamp", "timestamp_last_update", "is_outdated")


def quat_rotate(q, v, sign=1.0):
    """quat_rotate (sign +1) / quat_rotate_inverse (sign -1): a +- b + c."""
    w, xyz = q[:, 0:1], q[:, 1:]
    a = v * (2.0 * w * w - 1.0)
    b = torch.linalg.cross(xyz, v, dim=-1) * w * 2.0
    c = xyz * (xyz * v).sum(-1, keepdim=True) * 2.0
    return a + sign * b + c


def quat_mul(q1, q2):
    w1, x1, y1, z1 = q1.unbind(-1)
    w2, x2, y2, z2 = q2.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                        qq - zz + (z1 + y1) * (w2 - x2)], dim=-1)


class ImuOracle:
    def __init__(self, num_envs, offset_pos=(0.0, 0.0, 0.0), offset_rot=(1.0, 0.0, 0.0, 0.0), gravity_bias=(0.0, 0.0, 9.81),
                 update_period=0.0, history_length=0, com_pos_b=None, dtype=torch.float64):
        N, self.dtype = int(num_envs), dtype
        self.N = N
        t = lambda v: torch.tensor(list(v), dtype=torch.float32).to(dtype)  # noqa: E731  (the cfg values are fp32 in the reference)
        self.offset_pos, self.offset_rot, self.gravity_bias = t(offset_pos).repeat(N, 1), t(offset_rot).repeat(N, 1), t(gravity_bias).repeat(N, 1)
        self.update_period, self.history_length = float(update_period), int(history_length)
        com = torch.zeros(N, 3) if com_pos_b is None else torch.as_tensor(com_pos_b, dtype=torch.float32)
        self.com_pos_b = (com.repeat(N, 1) if com.dim() == 1 else com).to(dtype)
        z = lambda *s: torch.zeros(*s, dtype=dtype)  # noqa: E731
        self.data_ = types.SimpleNamespace(pos_w=z(N, 3), quat_w=z(N, 4), lin_vel_b=z(N, 3), ang_vel_b=z(N, 3), lin_acc_b=z(N, 3), ang_acc_b=z(N, 3))
        self.data_.quat_w[:, 0] = 1.0
        self.prev_lin_vel_w, self.prev_ang_vel_w = z(N, 3), z(N, 3)
        self.timestamp, self.timestamp_last_update = torch.zeros(N), torch.zeros(N)
        self.is_outdated = torch.ones(N, dtype=torch.bool)
        self.dt = None
        self.inputs = None

    def reset(self, env_ids=None):
        ids = slice(None) if env_ids is None else env_ids
        self.timestamp[ids] = 0.0
        self.timestamp_last_update[ids] = 0.0
        self.is_outdated[ids] = True
        for f in ("quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b"):
            getattr(self.data_, f)[ids] = 0.0

    def update(self, dt, pos_w, quat_w, lin_vel_w, ang_vel_w, force_recompute=False, substeps=1):
        self.inputs = tuple(torch.as_tensor(t).detach().cpu().to(self.dtype) for t in (pos_w, quat_w, lin_vel_w, ang_vel_w))
        self.dt = float(dt)
        for _ in range(int(substeps)):
            self.timestamp += self.dt  # fp32 tensor += python float
            self.is_outdated |= self.timestamp - self.timestamp_last_update + 1e-6 >= self.update_period
        if force_recompute or self.history_length > 0:
            self._refresh()

    def _refresh(self):
        ids = self.is_outdated.nonzero().squeeze(-1)
        if len(ids) > 0:
            if self.dt is None:
                raise RuntimeError("The update function must be called before the data buffers are accessed the first time.")
            p, q, v, w = (t[ids] for t in self.inputs)
            d = self.data_
            d.pos_w[ids] = p + quat_rotate(q, self.offset_pos[ids])
            d.quat_w[ids] = quat_mul(q, self.offset_rot[ids])
            v = v + torch.linalg.cross(w, quat_rotate(q, self.offset_pos[ids] - self.com_pos_b[ids]), dim=-1)
            lin_acc = (v - self.prev_lin_vel_w[ids]) / self.dt + self.gravity_bias[ids]
            ang_acc = (w - self.prev_ang_vel_w[ids]) / self.dt
            qs = d.quat_w[ids]
            d.lin_vel_b[ids], d.ang_vel_b[ids] = quat_rotate(qs, v, -1.0), quat_rotate(qs, w, -1.0)
            d.lin_acc_b[ids], d.ang_acc_b[ids] = quat_rotate(qs, lin_acc, -1.0), quat_rotate(qs, ang_acc, -1.0)
            self.prev_lin_vel_w[ids], self.prev_ang_vel_w[ids] = v, w
            self.timestamp_last_update[ids] = self.timestamp[ids]
            self.is_outdated[ids] = False

    @property
    def data(self):
        self._refresh()
        return self.data_

    def state(self) -> dict:
        s = {f: getattr(self.data_, f).clone() for f in DATA}
        s.update(prev_lin_vel_w=self.prev_lin_vel_w.clone(), prev_ang_vel_w=self.prev_ang_vel_w.clone(), timestamp=self.timestamp.clone(),
                 timestamp_last_update=self.timestamp_last_update.clone(), is_outdated=self.is_outdated.clone())
        return s


# ------------------------------------------------------------------------------------------------- the fixture
def load_fixture(path=SENSOR_JSON) -> dict:
    with open(path) as f:
        return json.load(f)


def f32(x):
    return torch.tensor(np.asarray(x, dtype=np.float64).astype(np.float32))


def make_oracles(fx, dtype) -> dict:
    com = f32(fx["com_pos_b"])
    return {name: ImuOracle(fx["N"], c["offset_pos"], c["offset_rot"], c["gravity_bias"], c["update_period"], com_pos_b=com, dtype=dtype)
            for name, c in fx["sensors"].items()}


def replay(fx, sensors: dict, state_of):
    """Drive ``sensors`` (name -> an object with reset / update / data of the producer's signature) through the fixture's calls; yields
    (call index, call, {name: state}) after every call that records a state.  ``state_of(sensor)`` -> dict of CPU tensors."""
    inputs = None
    for k, call in enumerate(fx["calls"]):
        op = call["op"]
        if op == "inputs":
            inputs = call
            continue
        for s in sensors.values():
            if op == "update":
                s.update(call["dt"], *(inputs["_t"][n] for n in ("pos_w", "quat_w", "lin_vel_w", "ang_vel_w")),
                         force_recompute=bool(call.get("force_recompute", False)))
            elif op == "reset":
                s.reset(call["env_ids"])
            elif op == "data":
                s.data
            else:
                raise ValueError(op)
        yield k, call, {name: state_of(s) for name, s in sensors.items()}


def with_input_tensors(fx, to_tensor):
    """``call['_t'][name]``: the inputs of every "inputs" call as tensors made by ``to_tensor`` (once: the replay keeps them by reference)."""
    for call in fx["calls"]:
        if call["op"] == "inputs":
            call["_t"] = {n: to_tensor(f32(call[n])) for n in ("pos_w", "quat_w", "lin_vel_w", "ang_vel_w")}
    return fx


# ------------------------------------------------------------------------------------------------- the tolerance
def bound(reference32: torch.Tensor, oracle64: torch.Tensor) -> float:
    """4 x the largest deviation of the REFERENCE's fp32 result from the fp64 oracle on the same inputs (the factor covers another valid
    operation order and FMA contraction; the accelerations amplify velocity rounding by 1 / dt), floored at one fp32 ulp of the tensor's
    largest magnitude.  Never computed from the output under test."""
    dev = float((reference32.double() - oracle64.double()).abs().max())
    mag = float(oracle64.abs().max())
    ulp = float(np.spacing(np.float32(mag))) if mag > 0 else float(np.finfo(np.float32).tiny)
    return max(4.0 * dev, ulp)


def recorded(call, name, field):
    v = call["state"][name][field]
    return torch.tensor(v, dtype=torch.bool) if field == "is_outdated" else f32(v)


def check_against_fixture(fx, oracle64_states, states, who):
    """``states``: {call index: {sensor: {field: tensor}}} of the thing under test.  Clocks and flags bit for bit; every float tensor
    within 4 x the recorded reference's own deviation from the fp64 oracle (floor: one fp32 ulp), per call and tensor."""
    worst = {}
    for k, call in enumerate(fx["calls"]):
        if call["op"] == "inputs":
            continue
        for name in fx["sensors"]:
            got, ref64 = states[k][name], oracle64_states[k][name]
            for f in CLOCKS:
                assert torch.equal(got[f].cpu(), recorded(call, name, f)), f"{who}: call {k} ({call['op']}) {name}.{f}"
            for f in DATA + PREV:
                if f not in call["state"][name]:  # (an update without force_recompute records the clocks and flags only)
                    continue
                ref32 = recorded(call, name, f)
                b = bound(ref32, ref64[f])
                err = float((got[f].cpu().double() - ref64[f]).abs().max())
                worst[f] = max(worst.get(f, (0.0, 0.0)), (err, b))
                assert err <= b, f"{who}: call {k} ({call['op']}) {name}.{f}: |x - fp64| = {err:.3e} > bound {b:.3e}"
    print(who, {f: f"{e:.2e} (bound {b:.2e})" for f, (e, b) in worst.items()})
