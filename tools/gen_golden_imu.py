"""TEST INFRASTRUCTURE (build container only): the fixtures of the Imu sensor, from the REAL reference.

    python tools/gen_golden_imu.py

Writes
  * ``tests/golden/Isaac-Velocity-Flat-Anymal-C-v0-imu.json`` and its ``.managers.json`` side file: the reference's flat Anymal-C cfg
    (``AnymalCFlatEnvCfg()`` / ``AnymalCFlatPPORunnerCfg()`` through ``oracle.gen_golden.dump_cfg``) plus two ``ImuCfg`` scene entries
    -- ``imu`` on ``base`` with the defaults, ``imu_foot`` on ``LF_FOOT`` with an offset, a rotated frame, no gravity bias and an update
    period of 2.5 physics steps -- the three imu_* terms on ``imu`` appended to the policy group (one with ``Unoise`` and a scale) and
    ``imu_lin_acc`` on ``imu_foot`` in a second group.  The side file carries the two scene entries (settings only) and the robot's
    init state.
  * ``tests/golden/imu_sensor.json``: the REAL ``Imu`` class -- an instance made without ``__init__``, its real
    ``_initialize_buffers_impl``, ``reset``, ``update`` and ``data`` -- over a fake rigid-body view that returns fresh XYZW transforms,
    COMs and velocities on every call.  Two sensors (the two cfgs above) see the same N = 6 bodies through 8 steps: update bursts of
    1..4 substeps, partial resets, one change of dt in the middle, a forced recompute, a non-zero ``com_pos_b`` for half of the envs.
    After every call the clocks and flags; after every call that can change them (reset, read, forced update) also every ``ImuData``
    tensor and the previous velocities.
Deterministic: a second run reproduces the files bit for bit."""

from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden as gg  # noqa: E402  (installs oracle.ref_import)

imu_mod = importlib.import_module("isaaclab.sensors.imu.imu")
from isaaclab.sensors.imu import ImuCfg  # noqa: E402

from isaaclab_amd.robots import ANYMAL_C  # noqa: E402

TASK = "Isaac-Velocity-Flat-Anymal-C-v0-imu"
N = 6
PHYSICS_DT = 0.005
FOOT_OFFSET_POS = (0.05, -0.02, 0.1)
FOOT_OFFSET_ROT = (0.9238795, 0.0, 0.3826834, 0.0)  # 45 degrees about y


def imu_cfgs():
    return {"imu": ImuCfg(prim_path="{ENV_REGEX_NS}/Robot/base"),
            "imu_foot": ImuCfg(prim_path="{ENV_REGEX_NS}/Robot/LF_FOOT", offset=ImuCfg.OffsetCfg(pos=FOOT_OFFSET_POS, rot=FOOT_OFFSET_ROT),
                               gravity_bias=(0.0, 0.0, 0.0), update_period=2.5 * PHYSICS_DT)}


# ------------------------------------------------------------------------------------------------- the task cfg
def task_fixture():
    from isaaclab.managers import ObservationGroupCfg as ObsGroup
    from isaaclab.managers import ObservationTermCfg as ObsTerm
    from isaaclab.managers import SceneEntityCfg
    from isaaclab.utils import configclass
    from isaaclab.utils.noise import AdditiveUniformNoiseCfg as Unoise

    import isaaclab.envs.mdp as mdp

    pkg = "isaaclab_tasks.manager_based.locomotion.velocity.config.anymal_c"
    env_cfg = importlib.import_module(f"{pkg}.flat_env_cfg").AnymalCFlatEnvCfg()
    agent_cfg = importlib.import_module(f"{pkg}.agents.rsl_rl_ppo_cfg").AnymalCFlatPPORunnerCfg()
    assert abs(env_cfg.sim.dt - PHYSICS_DT) < 1e-12
    for name, c in imu_cfgs().items():
        setattr(env_cfg.scene, name, c)
    pol = env_cfg.observations.policy
    pol.imu_orientation = ObsTerm(func=mdp.imu_orientation)
    pol.imu_ang_vel = ObsTerm(func=mdp.imu_ang_vel, noise=Unoise(n_min=-0.2, n_max=0.2), scale=0.25)
    pol.imu_lin_acc = ObsTerm(func=mdp.imu_lin_acc, params={"asset_cfg": SceneEntityCfg("imu")})

    @configclass
    class FootCfg(ObsGroup):
        foot_lin_acc = ObsTerm(func=mdp.imu_lin_acc, params={"asset_cfg": SceneEntityCfg("imu_foot")}, clip=(-500.0, 500.0))

        def __post_init__(self):
            self.enable_corruption = False
            self.concatenate_terms = True

    env_cfg.observations.foot = FootCfg()
    gg.CONFIGS = gg.GOLDEN  # dump_cfg writes the cfg fixture next to the golden files
    gg.dump_cfg(TASK, env_cfg, agent_cfg, ANYMAL_C)
    path = os.path.join(gg.GOLDEN, TASK + ".json")  # the same content without the indentation: one section per line
    with open(path) as f:
        fx = json.load(f)
    with open(path, "w") as f:
        f.write("{" + ",\n".join(f"{json.dumps(k)}:" + (json.dumps(v, separators=(",", ":")) if k != "env" else
                                 "{" + ",\n ".join(f"{json.dumps(a)}:{json.dumps(b, separators=(',', ':'))}" for a, b in v.items()) + "}")
                                 for k, v in fx.items()) + "}\n")
    base = env_cfg.to_dict()
    scene = {"robot": {"init_state": {k: list(v) for k, v in base["scene"]["robot"]["init_state"].items() if k in ("pos", "rot", "lin_vel", "ang_vel")}}}
    for name in imu_cfgs():
        scene[name] = {k: v for k, v in base["scene"][name].items() if k != "visualizer_cfg"}
    side = {"scene": scene}
    with open(os.path.join(gg.GOLDEN, TASK + ".managers.json"), "w") as f:
        json.dump(gg._jsonable(side), f, separators=(",", ":"))


# ------------------------------------------------------------------------------------------------- the sensor
class FakeView:
    """Stands in for the PhysX rigid-body view: fresh tensors on every call, transforms and COMs with XYZW quaternions."""

    def __init__(self, n, com):
        self.count = n
        self.com = com
        self.pos = self.quat = self.lin = self.ang = None

    def get_transforms(self):
        return torch.cat([self.pos, self.quat[:, 1:], self.quat[:, :1]], dim=-1)

    def get_coms(self):
        return torch.cat([self.com, torch.zeros(self.count, 3), torch.ones(self.count, 1)], dim=-1)

    def get_velocities(self):
        return torch.cat([self.lin, self.ang], dim=-1)


def make_sensor(cfg, view):
    s = imu_mod.Imu.__new__(imu_mod.Imu)
    s.cfg = cfg
    s._device, s._is_visualizing = "cpu", False
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # (SensorBase.__del__ reads them)
    s._view = view
    s._data = imu_mod.ImuData()
    n = view.count
    s._num_envs = n
    s._is_outdated = torch.ones(n, dtype=torch.bool)  # SensorBase._initialize_impl (sensor_base.py:226-231)
    s._timestamp = torch.zeros(n)
    s._timestamp_last_update = torch.zeros(n)
    s._initialize_buffers_impl()
    return s


def short(t: torch.Tensor):
    """An fp32 tensor as nested lists of the SHORTEST decimals that give the same fp32 back (a third of the 17-digit form's bytes)."""
    a = t.numpy()
    out = np.array([float(str(x)) for x in a.reshape(-1)], np.float64).reshape(a.shape)  # (str of an np.float32: its shortest form)
    assert np.array_equal(out.astype(np.float32), a)
    return out.tolist()


def state(s, full: bool) -> dict:
    """The clocks and flags; with ``full`` (a call that can change them) also every ``ImuData`` tensor and the previous velocities."""
    out = dict(timestamp=short(s._timestamp), timestamp_last_update=short(s._timestamp_last_update),
               is_outdated=[int(x) for x in s._is_outdated.tolist()])
    if full:
        out.update({f: short(getattr(s._data, f)) for f in ("pos_w", "quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b")})
        out.update(prev_lin_vel_w=short(s._prev_lin_vel_w), prev_ang_vel_w=short(s._prev_ang_vel_w))
    return out


def sensor_fixture():
    g = torch.Generator().manual_seed(77)
    com = torch.zeros(N, 3)
    com[: N // 2] = torch.rand(N // 2, 3, generator=g) * 0.1 - 0.05
    view = FakeView(N, com)
    cfgs = imu_cfgs()
    sensors = {name: make_sensor(c, view) for name, c in cfgs.items()}
    try:
        sensors["imu"].data
        raise AssertionError("data before update must raise")
    except RuntimeError as e:
        first_read_error = str(e)
    calls = []

    def record(op, **kw):
        full = op != "update" or kw.get("force_recompute")  # (an update without it moves the clocks and flags only)
        calls.append(dict(op=op, **kw, state={name: state(s, full) for name, s in sensors.items()}))

    # (burst of substeps, dt, force_recompute on the burst's last update, reset ids after the burst)
    steps = [(4, PHYSICS_DT, False, None), (1, PHYSICS_DT, False, [1, 4]), (2, PHYSICS_DT, False, None), (4, PHYSICS_DT, False, [0, 1, 5]),
             (2, 0.01, False, None), (1, 0.01, True, [2]), (3, 0.01, False, None), (4, PHYSICS_DT, False, [3])]
    vel = torch.randn(N, 3, generator=g) * 0.5
    ang = torch.randn(N, 3, generator=g)
    for burst, dt, force, reset_ids in steps:
        view.pos = torch.stack([torch.rand(N, generator=g) * 8 - 4, torch.rand(N, generator=g) * 8 - 4, torch.rand(N, generator=g) * 0.6 + 0.1], 1)
        q = torch.randn(N, 4, generator=g)
        view.quat = q / q.norm(dim=1, keepdim=True)
        vel = vel + torch.randn(N, 3, generator=g) * 0.05  # a velocity that changes by a plausible acceleration times dt
        ang = ang + torch.randn(N, 3, generator=g) * 0.1
        view.lin, view.ang = vel.clone(), ang.clone()
        calls.append(dict(op="inputs", pos_w=short(view.pos), quat_w=short(view.quat), lin_vel_w=short(view.lin), ang_vel_w=short(view.ang)))
        for k in range(burst):
            f = force and k == burst - 1
            for s in sensors.values():
                s.update(dt, force_recompute=f)
            record("update", dt=dt, force_recompute=f)
        if reset_ids is not None:
            assert float(vel[reset_ids].abs().min()) > 0.0  # reset while moving
            for s in sensors.values():
                s.reset(reset_ids)
            record("reset", env_ids=reset_ids)
        before = {name: s._is_outdated.clone() for name, s in sensors.items()}
        for s in sensors.values():
            s.data
        record("data", outdated_before={name: [int(x) for x in b.tolist()] for name, b in before.items()})
        assert torch.equal(view.lin, vel) and torch.equal(view.ang, ang)  # the in-place += landed in a copy
    mixed = [c for c in calls if c["op"] == "data" and 0 < sum(c["outdated_before"]["imu_foot"]) < N]
    assert mixed, "no read of imu_foot with some envs outdated and some not"
    print("imu_foot refreshes per read:", [sum(c["outdated_before"]["imu_foot"]) for c in calls if c["op"] == "data"])
    fx = {"N": N, "physics_dt": PHYSICS_DT, "first_read_error": first_read_error, "com_pos_b": short(com),
          "sensors": {name: {"offset_pos": list(c.offset.pos), "offset_rot": list(c.offset.rot), "gravity_bias": list(c.gravity_bias),
                             "update_period": c.update_period, "history_length": c.history_length} for name, c in cfgs.items()},
          "calls": calls}
    path = os.path.join(gg.GOLDEN, "imu_sensor.json")
    with open(path, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes,", len(calls), "calls")


if __name__ == "__main__":
    task_fixture()
    sensor_fixture()
