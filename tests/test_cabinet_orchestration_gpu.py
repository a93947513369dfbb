"""GPU: the Open-Drawer task's ``_reset_idx`` inside the one orchestration launch (``imx_reset_orchestrate_scene``) --
``reset_scene_to_default`` on the robot and the cabinet, joint and root-state reset events on the cabinet -- against the fixtures of the
REAL reference (tools/gen_golden_cabinet_orchestration.py) and the numpy restatement (tests/_cabinet_orch_oracle.py)."""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import _cabinet_cases as cc
import _cabinet_orch_oracle as co
import _manip_orch_oracle as mo

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF
DEV = "cuda:0"
# The one quantity of the direct-launch cases that is not compared bit for bit: the quaternion of reset_root_state_uniform with a
# rotation in its range.  sinf / cosf of the device library and of numpy may differ in the last place; the six of them enter products of
# three factors of magnitude <= 1, summed in pairs, and quat_mul adds <= 8 products of those: <= 16 roundings of values <= 1.
QUAT_TOL = 16 * 2.0 ** -23


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(torch.as_tensor(a).cpu().float()), _bits(torch.as_tensor(b).cpu().float()))


# ------------------------------------------------------------------------------------------------ parity with the real managers
def _feed_draws(env, g, slot):
    d = g.draws(slot)
    for t in env.event_manager.terms:
        if t.width:
            t.uniforms = torch.from_numpy(d[t.name][:, :t.width]).cuda().contiguous()


@pytest.mark.parametrize("which", ["shipped", "events"])
def test_orchestration_matches_the_real_managers(which):
    """``own_managers=True`` on the fixture's cfg at N = 64, fed the recorded draws, ``reset()`` + every recorded step.  Reset ids, masks,
    episode lengths, trigger state and both step counters exact; all eight ``sim_writes`` tensors -- the robot's four and the cabinet's
    four -- BIT FOR BIT at every tag: copies, fp32 adds in the reference's order and clamps (the fixtures' ranges are symmetric and the
    cabinet's root event does not rotate, so no quantity depends on a transcendental function or on where ``hi - lo`` is rounded)."""
    from isaaclab_amd.env import ManagerBasedRLEnv

    g = co.CabinetOrchGolden(which)
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed(DEV), own_managers=True)
    ev = env.event_manager
    assert ev.active_terms == g.meta["event_terms"] and ev.needs_scene and ev.skipped_terms == g.meta["skipped_startup_terms"]
    assert env.command_term is None and env._orch_articulation is None  # (built with the first launch)
    assert set(g.write_keys) <= set(env.sim_writes)
    st = g.static()
    data = env.scene["cabinet"].data
    assert _same(data.default_root_state, st["cabinet_default_root_state"]) and _same(data.default_joint_pos, st["cabinet_default_joint_pos"])
    if which == "events":  # the soft limits the env derives from the scene entry's tables are the reference's
        assert _same(data.soft_joint_pos_limits, st["cabinet_soft_joint_pos_limits"]) and _same(data.soft_joint_vel_limits, st["cabinet_soft_joint_vel_limits"])
    else:
        assert data.soft_joint_pos_limits is None and data.soft_joint_vel_limits is None

    def check(tag, count):
        torch.cuda.synchronize()
        for k in g.write_keys:
            assert _same(env.sim_writes[k], g.a(f"{tag}/sim_writes/{k}")), f"{tag} sim_writes[{k}]"
        assert torch.equal(torch.stack([t.last_triggered_step.cpu() for t in ev.terms]).long(), g.t(f"{tag}/reset_last_triggered_step").long()), tag
        assert torch.equal(torch.stack([t.triggered_once.cpu() for t in ev.terms]), g.t(f"{tag}/reset_triggered_once")), tag
        assert env.common_step_counter == count == int(g.z[f"{tag}/common_step_counter"]) == int(env._counters[2]), tag

    _feed_draws(env, g, 0)
    env.reset()
    assert env._orch_articulation is not None
    check("reset", 0)
    env.episode_length_buf = g.t("reset/episode_length_buf")
    resets = 0
    for k in range(g.steps):
        tag = f"step{k}"
        _feed_draws(env, g, k + 1)
        _, _, terminated, time_outs, _ = env.step(g.t(f"{tag}/action").cuda())
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")) and torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs"))
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids"))
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf"))
        check(tag, k + 1)
        resets += len(g.reset_ids(k))
    assert resets == g.meta["n_resets"]
    env.close()


# ------------------------------------------------------------------------------------------------ the launch alone
class _Launch:
    """One direct ``imx_reset_orchestrate_scene`` launch on tensors of the test's own: robot with J joints, second articulation with J2.
    Every out buffer has a guard row before and after its N rows and starts as a NaN bit pattern."""

    def __init__(self, N, J2, J=3, seed=0):
        from isaaclab_amd import _lib

        self.N, self.J, self.J2, self._lib = N, J, J2, _lib
        rng = np.random.default_rng(1000 * N + J2 + seed)
        f = lambda *s: rng.normal(size=s).astype(np.float32)  # noqa: E731
        st = {"env_origins": f(N, 3) * 4}
        for pre, j in (("", J), ("cabinet_", J2)):
            d = f(N, 13)
            d[:, 3:7] /= np.linalg.norm(d[:, 3:7], axis=1, keepdims=True)
            lo = rng.uniform(-1.0, 0.0, (N, j))
            st.update({pre + "default_root_state": d, pre + "default_joint_pos": f(N, j) * 0.5, pre + "default_joint_vel": f(N, j) * 0.5,
                       pre + "soft_joint_pos_limits": np.stack([lo, lo + rng.uniform(0.1, 1.5, (N, j))], -1).astype(np.float32),
                       pre + "soft_joint_vel_limits": rng.uniform(0.1, 1.0, (N, j)).astype(np.float32)})
        self.st, self.rng = st, rng
        self.dev = {k: torch.from_numpy(v).to(DEV) for k, v in st.items()}
        nan = torch.tensor(NAN_BITS, dtype=torch.int32).view(torch.float32).item()
        shape = {"root_pose": 7, "root_vel": 6}
        self.out = {pre + k: torch.full((N + 2, shape.get(k, j)), nan, device=DEV) for pre, j in (("", J), ("cabinet_", J2)) for k in co.KINDS}
        self.count = torch.tensor([5], dtype=torch.int32, device=DEV)
        self.keep = []

    def structs(self, terms, mask):
        """``terms``: (op name, asset, ranges, uniforms or None)."""
        from isaaclab_amd import _abi
        from isaaclab_amd._lib import ImxOrch, ImxOrchArticulation, ImxOrchManip

        ops, d, N = _abi.ENUMS["imx_event_op"], self.dev, self.N
        row1 = lambda k: self.out[k][1:].data_ptr()  # noqa: E731
        self.mask = torch.from_numpy(mask).to(DEV)
        o = ImxOrch(num_envs=N, num_joints=self.J, num_bodies=1, dt=0.02, env_origins_d=d["env_origins"].data_ptr(), num_terms=len(terms),
                    step_counter_d=self.count.data_ptr(), reset_mask_d=self.mask.data_ptr(), seed=77,
                    default_root_state_d=d["default_root_state"].data_ptr(), default_joint_pos_d=d["default_joint_pos"].data_ptr(),
                    default_joint_vel_d=d["default_joint_vel"].data_ptr(), soft_joint_pos_limits_d=d["soft_joint_pos_limits"].data_ptr(),
                    soft_joint_vel_limits_d=d["soft_joint_vel_limits"].data_ptr(), root_pose_out_d=row1("root_pose"), root_vel_out_d=row1("root_vel"),
                    joint_pos_out_d=row1("joint_pos"), joint_vel_out_d=row1("joint_vel"))
        self.trig = []
        for i, (op, asset, ranges, u) in enumerate(terms):
            T = o.terms[i]
            last, once = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
            self.trig.append((last, once))
            T.op, T.asset, T.last_triggered_step_d, T.triggered_once_d = ops["IMX_E_" + op.upper()], asset, last.data_ptr(), once.data_ptr()
            for k, v in enumerate(ranges):
                T.ranges[k] = v
            if u is not None:
                self.keep.append(torch.from_numpy(np.ascontiguousarray(u, np.float32)).to(DEV))
                T.uniforms_d = self.keep[-1].data_ptr()
        a = ImxOrchArticulation(num_joints=self.J2, default_root_state_d=d["cabinet_default_root_state"].data_ptr(),
                                default_joint_pos_d=d["cabinet_default_joint_pos"].data_ptr(), default_joint_vel_d=d["cabinet_default_joint_vel"].data_ptr(),
                                soft_joint_pos_limits_d=d["cabinet_soft_joint_pos_limits"].data_ptr(),
                                soft_joint_vel_limits_d=d["cabinet_soft_joint_vel_limits"].data_ptr(), root_pose_out_d=row1("cabinet_root_pose"),
                                root_vel_out_d=row1("cabinet_root_vel"), joint_pos_out_d=row1("cabinet_joint_pos"), joint_vel_out_d=row1("cabinet_joint_vel"))
        return o, ImxOrchManip(), a

    def run(self, o, m, a):
        L = self._lib.lib()
        status = L.imx_reset_orchestrate_scene(ctypes.byref(o), ctypes.byref(m), ctypes.byref(a), self._lib.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return status, L.imx_last_error().decode()

    def untouched(self, keys=None, rows=None):
        """The guard rows of every buffer, and of ``keys`` (default: all) also the rows ``rows`` (default: all), still hold the fill."""
        for k, t in self.out.items():
            b = _bits(t.cpu())
            sel = torch.zeros(self.N + 2, dtype=torch.bool)
            sel[0] = sel[-1] = True
            if keys is None or k in keys:
                sel[1:-1] = True if rows is None else torch.from_numpy(rows)
            if not bool((b[sel] == NAN_BITS).all()):
                return False
        return True


def _mask(N, rng):
    mask = rng.random(N) < 0.3
    mask[[i for i in (0, 62, 63, 64, 65, N - 1) if i < N]] = True
    if N > 2:
        mask[1] = False
    return mask


@pytest.mark.parametrize("J2", [1, 4, 65])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_masking_and_tails(N, J2):
    """N below, at and past one and two workgroups, J2 below and past the lane stride of 64.  Out buffers start as a NaN bit pattern and
    carry guard rows.  Three launches: ``reset_scene_to_default``; ``reset_joints_by_offset`` + ``reset_root_state_uniform`` on the second
    articulation; ``reset_joints_by_scale`` on it.  Guards and rows not flagged keep their bits, and so does every buffer of the asset a
    launch has no term for; flagged rows equal the restatement bit for bit, except the rotated quaternion (QUAT_TOL above)."""
    x = _Launch(N, J2)
    st, rng = x.st, x.rng
    mask = _mask(N, rng)
    ids = np.nonzero(mask)[0]
    pr = {a: (-b, b) for a, b in zip(mo.AXES, (0.3, 0.2, 0.1, 0.4, 0.5, 3.0))}
    vr = {a: (-b, b) for a, b in zip(mo.AXES, (0.5, 0.4, 0.3, 0.2, 0.1, 1.0))}
    uj, ur, us = rng.random((N, 2 * J2), np.float32), rng.random((N, 12), np.float32), rng.random((N, 2 * J2), np.float32)
    cab = {"name": "cabinet"}
    rounds = [
        ({"all": {"func": "m:reset_scene_to_default", "params": {}}}, [("reset_scene_to_default", 0, [], None)], {}, None),
        ({"j": {"func": "m:reset_joints_by_offset", "params": {"position_range": (-0.5, 0.5), "velocity_range": (-1.0, 1.0), "asset_cfg": cab}},
          "r": {"func": "m:reset_root_state_uniform", "params": {"pose_range": pr, "velocity_range": vr, "asset_cfg": cab}}},
         [("reset_joints_by_offset", 2, [-0.5, 0.5, -1.0, 1.0], uj),
          ("reset_root_state_uniform", 2, np.concatenate([mo.axis_ranges(pr).ravel(), mo.axis_ranges(vr).ravel()]), ur)], {"j": uj, "r": ur}, "cabinet_"),
        ({"s": {"func": "m:reset_joints_by_scale", "params": {"position_range": (0.5, 1.5), "velocity_range": (-2.0, 2.0), "asset_cfg": cab}}},
         [("reset_joints_by_scale", 2, [0.5, 1.5, -2.0, 2.0], us)], {"s": us}, "cabinet_"),
    ]
    sw = co.new_sim_writes(N, x.J, "cabinet", J2, fill=np.float32(np.nan))
    written = set()
    for events, terms, draws, only in rounds:
        status, err = x.run(*x.structs(terms, mask))
        assert status == 0, err
        trig = {"last": np.zeros((len(terms), N), np.int64), "once": np.zeros((len(terms), N), bool)}
        co.apply_reset_events(events, ids, 5, sw, trig, st, draws, "cabinet")
        written |= set(sw) if only is None else ({"cabinet_joint_pos", "cabinet_joint_vel"} | ({"cabinet_root_pose", "cabinet_root_vel"} if "r" in events else set()))
        assert x.untouched(rows=~mask) and x.untouched(keys=set(sw) - written)
        for k in written:
            got, want = x.out[k][1:-1].cpu()[mask], torch.from_numpy(sw[k][mask])
            if k == "cabinet_root_pose" and "all" not in events:  # (what the second launch wrote stays through the third)
                assert torch.equal(_bits(got[:, :3]), _bits(want[:, :3])), k
                assert float((got[:, 3:] - want[:, 3:]).abs().max()) <= QUAT_TOL, k
            else:
                assert torch.equal(_bits(got), _bits(want)), k
        for i, (last, once) in enumerate(x.trig):
            assert np.array_equal(last.cpu().numpy(), trig["last"][i]) and np.array_equal(once.cpu().numpy().astype(bool), trig["once"][i])
    if J2 > 1 and len(ids) > 1:  # the clamps were hit and missed
        lim = st["cabinet_soft_joint_pos_limits"][mask]
        jp = x.out["cabinet_joint_pos"][1:-1].cpu().numpy()[mask]
        assert (jp == lim[..., 0]).any() or (jp == lim[..., 1]).any()
        assert ((jp > lim[..., 0]) & (jp < lim[..., 1])).any()


def test_in_kernel_draws_are_keyed_as_the_robot_s():
    """No draw tables: ``draw(U = NULL, 2 J2, env, column, seed, term, step)``.  The same term index, seed, step and joint count on the
    robot and on the second articulation, the same defaults and limits: the same joint state, bit for bit -- and not the defaults."""
    N, J = 70, 5
    x = _Launch(N, J, J=J)
    for k in ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits"):
        x.dev["cabinet_" + k].copy_(x.dev[k])
    mask = np.ones(N, bool)
    r = [-0.5, 0.5, -1.0, 1.0]
    for asset in (0, 2):
        status, err = x.run(*x.structs([("reset_joints_by_offset", asset, r, None)], mask))
        assert status == 0, err
    for k in ("joint_pos", "joint_vel"):
        a, b = x.out[k][1:-1], x.out["cabinet_" + k][1:-1]
        assert torch.equal(_bits(a), _bits(b)) and not torch.isnan(a).any()
    assert float((x.out["joint_pos"][1:-1] - x.dev["default_joint_pos"]).abs().max()) > 0.05
    assert x.untouched(keys={"root_pose", "root_vel", "cabinet_root_pose", "cabinet_root_vel"})


def test_argument_checks_name_what_is_missing_and_launch_nothing():
    from isaaclab_amd import _lib

    N, J2 = 65, 4
    x = _Launch(N, J2)
    mask = np.ones(N, bool)
    L, s = _lib.lib(), _lib.current_stream(torch.device(DEV))
    err = lambda: L.imx_last_error().decode()  # noqa: E731
    r = [-0.5, 0.5, -1.0, 1.0]
    joints = [("reset_scene_to_default", 0, [], None), ("reset_joints_by_offset", 2, r, None)]
    # a null out buffer, by name, for the term that needs it
    for field, terms, words in (("joint_vel_out_d", joints, ("term 0", "reset_scene_to_default", "joint_vel_out")),
                                ("root_pose_out_d", [("reset_root_state_uniform", 2, [0.0] * 24, None)], ("term 0", "second articulation", "root_pose_out")),
                                ("joint_pos_out_d", joints[1:], ("term 0", "second articulation", "joint_pos_out"))):
        o, m, a = x.structs(terms, mask)
        setattr(a, field, None)
        status, e = x.run(o, m, a)
        assert status != 0 and all(w in e for w in words), e
    # a joint event on the second articulation without a limit table; reset_scene_to_default and the root event do without both
    for field, word in (("soft_joint_pos_limits_d", "soft_joint_pos_limits"), ("soft_joint_vel_limits_d", "soft_joint_vel_limits")):
        o, m, a = x.structs(joints, mask)
        setattr(a, field, None)
        status, e = x.run(o, m, a)
        assert status != 0 and "term 1" in e and "joint event" in e and word in e, e
    # an op without a kernel on that asset
    status, e = x.run(*x.structs([("push_by_setting_velocity", 2, [0.0] * 12, None)], mask))
    assert status != 0 and "term 0" in e and "second articulation has no kernel" in e, e
    status, e = x.run(*x.structs([("reset_joints_around_default", 2, r, None)], mask))
    assert status != 0 and "second articulation has no kernel" in e, e
    # null structs, and asset = 2 through the two older entry points
    o, m, a = x.structs(joints[1:], mask)
    assert L.imx_reset_orchestrate_scene(ctypes.byref(o), ctypes.byref(m), None, s) != 0 and "null imx_orch_articulation_t" in err()
    assert L.imx_reset_orchestrate_scene(ctypes.byref(o), None, ctypes.byref(a), s) != 0 and "null imx_orch_manip_t" in err()
    assert L.imx_reset_orchestrate(ctypes.byref(o), s) != 0 and "asset 2" in err() and "imx_reset_orchestrate_scene" in err()
    assert L.imx_reset_orchestrate_manip(ctypes.byref(o), ctypes.byref(m), s) != 0 and "asset 2" in err() and "imx_reset_orchestrate_scene" in err()
    a.num_joints = 0
    status, e = x.run(o, m, a)
    assert status != 0 and "0 joints" in e, e
    torch.cuda.synchronize()
    assert x.untouched()  # nothing was launched
    for last, once in x.trig:
        assert not bool(last.any()) and not bool(once.any())
    # ... and the complete call goes through, without the limits when no joint event asks for them
    o, m, a = x.structs([("reset_scene_to_default", 0, [], None), ("reset_root_state_uniform", 2, [0.0] * 24, None)], mask)
    a.soft_joint_pos_limits_d = a.soft_joint_vel_limits_d = None
    status, e = x.run(o, m, a)
    assert status == 0, e
    assert not torch.isnan(x.out["cabinet_joint_pos"][1:-1]).any() and x.untouched(rows=~mask)


# ------------------------------------------------------------------------------------------------ the env's paths
def _feed(task, N, seed, snapshots):
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    return StateFeed(ROBOTS[cc.load_fixture(task)["robot"]], N, DEV, seed=seed, num_snapshots=snapshots)


@pytest.mark.parametrize("kw", [dict(events_cfg=True), dict(own_managers=True)], ids=["events_cfg", "own_managers"])
@pytest.mark.parametrize("task", [cc.TASK, cc.TASK_IK_ABS, cc.TASK_IK_REL])
def test_the_env_owns_the_reset_of_the_open_drawer_tasks(task, kw):
    """The committed task fixtures at N = 64, eagerly: the parent refused both keywords at construction.  After ``reset()`` every env's
    cabinet sits at its default root pose + env origin with its default joint state; a time-out rewrites exactly that env's rows."""
    from isaaclab_amd.env import ManagerBasedRLEnv

    N = 64
    fx = cc.load_fixture(task)
    env = ManagerBasedRLEnv(fx, state_feed=_feed(task, N, 5, 4), seed=5, noise_seed=5, **kw)
    assert env.event_manager.needs_scene and [t.name for t in env.event_manager.terms] == ["reset_all", "reset_robot_joints"]
    assert {"cabinet_root_pose", "cabinet_root_vel", "cabinet_joint_pos", "cabinet_joint_vel"} <= set(env.sim_writes)
    data = env.scene["cabinet"].data
    assert tuple(data.default_root_state.shape) == (N, 13) and data.default_root_state[0, :7].tolist() == pytest.approx([0.8, 0, 0.4, 0, 0, 0, 1])
    env.reset()
    want = data.default_root_state[:, :7].clone()
    want[:, :3] += env.feed["env_origins"]
    assert torch.equal(env.sim_writes["cabinet_root_pose"], want) and not bool(env.sim_writes["cabinet_root_vel"].any())
    assert torch.equal(env.sim_writes["cabinet_joint_pos"], data.default_joint_pos)
    dq = env.sim_writes["joint_pos"] - env.feed["default_joint_pos"]
    assert 0.01 < float(dq.abs().max()) <= 0.1 + 1e-6  # reset_robot_joints: default + U(-0.1, 0.1), after reset_all
    nan = float("nan")
    for k in ("cabinet_root_pose", "cabinet_joint_vel"):
        env.sim_writes[k].fill_(nan)
    ep = torch.zeros(N, dtype=torch.long)
    ep[37] = env.max_episode_length - 1
    env.episode_length_buf = ep
    env.step(torch.zeros(N, env.plan.action_dim, device=DEV))
    assert env.reset_env_ids.cpu().tolist() == [37]
    rows = torch.isnan(env.sim_writes["cabinet_root_pose"]).any(dim=1)
    assert (~rows).nonzero().flatten().tolist() == [37] and torch.equal(env.sim_writes["cabinet_root_pose"][37], want[37])
    assert (~torch.isnan(env.sim_writes["cabinet_joint_vel"]).any(dim=1)).nonzero().flatten().tolist() == [37]
    env.close()


def test_pose2d_command_beside_these_events_stays_refused():
    """The launch of a pose-2d command term has no place for the second articulation either: the Navigation cfg with a cabinet in its
    scene and a reset event on it is refused by name when the orchestration descriptor is built, as beside a rigid object's event."""
    from _pose2d_cases import NavOrchGolden
    from isaaclab_amd import producers
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.state_feed import StateFeed

    g, c = NavOrchGolden(), co.CabinetOrchGolden("events").fixture["env"]
    fx = copy.deepcopy(g.fixture)
    fx["env"]["scene"]["cabinet"] = c["scene"]["cabinet"]
    fx["env"]["events"] = dict(fx["env"]["events"], reset_cabinet_root=c["events"]["reset_cabinet_root"])
    N = 64
    term = producers.UniformPose2dCommand(fx["env"]["commands"]["pose_command"], N, g.meta["step_dt"], DEV, seed=5)
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(g.robot, N, DEV, seed=3, num_snapshots=2), command_term=term, events_cfg=True)
    assert env.event_manager.needs_scene and not env.event_manager.needs_manip
    with pytest.raises(NotImplementedError, match="command term '.*': a pose-2d command beside an event on a rigid object or reset_scene_to_default is not built"):
        env.reset()  # (the orchestration descriptor is built with the first launch)
    env.close()


def _rollout(task, graph, tmp_path):
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    N, T = 64, 3
    fx = cc.load_fixture(task)
    torch.manual_seed(31)
    env = ManagerBasedRLEnv(fx, state_feed=_feed(task, N, 9, T), own_managers=True, seed=31, noise_seed=31)
    env.seed(31)
    venv = RslRlVecEnvWrapper(env)
    runner = OnPolicyRunner(venv, dict(fx["agent"], num_steps_per_env=T), log_dir=str(tmp_path / f"{task}-g{int(graph)}"), device=DEV, use_graph=graph)
    assert runner._fusable()
    venv.episode_length_buf = env.max_episode_length - 1 - (torch.arange(N) % 7)  # time-outs on every step of the three rollouts
    if not graph:  # the captured runner's first rollout is its eager warm-up: the same rollout here, discarded
        runner.collect()
        runner.alg.storage.clear()
    for _ in range(2):
        runner.learn(1)
    torch.cuda.synchronize()
    st = runner.alg.storage
    out = {k: getattr(st, k).clone() for k in ("observations", "actions", "rewards", "dones", "values")}
    out.update({"sim_writes/" + k: v.clone() for k, v in env.sim_writes.items()})
    captured = runner._graph is not None
    env.close()
    return out, captured


@pytest.mark.parametrize("task", [cc.TASK, cc.TASK_IK_ABS, cc.TASK_IK_REL])
def test_captured_rollout_equals_eager(task, tmp_path):
    """``OnPolicyRunner`` on ``own_managers=True`` at N = 64, three steps per rollout, ``use_graph`` True and False with the same seeds:
    the fused rollout holds, the graph is captured, and storages and all ``sim_writes`` are bit-identical."""
    os.environ["IMX_RUNNER_QUIET"] = "1"
    try:
        (a, cap_a), (b, cap_b) = _rollout(task, True, tmp_path), _rollout(task, False, tmp_path)
    finally:
        os.environ.pop("IMX_RUNNER_QUIET", None)
    assert cap_a and not cap_b
    assert bool(a["dones"].any()) and float(a["sim_writes/cabinet_root_pose"].abs().sum()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between the captured and the eager rollout"
