"""Random sweeps of the stateful producers against their oracles (which the reference's fixtures pin): ContactSensor update (random
body / history counts, update period gating, thresholds, forces, partial resets), UniformVelocityCommand (random ranges, heading /
standing fractions, resampling windows shorter and longer than a step, resets, fed uniforms), UniformPoseCommand (the same, against
tests/_pose_command_oracle.py), and -- against the oracles run in float64,
cases in tests/_producer_cases.py -- the delayed / remotized PD actuator, the LSTM and MLP actuator nets, the empirical normaliser and the
reset / interval events with the terrain curriculum.  lstm_net picks one of the three ANYdrive-shape kernels per case; the two that
IMX_LSTM_KERNEL selects run in a persistent child process each.  Test infrastructure, run on the GPU box:
    python tools/fuzz_producers.py [cases] [seed] [kind ...]"""
import atexit
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from _util import assert_close

CONTACT_KEYS = ("net_forces_w", "net_forces_w_history", "last_air_time", "current_air_time", "last_contact_time", "current_contact_time")
CMD_KEYS = ("vel_command_b", "heading_target", "is_heading_env", "is_standing_env", "time_left", "command_counter")


def case_contact(rng):
    from isaaclab_amd.producers import ContactSensorState
    from oracle.producers_oracle import contact_sensor_update

    N, B, H = int(rng.choice([1, 7, 64, 65, 1000, 4096])), int(rng.choice([1, 4, 17, 30])), int(rng.choice([0, 1, 3, 5]))
    dt = float(rng.choice([0.005, 0.02]))
    period = float(rng.choice([0.0, dt, 2 * dt, 0.05]))
    thr = float(rng.choice([1.0, 0.1, 5.0]))
    steps = int(rng.integers(3, 10))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    s = ContactSensorState(N, B, H, True, period, thr, "cuda:0")
    st = dict(timestamp=torch.zeros(N), timestamp_last_update=torch.zeros(N), is_outdated=torch.ones(N, dtype=torch.bool),
              net_forces_w=torch.zeros(N, B, 3), net_forces_w_history=torch.zeros(N, max(H, 0), B, 3), last_air_time=torch.zeros(N, B),
              current_air_time=torch.zeros(N, B), last_contact_time=torch.zeros(N, B), current_contact_time=torch.zeros(N, B))
    for k in range(steps):
        if rng.random() < 0.4:
            ids = torch.nonzero(torch.rand(N, generator=g) < 0.3).flatten()
            if len(ids):
                for name in ("timestamp", "timestamp_last_update", "net_forces_w", "net_forces_w_history", "current_air_time", "last_air_time",
                             "current_contact_time", "last_contact_time"):
                    st[name][ids] = 0.0
                st["is_outdated"][ids] = True
                s.reset(ids.cuda())
        f = torch.randn(N, B, 3, generator=g) * (torch.rand(N, B, 1, generator=g) < 0.5) * float(rng.choice([0.5, 3.0, 20.0]))
        contact_sensor_update(st, f, dt, period, thr, H, True)
        s.update(f.cuda(), dt)
        for name in CONTACT_KEYS:
            if name == "net_forces_w_history" and H == 0:
                continue
            assert torch.equal(getattr(s.data, name).cpu(), st[name]), (k, name)
        assert torch.equal(s._timestamp.cpu(), st["timestamp"]) and torch.equal(s._timestamp_last_update.cpu(), st["timestamp_last_update"]), (k, "stamps")
    return f"N={N} B={B} H={H} dt={dt} period={period} thr={thr} steps={steps}"


def case_command(rng):
    from isaaclab_amd.producers import UniformVelocityCommand
    from oracle.producers_oracle import VelocityCommandOracle

    N, step_dt = int(rng.choice([1, 63, 64, 65, 1000, 4096])), float(rng.choice([0.02, 0.005]))
    lo = float(rng.choice([0.5, 2.0, 10.0])) * step_dt
    rng2 = lambda a: [-float(a), float(a)]  # noqa: E731
    cfg = {"resampling_time_range": [lo, lo * float(rng.choice([1.0, 1.5, 3.0]))], "heading_command": bool(rng.integers(0, 2)),
           "heading_control_stiffness": float(rng.choice([0.5, 1.0])), "rel_standing_envs": float(rng.choice([0.0, 0.2, 1.0])),
           "rel_heading_envs": float(rng.choice([0.0, 0.7, 1.0])),
           "ranges": {"lin_vel_x": rng2(rng.choice([1.0, 0.3])), "lin_vel_y": [0.0, float(rng.choice([0.0, 0.5]))], "ang_vel_z": rng2(rng.choice([1.0, 2.0])),
                      "heading": [-3.141592653589793, 3.141592653589793]}}
    steps = int(rng.integers(3, 12))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    orc = VelocityCommandOracle(cfg, N, step_dt)
    cmd = UniformVelocityCommand(cfg, N, step_dt, "cuda:0")
    for k in range(steps):
        q = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
        lin, ang = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
        mask = torch.rand(N, generator=g) < float(rng.choice([0.0, 0.1, 1.0]))
        U = torch.rand(2, N, 7, generator=g)
        orc.reset_and_compute(step_dt, q, lin, ang, mask, U)
        cmd.compute(step_dt, q.cuda(), lin.cuda(), ang.cuda(), mask.cuda(), U.cuda())
        for name in CMD_KEYS:
            got, ref = getattr(cmd, name).cpu(), getattr(orc, name)
            if ref.dtype in (torch.bool, torch.long):
                assert torch.equal(got, ref), (k, name)
            else:
                assert_close(got, ref, 1e-5, f"step {k} {name}")
        assert_close(cmd.metrics["error_vel_xy"], orc.metrics["error_vel_xy"], 1e-5, "error_vel_xy")
        assert_close(cmd.metrics["error_vel_yaw"], orc.metrics["error_vel_yaw"], 1e-5, "error_vel_yaw")
    return f"N={N} step_dt={step_dt} resample={cfg['resampling_time_range']} heading={cfg['heading_command']} steps={steps}"


def case_pose_command(rng):
    """UniformPoseCommand: random ranges, body counts and indices, quat_unique on / off, resampling windows shorter and longer than a
    step (shorter: reset and timer resample in one call), reset masks all / none / mixed, do_compute 0 / 1, fed uniforms."""
    from _pose_command_cases import pose_case, random_cfg

    N, step_dt = int(rng.choice([1, 63, 64, 65, 257, 1000, 4096])), float(rng.choice([1.0 / 30.0, 0.02, 0.005]))
    NB = int(rng.choice([1, 8, 11, 30]))
    cfg = random_cfg(rng, step_dt, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
    plan = [(str(rng.choice(["all", "none", "mixed"])), bool(rng.random() < 0.8)) for _ in range(int(rng.integers(3, 12)))]
    return pose_case(N, NB, int(rng.integers(0, NB)), cfg, step_dt, plan, int(rng.integers(0, 1 << 30)))


def case_pd_actuator(rng):
    from isaaclab_amd.producers import PDActuator
    from oracle.producers_oracle import actuator_pd

    N, J = int(rng.choice([1, 7, 64, 1000, 4096])), int(rng.choice([1, 2, 12, 23, 37]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    stiff, damp, elim, vlim = 20 + 80 * r(N, J), 0.5 + 4 * r(N, J), 20 + 60 * r(N, J), 2 + 8 * r(N, J)
    sat = float(rng.choice([60.0, 120.0]))
    q_des, q, qd, qd_des, ff = (torch.randn(N, J, generator=g) * float(rng.choice([0.3, 2.0])) for _ in range(5))
    dc = bool(rng.integers(0, 2))
    kw = dict(velocity_limit=vlim, saturation_effort=sat) if dc else {}
    c0, a0 = actuator_pd(q_des, qd_des, ff, q, qd, stiff, damp, elim, **kw)
    act = PDActuator(stiff.cuda(), damp.cuda(), elim.cuda(), **({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}))
    applied = act.compute(q_des.cuda(), q.cuda(), qd.cuda(), qd_des.cuda(), ff.cuda())
    assert_close(act.computed_effort, c0, 1e-5, "computed effort")
    assert_close(applied, a0, 1e-5, "applied effort")
    return f"N={N} J={J} dc_motor={dc}"


def case_articulation(rng):
    from isaaclab_amd.producers import ArticulationRootState
    from oracle.mdp_oracle import convert_quat

    N, J, dt = int(rng.choice([1, 63, 1000, 4096])), int(rng.choice([1, 12, 37])), float(rng.choice([0.005, 0.02]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    prev = torch.randn(N, J, generator=g)
    st = ArticulationRootState(N, J, "cuda:0", prev.cuda())
    sim_t, acc_t = 0.0, -1.0
    for k in range(int(rng.integers(2, 6))):
        tf = torch.cat([torch.randn(N, 3, generator=g), torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)], 1)
        vel, dv = torch.randn(N, 6, generator=g), torch.randn(N, J, generator=g)
        sim_t += dt
        elapsed, acc_t = sim_t - acc_t, sim_t
        st.update(tf.cuda(), vel.cuda(), dv.cuda(), dt)
        assert torch.equal(st.root_pos_w.cpu(), tf[:, :3]) and torch.equal(st.root_quat_w.cpu(), convert_quat(tf[:, 3:7], to="wxyz")), (k, "root pose")
        assert torch.equal(st.root_lin_vel_w.cpu(), vel[:, :3]) and torch.equal(st.root_ang_vel_w.cpu(), vel[:, 3:]), (k, "root velocity")
        assert_close(st.joint_acc, (dv - prev) / elapsed, 1e-5, "joint_acc")
        prev = dv.clone()
    return f"N={N} J={J} dt={dt}"


def case_delayed(rng):
    from _producer_cases import delayed_case

    mx = int(rng.choice([0, 1, 2, 4, 7, 37]))
    mn = int(rng.integers(0, mx + 1))
    N, J = int(rng.choice([1, 2, 63, 65, 1000, 4097])), int(rng.choice([1, 3, 12, 23]))
    return delayed_case(N, J, mn, mx, None, int(rng.integers(0, 1 << 30)))


def case_remotized(rng):
    from _producer_cases import delayed_case

    mx = int(rng.choice([0, 1, 4, 37]))
    mn = int(rng.integers(0, mx + 1))
    N, J = int(rng.choice([1, 7, 63, 65, 1000, 4097])), int(rng.choice([1, 3, 12]))
    return delayed_case(N, J, mn, mx, int(rng.choice([1, 2, 3, 9, 16])), int(rng.integers(0, 1 << 30)), dup=bool(rng.integers(0, 2)))


_CHILDREN = {}


def _close(p):
    if p.poll() is None:
        p.stdin.close()
        p.wait(timeout=60)


def _child(kern):
    p = _CHILDREN.get(kern)
    if p is None or p.poll() is not None:
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "_producer_cases.py"), "--serve"]
        p = subprocess.Popen(cmd, env=dict(os.environ, IMX_LSTM_KERNEL=kern), cwd=ROOT, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        _CHILDREN[kern] = p
        atexit.register(_close, p)
    return p


def case_lstm_net(rng):
    """Random network and shape.  ANYdrive shapes (hidden 8, <= 4 layers, head none / 16 / 32) go to the matrix-core kernel in this
    process or to the lanes / register kernel in its child; the others to the generic kernel here."""
    from _producer_cases import ACTS, lstm_case

    fast = bool(rng.integers(0, 2))
    if fast:
        H, L, head = 8, int(rng.integers(1, 5)), [[], [16], [32]][int(rng.integers(0, 3))]
    else:
        H, L = int(rng.choice([1, 3, 5, 8, 16, 32])), int(rng.integers(1, 6))
        L = min(L, 3) if H == 32 else L
        head = [[], [8], [24], [16, 8], [64]][int(rng.integers(0, 5))]
        if H == 8 and L <= 4 and head in ([], [16], [32]):
            head = [24]
    N, J = int(rng.choice([1, 7, 31, 64, 129, 1000, 4097])), int(rng.choice([1, 3, 12]))
    kw = dict(N=N, J=J, H=H, L=L, head=head, act=str(rng.choice(ACTS)), seed=int(rng.integers(0, 1 << 30)), steps=int(rng.integers(2, 9)),
              unaligned=bool(not fast and H == 8 and rng.integers(0, 2)))
    kern = str(rng.choice(["m", "l", "r"])) if fast else "generic"
    if kern in ("m", "generic"):
        return f"[{kern}] " + lstm_case(**kw)
    p = _child(kern)
    p.stdin.write(json.dumps(kw) + "\n")
    p.stdin.flush()
    for line in p.stdout:
        if line.startswith("@@ ok "):
            return f"[{kern}] " + line[6:].strip()
        if line.startswith("@@ FAIL "):
            raise AssertionError(f"IMX_LSTM_KERNEL={kern}: " + line[8:].strip())
    raise RuntimeError(f"IMX_LSTM_KERNEL={kern} child exited with {p.wait(timeout=60)} on {kw}")


def case_mlp_net(rng):
    from _producer_cases import ACTS, mlp_case

    idx = [int(v) for v in rng.integers(0, 6, size=int(rng.integers(1, 4)))]
    widths = [int(rng.choice([1, 8, 16, 24, 32, 64])) for _ in range(int(rng.integers(0, 4)))]
    N, J = int(rng.choice([1, 7, 63, 65, 1000, 4097])), int(rng.choice([1, 3, 12]))
    scales = tuple(float(v) for v in rng.choice([0.1, 0.5, 1.0, 2.0, 7.5], size=3))
    return mlp_case(N, J, idx, str(rng.choice(["pos_vel", "vel_pos"])), str(rng.choice(ACTS)), widths, int(rng.integers(0, 1 << 30)), scales)


def case_normalizer(rng):
    from _producer_cases import normalizer_case

    D = int(rng.choice([1, 2, 63, 64, 65, 235, 310, 513]))
    rows = [1, 2, 63, 64, 4096, 4097] + ([100003] if D <= 65 else [])  # (a 100 003 x 513 batch is 0.2 GB of oracle work per call)
    batches = [int(rng.choice(rows)) for _ in range(int(rng.integers(1, 5)))]
    return normalizer_case(D, batches, int(rng.integers(0, 1 << 30)))


def case_events(rng):
    from _producer_cases import events_case

    N, J, NB = int(rng.choice([1, 2, 63, 64, 65, 255, 257, 4097, 100003])), int(rng.choice([1, 12, 37])), int(rng.choice([1, 4, 17]))
    ids = None
    if rng.integers(0, 2):
        ids = sorted(int(b) for b in rng.choice(NB, size=int(rng.integers(1, NB + 1)), replace=False))
    R, C = int(rng.choice([1, 2, 10])), int(rng.choice([1, 3, 20]))
    return events_case(N, J, NB, R, C, int(rng.integers(0, 1 << 30)), body_ids=ids, degenerate=bool(rng.integers(0, 2)))


KINDS = (("contact_sensor", case_contact), ("velocity_command", case_command), ("pose_command", case_pose_command), ("pd_actuator", case_pd_actuator), ("articulation", case_articulation),
         ("delayed", case_delayed), ("remotized", case_remotized), ("lstm_net", case_lstm_net), ("mlp_net", case_mlp_net),
         ("normalizer", case_normalizer), ("events", case_events))

if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    only = set(sys.argv[3:])
    bad = 0
    for name, fn in KINDS:
        if only and name not in only:
            continue
        rng = np.random.default_rng(seed)
        nbad, last = 0, ""
        for c in range(cases):
            try:
                last = fn(rng)
            except (AssertionError, RuntimeError, ValueError) as exc:
                nbad += 1
                print(f"{name} case {c}: FAIL {type(exc).__name__}: {str(exc)[:300]}", flush=True)
        bad += nbad
        print(f"{name}: {cases - nbad} / {cases} cases agree (last: {last})", flush=True)
    sys.exit(1 if bad else 0)
