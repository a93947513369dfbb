"""Shape / edge cases of the actuator, normaliser and event kernels against their oracles run in float64 on the same fp32 inputs, shared by
tests/test_producer_shapes_gpu.py and tools/fuzz_producers.py.  Every case asserts and returns a one-line description.

``imx_actuator_net_lstm`` picks its ANYdrive-shape kernel once per process (``IMX_LSTM_KERNEL``: unset = matrix core, ``l`` = eight lanes
per sample, ``r`` = one lane per sample); the other two are reached in a fresh child process:
    IMX_LSTM_KERNEL=r python tests/_producer_cases.py '<json list of lstm_case keyword dicts>'"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from _util import FLOAT_TOL, assert_close, assert_close_terms, check_normalizer_step  # noqa: E402

ACTS = ("identity", "softsign", "tanh", "relu", "elu")
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _subset(g, N, frac=0.3):
    ids = torch.nonzero(torch.rand(N, generator=g) < frac).flatten()
    return ids if len(ids) else torch.tensor([N - 1])


def _dc_inputs(g, N, J, sat_scale):
    """Per-joint effort / velocity limits, the saturation below part of the effort limits, and a joint velocity that sits exactly on
    +-v_lim for every 5th sample and beyond it for others (the DC-motor clip active in both directions)."""
    elim = 0.2 + torch.rand(J, generator=g) * sat_scale
    vlim = 0.5 + 2.0 * torch.rand(J, generator=g)
    sat = 0.8 * sat_scale
    return elim, vlim, sat


def _joint_vel(g, N, J, vlim):
    qd = torch.randn(N, J, generator=g) * 1.5
    flat = qd.view(-1)
    k = torch.arange(flat.numel())
    vl = vlim.expand(N, J).reshape(-1)
    flat[k % 5 == 0] = vl[k % 5 == 0]
    flat[k % 5 == 1] = -vl[k % 5 == 1]
    return qd


# ----------------------------------------------------------------------------------------------------------------- ActuatorNetLSTM
def lstm_case(N, J, H, L, head, act, seed, steps=8, unaligned=False):
    """``head``: widths of the hidden dense layers of the head ([] = H -> 1).  ``unaligned``: the hidden / cell state tensors start one
    float past a 16-byte boundary (the library must take the generic kernel)."""
    from isaaclab_amd.producers import ActuatorNetLSTM
    from oracle.producers_oracle import ActuatorNetLSTMOracle

    g = _gen(seed)
    r = lambda *s: torch.rand(*s, generator=g) - 0.5  # noqa: E731
    lstm = [(r(4 * H, 2 if k == 0 else H), r(4 * H, H), r(4 * H), r(4 * H)) for k in range(L)]
    widths, dense, d_in = list(head) + [1], [], H
    for w in widths:
        dense.append((r(w, d_in) * 2.0, r(w)))
        d_in = w
    elim, vlim, sat = _dc_inputs(g, N, J, 1.0)
    # centre the torque on zero (the output bias less the median of a probe step): a random net's torque is mostly of one sign, and the
    # clip must act on both
    probe = ActuatorNetLSTMOracle(N, J, lstm, dense, act, sat, elim.expand(N, J), vlim.expand(N, J))
    c0 = probe.compute(torch.randn(N, J, generator=g), torch.randn(N, J, generator=g), torch.randn(N, J, generator=g))[0]
    dense[-1] = (dense[-1][0], dense[-1][1] - c0.median())
    dev = "cuda:0"
    a = ActuatorNetLSTM(N, J, elim.cuda(), vlim.cuda(), sat, lstm_layers=[tuple(t.cuda() for t in l_) for l_ in lstm],
                        head=[tuple(t.cuda() for t in d) for d in dense], head_activation=act, device=dev)
    n = N * J
    if unaligned:
        for name in ("sea_hidden_state", "sea_cell_state"):
            buf = torch.zeros(L * n * H + 1, device=dev)[1:].view(L, n, H)
            setattr(a, name, buf)
            setattr(a, name + "_per_env", buf.view(L, N, J, H))
        assert a.sea_hidden_state.data_ptr() % 16 != 0
    o = ActuatorNetLSTMOracle(N, J, [tuple(t.to(F64) for t in l_) for l_ in lstm], [tuple(t.to(F64) for t in d) for d in dense], act, sat,
                              elim.to(F64).expand(N, J), vlim.to(F64).expand(N, J))
    o.h, o.c = o.h.to(F64), o.c.to(F64)
    lo_hit = hi_hit = 0
    for k in range(steps):
        if k in (3, 6):
            ids = _subset(g, N)
            a.reset(ids.cuda())
            o.reset(ids)
        q_des, q = torch.randn(N, J, generator=g), torch.randn(N, J, generator=g)
        qd = _joint_vel(g, N, J, vlim)
        a.compute(q_des.cuda(), q.cuda(), qd.cuda())
        c64, a64 = o.compute(q_des.to(F64), q.to(F64), qd.to(F64))
        what = f"lstm N={N} J={J} H={H} L={L} head={head} {act} step {k}"
        assert_close(a.computed_effort, c64, FLOAT_TOL, what + " computed")
        assert_close(a.applied_effort, a64, FLOAT_TOL, what + " applied")
        assert_close(a.sea_hidden_state, o.h, FLOAT_TOL, what + " hidden")
        assert_close(a.sea_cell_state, o.c, FLOAT_TOL, what + " cell")
        lo_hit += int((a64 > c64).sum())
        hi_hit += int((a64 < c64).sum())
    if n >= 4096:
        assert lo_hit > 0 and hi_hit > 0, f"the DC-motor clip was not exercised in both directions ({lo_hit}, {hi_hit})"
    return f"lstm N={N} J={J} H={H} L={L} head={head} act={act} unaligned={unaligned}"


# ----------------------------------------------------------------------------------------------------------------- ActuatorNetMLP
def mlp_case(N, J, input_idx, order, act, widths, seed, scales=(1.7, 0.35, 3.0), steps=None):
    from isaaclab_amd.producers import ActuatorNetMLP
    from oracle.producers_oracle import ActuatorNetMLPOracle

    g = _gen(seed)
    r = lambda *s: torch.rand(*s, generator=g) - 0.5  # noqa: E731
    layers, d_in = [], 2 * len(input_idx)
    for w in list(widths) + [1]:
        layers.append((r(w, d_in) * 2.0, r(w)))
        d_in = w
    elim, vlim, sat = _dc_inputs(g, N, J, 3.0)
    ps, vs, ts = scales
    a = ActuatorNetMLP(N, J, elim.cuda(), vlim.cuda(), sat, input_idx, ps, vs, ts, order, layers=[tuple(t.cuda() for t in l_) for l_ in layers],
                       activation=act, device="cuda:0")
    o = ActuatorNetMLPOracle(N, J, [tuple(t.to(F64) for t in l_) for l_ in layers], act, input_idx, ps, vs, ts, order, sat,
                             elim.to(F64).expand(N, J), vlim.to(F64).expand(N, J))
    o.pos_hist, o.vel_hist = o.pos_hist.to(F64), o.vel_hist.to(F64)
    steps = steps or a.history_length + 4
    for k in range(steps):
        if k in (2, a.history_length + 1):
            ids = _subset(g, N)
            a.reset(ids.cuda())
            o.reset(ids)
        q_des, q = torch.randn(N, J, generator=g), torch.randn(N, J, generator=g)
        qd = _joint_vel(g, N, J, vlim)
        a.compute(q_des.cuda(), q.cuda(), qd.cuda())
        c64, a64 = o.compute(q_des.to(F64), q.to(F64), qd.to(F64))
        what = f"mlp N={N} J={J} idx={input_idx} {order} {act} widths={widths} step {k}"
        # fp64 (q_des - q) of two floats rounds to the fp32 difference: the histories must agree bit for bit
        assert torch.equal(a._joint_pos_error_history.cpu(), o.pos_hist.float()), what + " position-error history"
        assert torch.equal(a._joint_vel_history.cpu(), o.vel_hist.float()), what + " velocity history"
        pos = torch.stack([o.pos_hist[:, i] for i in input_idx], dim=2).reshape(N * J, -1).abs() * abs(ps)
        vel = torch.stack([o.vel_hist[:, i] for i in input_idx], dim=2).reshape(N * J, -1).abs() * abs(vs)
        m = torch.cat([pos, vel], dim=1) if order == "pos_vel" else torch.cat([vel, pos], dim=1)
        for w, b in o.layers:
            m = m @ w.abs().t() + b.abs()
        terms = (m * abs(ts)).reshape(N, J)
        assert_close_terms(a.computed_effort, c64, terms, what + " computed")
        assert_close_terms(a.applied_effort, a64, terms, what + " applied")
    return f"mlp N={N} J={J} idx={input_idx} order={order} act={act} widths={widths}"


# ----------------------------------------------------------------------------------------------------------------- PD / DC motor
def pd_case(N, J, seed, dc=True):
    from isaaclab_amd.producers import PDActuator
    from oracle.producers_oracle import actuator_pd

    g = _gen(seed)
    rr = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    stiff, damp, elim, vlim = 20 + 80 * rr(N, J), 0.5 + 4 * rr(N, J), 40 + 60 * rr(N, J), 2 + 8 * rr(N, J)
    sat = 60.0  # below most effort limits: the saturation line, not the box, bounds the torque
    q_des, q, qd_des, ff = (torch.randn(N, J, generator=g) * 2.0 for _ in range(4))
    qd = _joint_vel(g, N, J, vlim) * 3.0
    qd.view(-1)[::5] = vlim.view(-1)[::5]
    qd.view(-1)[1::5] = -vlim.view(-1)[1::5]
    kw = dict(velocity_limit=vlim, saturation_effort=sat) if dc else {}
    c64, a64 = actuator_pd(*(t.to(F64) for t in (q_des, qd_des, ff, q, qd, stiff, damp, elim)),
                           **({"velocity_limit": vlim.to(F64), "saturation_effort": sat} if dc else {}))
    act = PDActuator(stiff.cuda(), damp.cuda(), elim.cuda(), **({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}))
    applied = act.compute(q_des.cuda(), q.cuda(), qd.cuda(), qd_des.cuda(), ff.cuda())
    what = f"pd N={N} J={J} dc={dc}"
    assert_close(act.computed_effort, c64, FLOAT_TOL, what + " computed")
    assert_close(applied, a64, FLOAT_TOL, what + " applied")
    if dc and N * J >= 64:
        assert bool((a64 > c64).any()) and bool((a64 < c64).any()), what + ": clip not active in both directions"
    return what


# ----------------------------------------------------------------------------------------------------------------- Delayed / remotized PD
def _lookup(g, K, dup):
    x = torch.sort(torch.rand(K, generator=g) * 3.0 - 1.5).values
    if dup and K >= 4:
        x[K // 2] = x[K // 2 - 1]  # a repeated angle: the torque limit jumps there (sorted, not strictly)
    y = 5.0 + 35.0 * torch.rand(K, generator=g)
    return torch.stack([x, torch.rand(K, generator=g), y], dim=1)


def delayed_case(N, J, min_delay, max_delay, K, seed, dup=True):
    """``K``: rows of the remotized lookup table (None = box-limited DelayedPDActuator).  Joint angles below, above and exactly on the
    table's samples; resets at steps that are not multiples of the ring length."""
    from isaaclab_amd.producers import DelayedPDActuator
    from oracle.producers_oracle import DelayedPDOracle

    g = _gen(seed)
    rr = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    stiff, damp, elim = 20 + 80 * rr(N, J), 0.5 + 4 * rr(N, J), 10 + 40 * rr(N, J)
    lookup = None if K is None else _lookup(g, K, dup)
    act = DelayedPDActuator(stiff.cuda(), damp.cuda(), min_delay, max_delay, effort_limit=elim.cuda(),
                            joint_parameter_lookup=None if lookup is None else lookup.cuda())
    o = DelayedPDOracle(N, J, max_delay, stiff.to(F64), damp.to(F64), elim.to(F64), None if lookup is None else lookup.to(F64))
    o.ring = o.ring.to(F64)
    L1 = max_delay + 1
    lags = torch.randint(min_delay, max_delay + 1, (N,), generator=g, dtype=torch.int32)
    lags[0], lags[-1] = min_delay, max_delay
    act.reset(None, lags.cuda())
    o.reset(torch.arange(N), lags)
    steps = 3 * L1 + 1
    reset_at = {s for s in (2, L1 + 1, 2 * L1 + 3) if s < steps and (L1 == 1 or s % L1)}
    for k in range(steps):
        if k in reset_at:
            ids = _subset(g, N, 0.4)
            lg = torch.randint(min_delay, max_delay + 1, (len(ids),), generator=g, dtype=torch.int32)
            act.reset(ids.cuda(), lg.cuda())
            o.reset(ids, lg)
        q_des, qd_des, ff = torch.randn(N, J, generator=g), torch.randn(N, J, generator=g), torch.randn(N, J, generator=g)
        q, qd = torch.randn(N, J, generator=g), torch.randn(N, J, generator=g)
        if lookup is not None:  # exactly on every sample, below the first, above the last
            x = lookup[:, 0]
            flat = q.view(-1)
            m = flat.numel()
            flat[: min(m, 3 * K):3] = x.repeat(3)[: len(range(0, min(m, 3 * K), 3))]
            if m > 3 * K + 2:
                flat[3 * K] = float(x[0]) - 0.75
                flat[3 * K + 1] = float(x[-1]) + 0.75
        applied = act.compute(q_des.cuda(), q.cuda(), qd.cuda(), qd_des.cuda(), ff.cuda())
        c64, a64 = o.compute(*(t.to(F64) for t in (q_des, qd_des, ff, q, qd)))
        what = f"delayed N={N} J={J} delay=[{min_delay}, {max_delay}] K={K} step {k}"
        assert_close(act.computed_effort, c64, FLOAT_TOL, what + " computed")
        assert_close(applied, a64, FLOAT_TOL, what + " applied")
        assert torch.equal(act.ring.cpu(), o.ring.float()), what + " delay ring"  # a fresh env's first sample fills every slot
    return f"delayed N={N} J={J} delay=[{min_delay}, {max_delay}] K={K} steps={steps}"


# ----------------------------------------------------------------------------------------------------------------- EmpiricalNormalization
def normalizer_case(D, batches, seed):
    """Batches of the given row counts through one normaliser; columns with |mean| up to 1e3 and std down to 1e-2."""
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
    from oracle.rsl_rl_oracle import EmpiricalNormalizationOracle

    g = _gen(seed)
    mu = torch.sign(torch.randn(D, generator=g)) * 10.0 ** (torch.rand(D, generator=g) * 4.0 - 1.0)
    sd = 10.0 ** (torch.rand(D, generator=g) * 2.5 - 2.0)
    mu[0], sd[0] = 1.0e3, 1.0e-2
    norm = EmpiricalNormalization([D]).cuda()
    o64, o32 = EmpiricalNormalizationOracle(D), EmpiricalNormalizationOracle(D)
    o64.mean, o64.var, o64.std = (t.to(F64) for t in (o64.mean, o64.var, o64.std))
    for k, N in enumerate(batches):
        x = (mu + sd * torch.randn(N, D, generator=g)).float()
        out = norm(x.cuda())
        check_normalizer_step(norm, out, o64, o32, x, f"normalizer D={D} batch {k} (N={N})")
    assert int(norm.count) == o64.count
    return f"normalizer D={D} batches={list(batches)}"


# ----------------------------------------------------------------------------------------------------------------- events
def events_case(N, J, NB, R, C, seed, body_ids=None, degenerate=False):
    from isaaclab_amd.events import ExternalForceTorque, ResetEvents, TerrainCurriculum
    from oracle import events_oracle as eo

    g = _gen(seed)
    rr = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    cu = lambda t: t.cuda()  # noqa: E731
    mask = rr(N) < 0.5
    mask[0] = True
    m8 = cu(mask.to(torch.uint8))
    # ---- reset_root_state_uniform + reset_joints_by_scale / _offset, push_by_setting_velocity
    pose_range = {"x": (-0.5, 0.5), "y": (-0.25, 0.75), "z": (0.1, 0.1) if degenerate else (0.0, 0.2), "roll": (-0.3, 0.3),
                  "pitch": (-0.2, 0.1), "yaw": (-3.14, 3.14)}
    vel_range = {"x": (-0.5, 0.5), "z": (0.2, 0.2) if degenerate else (-0.1, 0.3), "yaw": (-1.0, 1.0)}
    push_range = {"x": (-1.0, 1.0), "y": (0.3, 0.3) if degenerate else (-0.5, 0.5), "roll": (-0.1, 0.2)}
    drs = torch.randn(N, 13, generator=g)
    drs[:, 3:7] = torch.nn.functional.normalize(drs[:, 3:7], dim=1)
    org = torch.randn(N, 3, generator=g) * 4.0
    djp, djv = torch.randn(N, J, generator=g), torch.randn(N, J, generator=g)
    plim = torch.stack([-0.8 - rr(N, J), 0.8 + rr(N, J)], dim=-1)
    vlim = 0.5 + rr(N, J)
    for mode in ("scale", "offset"):
        jpr, jvr = ((0.5, 1.5), (-0.2, 0.4)) if mode == "scale" else ((-0.3, 0.3), (0.25, 0.25) if degenerate else (-1.0, 1.0))
        ev = ResetEvents(N, J, "cuda", pose_range, vel_range, jpr, jvr, mode, push_range)
        U = rr(N, 12 + 2 * J)
        pose, vel = torch.full((N, 7), 7.0, device="cuda"), torch.full((N, 6), 7.0, device="cuda")
        jp, jv = torch.full((N, J), 7.0, device="cuda"), torch.full((N, J), 7.0, device="cuda")
        ev.reset(m8, cu(drs), cu(org), pose, vel, cu(djp), cu(djv), cu(plim), cu(vlim), jp, jv, uniforms=cu(U))
        p64, v64 = eo.reset_root_state_uniform(drs.to(F64), org.to(F64), pose_range, vel_range, U[:, :6].to(F64), U[:, 6:12].to(F64))
        jp64, jv64 = eo.reset_joints(djp.to(F64), djv.to(F64), plim.to(F64), vlim.to(F64), jpr, jvr, U[:, 12:12 + J].to(F64),
                                     U[:, 12 + J:].to(F64), mode == "offset")
        what = f"reset N={N} J={J} {mode}"
        for got, ref, name in ((pose, p64, "pose"), (vel, v64, "velocity"), (jp, jp64, "joint pos"), (jv, jv64, "joint vel")):
            assert_close(got.cpu()[mask], ref[mask], FLOAT_TOL, f"{what} {name}")
            assert bool((got.cpu()[~mask] == 7.0).all()), f"{what} {name}: a row outside the mask was written"
        rv = torch.randn(N, 6, generator=g)
        v = cu(rv)
        Up = rr(N, 6)
        ev.push(m8, v, uniforms=cu(Up))
        ref = eo.push_by_setting_velocity(rv.to(F64), push_range, Up.to(F64))
        assert_close(v.cpu()[mask], ref[mask], FLOAT_TOL, f"push N={N}")
        assert torch.equal(v.cpu()[~mask], rv[~mask]), f"push N={N}: a row outside the mask was written"
    # ---- apply_external_force_torque on a body subset
    fr, tr = ((2.0, 2.0), (-1.0, -1.0)) if degenerate else ((-10.0, 10.0), (-2.0, 3.0))
    ids = list(range(NB)) if body_ids is None else list(body_ids)
    ext = ExternalForceTorque(N, NB, "cuda", fr, tr, body_ids=body_ids)
    forces, torques = torch.full((N, NB, 3), 9.0, device="cuda"), torch.full((N, NB, 3), 9.0, device="cuda")
    Uf = rr(2, N, len(ids), 3)
    ext.apply(m8, forces, torques, uniforms=cu(Uf))
    f64, t64 = eo.apply_external_force_torque(fr, tr, Uf[0].to(F64), Uf[1].to(F64))
    fc, tc = forces.cpu(), torques.cpu()
    assert_close(fc[mask][:, ids], f64[mask], FLOAT_TOL, f"external force N={N} bodies={ids}")
    assert_close(tc[mask][:, ids], t64[mask], FLOAT_TOL, f"external torque N={N} bodies={ids}")
    other = [b for b in range(NB) if b not in ids]
    assert bool((fc[:, other] == 9.0).all()) and bool((fc[~mask] == 9.0).all()) and bool((tc[~mask] == 9.0).all()), \
        f"external force N={N}: a body or row outside the selection was written"
    # ---- terrain_levels_vel + update_env_origins (random top-level draws fed)
    size_x, T = 16.0, 20.0
    origins_grid = torch.round(torch.randn(R, C, 3, generator=g) * 40.0) / 4.0  # quarter metres: origin + walk below is exact
    levels = torch.randint(0, R, (N,), generator=g)
    types = torch.randint(0, C, (N,), generator=g)
    levels[0], levels[-1] = 0, R - 1
    env_org = origins_grid[levels, types].clone()
    walk = torch.randn(N, 3, generator=g) * 6.0
    cmd = torch.randn(N, 3, generator=g)
    walk[0, :2], cmd[0, :2] = torch.tensor([0.5, 0.0]), torch.tensor([1.0, 0.0])   # level 0 moving down: stays at 0
    walk[-1, :2] = torch.tensor([9.0, 0.0])                                         # the last level moving up: a random level
    if N >= 4:
        walk[1, :2], cmd[1, :2] = torch.tensor([8.0, 0.0]), torch.tensor([0.0, 0.0])  # dist == size_x / 2: not up (strict >)
        walk[2, :2], cmd[2, :2] = torch.tensor([0.0, 5.0]), torch.tensor([0.5, 0.0])  # dist == |cmd| T / 2: not down (strict <)
        mask[1:3] = True
    mask[-1] = True
    root = env_org + walk
    rand = torch.randint(0, R, (N,), generator=g)
    lv_d, org_d = cu(levels.clone()), cu(env_org.clone())
    cur = TerrainCurriculum(cu(origins_grid), lv_d, cu(types), org_d, size_x, T)
    mean = cur.update(cu(mask.to(torch.uint8)), cu(root), cu(cmd), rand_levels=cu(rand))
    l64, o64, m64 = eo.terrain_levels_vel(mask, root.to(F64), env_org.to(F64), cmd.to(F64), origins_grid.to(F64), levels, types, size_x, T, rand)
    what = f"terrain N={N} R={R} C={C}"
    assert torch.equal(lv_d.cpu(), l64), what + " levels"
    assert torch.equal(org_d.cpu(), o64.float()), what + " env origins"
    assert_close(mean.cpu(), l64.to(F64).mean().reshape(1), FLOAT_TOL, what + " mean level")
    if N >= 4:
        assert int(lv_d[0]) == 0 and int(lv_d[1]) == int(levels[1]) and int(lv_d[2]) == int(levels[2]), what + " threshold cases"
    return f"events N={N} J={J} bodies={ids} of {NB} R={R} C={C} degenerate={degenerate}"


def run_child(cases: list[dict]) -> int:
    """The child-process side of the LSTM variant checks: run ``lstm_case`` on every dict, report, exit status 1 on the first failure."""
    kern = os.environ.get("IMX_LSTM_KERNEL", "")
    for kw in cases:
        try:
            print(f"IMX_LSTM_KERNEL={kern}: {lstm_case(**kw)}", flush=True)
        except AssertionError as exc:
            print(f"IMX_LSTM_KERNEL={kern}: FAIL {kw}: {exc}", flush=True)
            return 1
    return 0


def lstm_in_child(kernel: str, cases: list[dict], timeout: float = 300.0):
    """Run ``cases`` in a fresh interpreter with ``IMX_LSTM_KERNEL=kernel``.  -> (return code, output)."""
    import subprocess

    env = dict(os.environ, IMX_LSTM_KERNEL=kernel)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), json.dumps(cases)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout + p.stderr


def serve() -> int:
    """Persistent child for sweeps: one JSON dict of ``lstm_case`` keywords per input line, one ``@@ ok ...`` / ``@@ FAIL ...`` line back."""
    for line in sys.stdin:
        if not line.strip():
            continue
        try:
            msg = "@@ ok " + lstm_case(**json.loads(line))
        except AssertionError as exc:
            msg = "@@ FAIL " + " ".join(str(exc).split())
        print(msg, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(serve() if sys.argv[1:] == ["--serve"] else run_child(json.loads(sys.argv[1])))
