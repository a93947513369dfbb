"""The post-physics env step against ``OracleEnv`` in float64 (and in fp32, for the tolerance rule of tests/_util.py): cases shared by
tests/test_step_terms_gpu.py and tools/fuzz_cfg.py.

A case builds a ``ManagerBasedRLEnv`` from a cfg at N envs on a seeded ``StateFeed`` shaped by ``edge_pass`` (values on, just beside and
across every threshold the step decides on), primes ``episode_length_buf`` so that time-outs fall inside the run, and steps it with
non-zero noise uniforms.  The same inputs go through the oracle in float64 and in fp32.  Every reward term (raw value), the reward sum,
every episode sum, every observation term's column block in every group, the processed actions, every Episode_* log entry, the reset
count and ids, and the termination masks are compared per step."""

from __future__ import annotations

import copy
import numpy as np
import torch

from _util import FLOAT_TOL, STEP_ACOS_BAND, STEP_NEAR_FRACTION, STEP_SUM_FLOOR, STEP_TORCH_FACTOR, assert_close, assert_close_step
from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
from isaaclab_amd.plan import compile_plan, f32
from isaaclab_amd.robots import ROBOTS
from isaaclab_amd.state_feed import StateFeed
from isaaclab_amd.terrain import make_rough_terrain
from oracle.mdp_oracle import OracleEnv, _ids, quat_apply, quat_apply_yaw

ROUGH, FLAT, KITCHEN = "Isaac-Velocity-Rough-Anymal-C-v0", "Isaac-Velocity-Flat-Anymal-C-v0", "Isaac-Velocity-Rough-Anymal-C-v0-kitchen"
_CONTACT_FUNCS = ("illegal_contact", "undesired_contacts", "contact_forces", "feet_slide")


def _up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


# ------------------------------------------------------------------------------------------------ cfg variants
def variant(fx: dict, kind: str | None) -> dict:
    """A shipped cfg with one change that takes a kernel branch the shipped cfgs do not:
    ``single_reward`` one reward term and no termination term (k_term_rew with one work item: NW = 2);
    ``tilted`` rays 0.2 off the vertical, ``no_yaw`` a sensor frame that follows the full root rotation (the GENERAL_RAYS kernels);
    ``wide_rays`` a 3.3 x 3.3 m scan of 34 x 34 rays, too many for one single-wave workgroup per 64 rays, tilted (k_obs<true,true>);
    ``cols<n>`` the flat policy group padded with joint terms up to n computed columns (the obs block sizes)."""
    fx = copy.deepcopy(fx)
    env = fx["env"]
    if kind is None:
        return fx
    if kind == "single_reward":
        env["rewards"] = {"dof_acc_l2": env["rewards"]["dof_acc_l2"]}
        env["terminations"] = {}
    elif kind in ("tilted", "no_yaw", "wide_rays"):
        sc = env["scene"]["height_scanner"]
        if kind in ("tilted", "wide_rays"):
            sc["pattern_cfg"]["direction"] = [0.2, 0.0, -1.0]
        if kind == "no_yaw":
            sc["attach_yaw_only"] = False
        if kind == "wide_rays":
            sc["pattern_cfg"]["size"] = [3.3, 3.3]
    elif kind.startswith("cols"):
        target = int(kind[4:])
        pol = env["observations"]["policy"]
        J = 12
        width = sum({"base_lin_vel": 3, "base_ang_vel": 3, "projected_gravity": 3, "velocity_commands": 3, "joint_pos": J,
                     "joint_vel": J, "actions": J}.get(k, 0) for k, v in pol.items() if isinstance(v, dict))
        extra, i = target - width, 0
        pool = ["joint_pos_rel", "joint_vel_rel", "joint_pos_limit_normalized", "joint_pos", "joint_vel"]
        while extra > 0:  # repeated joint terms, then single joints for the remainder
            fn = pool[i % len(pool)]
            t = {"func": "isaaclab.envs.mdp.observations:" + fn, "params": {}, "noise": None, "clip": None, "scale": None}
            if extra < J:
                t["params"] = {"asset_cfg": {"name": "robot", "joint_names": [ROBOTS["anymal_c"].joint_names[k] for k in range(extra)],
                                             "preserve_order": False}}
            pol[f"pad{i}"] = t
            extra -= min(extra, J)
            i += 1
    else:
        raise ValueError(kind)
    return fx


def computed_columns(orc: OracleEnv, plan) -> int:
    """``plan.DC``: computed observation columns over every group (history windows count once: include/imx_internal.h)."""
    dc = 0
    for g, pg in zip(orc.obs_groups, plan.obs_groups):
        for (name, _), dims in zip(g["terms"], pg.term_dims):
            H = g["hist_len"].get(name, 0)
            dc += int(np.prod(dims)) // max(H, 1)
    return dc


# ------------------------------------------------------------------------------------------------ the edge pass
def _contact_terms(env_cfg: dict, robot):
    """(bodies, threshold) of every term that decides on the contact-force norm."""
    out = []
    for sec in ("rewards", "terminations"):
        for t in env_cfg[sec].values():
            if not t or t["func"].split(":")[-1] not in _CONTACT_FUNCS:
                continue
            if sec == "rewards" and t.get("weight") == 0.0:
                continue
            p = t.get("params") or {}
            e = dict(p["sensor_cfg"])
            e["_kind"] = "body"
            ids = _ids(e, robot.body_names)
            ids = list(range(robot.num_bodies)) if isinstance(ids, slice) else ids
            out.append((ids, f32(p.get("threshold", 1.0))))
    return out


def _param(env_cfg, fn, key, default=None):
    for sec in ("rewards", "terminations"):
        for t in env_cfg[sec].values():
            if t and t["func"].split(":")[-1] == fn and (sec == "terminations" or t.get("weight") != 0.0):
                return (t.get("params") or {}).get(key, default)
    return default


def edge_pass(feed: StateFeed, env_cfg: dict, robot, step_dt: float):
    """Put values on, one fp32 ulp either side of and across every threshold into some envs of every snapshot: env e gets edge kind
    e % 16 (ragged N: the kinds of the envs it has)."""
    st, sta, N = feed._stack, feed._static, feed.num_envs
    idx = torch.arange(N)
    kind = idx % 16
    lim = sta["soft_joint_pos_limits"]
    vlim = sta["soft_joint_vel_limits"]
    J = lim.shape[1]
    ratio = f32(_param(env_cfg, "joint_vel_limits", "soft_ratio", 1.0))
    contacts = _contact_terms(env_cfg, robot)
    p1 = f32(step_dt + 1.0e-8)
    hmin = _param(env_cfg, "root_height_below_minimum", "minimum_height")
    limit_angle = _param(env_cfg, "bad_orientation", "limit_angle", 0.4)
    for k in range(feed.num_snapshots):
        jp, jv = st["joint_pos"][k], st["joint_vel"][k]
        m = kind == 0  # on the soft limits, exactly
        jp[m] = torch.where(torch.arange(J) % 2 == 0, lim[m, :, 0], lim[m, :, 1])
        m = kind == 1  # below / above them
        jp[m] = torch.where(torch.arange(J) % 2 == 0, lim[m, :, 0] - 0.3, lim[m, :, 1] + 0.2)
        m = kind == 2  # |v| beyond soft limit x ratio by more than 1 (the clip at 1), either sign
        jv[m] = torch.where(torch.arange(J) % 2 == 0, 1.0, -1.0) * (vlim[m] * ratio + 1.5)
        ct, at = st["computed_torque"][k], st["applied_torque"][k]
        m = kind == 3  # applied == computed
        at[m] = ct[m]
        m = kind == 4  # within the isclose tolerance (|a-b| <= 1e-8 + 1e-5 |b|) by a factor 2, then beyond it by a factor 2
        at[m] = ct[m] + 0.5e-5 * ct[m].abs()
        m = kind == 5
        at[m] = ct[m] + 2e-5 * ct[m].abs() + 1e-7
        F = st["net_forces_w_history"][k]
        for kk, off in ((6, 0), (7, -1), (8, 1)):  # contact-force norm on a threshold, one ulp below, one ulp above
            m = (kind == kk).nonzero().flatten()
            for i, e in enumerate(m.tolist()):
                if not contacts:
                    break
                ids, th = contacts[(i + e // 16) % len(contacts)]
                v = th if off == 0 else (_down(th) if off < 0 else _up(th))
                F[e, :, ids] = 0.0
                F[e, 0, ids, 0] = v
                F[e, 1:, ids, 0] = v * 0.5
        cct = st["current_contact_time"][k]
        B = cct.shape[1]
        m = kind == 9  # first contact: exactly at f32(step_dt + 1e-8), one ulp below it, zero
        cct[m] = torch.tensor([p1, _down(p1), 0.0])[torch.arange(B) % 3]
        m = kind == 10
        cct[m] = torch.tensor([_down(p1), p1, 0.0, 1e-30])[torch.arange(B) % 4]
        z = st["root_pos_w"][k]
        if hmin is not None:
            z[kind == 11, 2] = f32(hmin)
            z[kind == 12, 2] = _down(hmin)
        q = st["root_quat_w"][k]
        m = kind == 13  # w < 0 (same rotation) and w == 0
        q[m] = -q[m]
        m = (kind == 12).nonzero().flatten()
        q[m] = torch.tensor([[0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.0]])[torch.arange(len(m)) % 2]
        m = (kind == 14).nonzero().flatten()  # tilt on both sides of limit_angle, 0.01 rad off it
        ang = torch.where(torch.arange(len(m)) % 2 == 0, limit_angle - 0.01, limit_angle + 0.01).double()
        q[m] = torch.stack([torch.cos(ang / 2), torch.sin(ang / 2), torch.zeros_like(ang), torch.zeros_like(ang)], dim=1).float()
        cmd = st["command"][k]
        m = kind == 15  # zero commands; |cmd_xy| exactly f32(0.1) (gate closed) and one ulp above it (open)
        cmd[m] = 0.0
        m = (kind == 14).nonzero().flatten()
        cmd[m, 0] = torch.tensor([f32(0.1), _up(0.1)])[torch.arange(len(m)) % 2]
        cmd[m, 1] = 0.0
    if "command_time_left" in st:
        st["command_time_left"][:, idx % 16 == 3] = f32(step_dt)


# ------------------------------------------------------------------------------------------------ one case
def _near_envs(orc64, out64, out32, step_dt):
    """Envs where a decision of the step sits within rounding of its threshold (tests/_util.py)."""
    near = out64["reset_buf"] != out32["reset_buf"]
    near |= out64["terminated"] != out32["terminated"]
    for name, t in orc64.term_cfgs:
        if t["func"].split(":")[-1] == "bad_orientation":
            ang = torch.acos(-orc64.projected_gravity_b[:, 2]).abs()
            near |= (ang - f32(t["params"]["limit_angle"])).abs() < STEP_ACOS_BAND
    # a reward gate that fp32 decides differently: the fp32 oracle is off by a whole term value, not by rounding
    bad = ((out32["step_reward"].double() - out64["step_reward"]).abs() > FLOAT_TOL * out64["step_reward"].abs().clamp(min=1.0)).any(1)
    return near | bad


def run_case(task, N, *, seed=0, steps=3, tail="deferred", kind=None, check=None, product=True):
    """One case (see the module doc).  ``task``: a shipped cfg's name or a fixture dict.  ``check`` collects coverage: kernel name,
    DC, seen gates.  ``product=False`` runs the fp32 oracle in place of the HIP path (a CPU dry run of the harness)."""
    fx = variant(load_task_cfg(task), kind) if isinstance(task, str) else copy.deepcopy(task)
    name = task if isinstance(task, str) else fx.get("task", "cfg")
    ecfg = fx["env"]
    robot = ROBOTS[fx["robot"]]
    scanner = (ecfg.get("scene") or {}).get("height_scanner")
    rough = scanner is not None and any(isinstance(g, dict) and any(isinstance(t, dict) and t.get("func", "").endswith("height_scan")
                                                                     for t in g.values()) for g in ecfg["observations"].values())
    terrain = ext = None
    if rough:
        v, t, e = make_rough_terrain(2, 3, tile=8.0, border=5.0, seed=seed % 7)
        terrain, ext = (v, t), (e[0] - 1.0, e[1] - 1.0)
    snaps = 3
    gen = torch.Generator().manual_seed(1000 + seed)
    feed = StateFeed(robot, N, "cpu", seed=seed + 17, num_snapshots=snaps, extent_xy=ext)
    step_dt = ecfg["sim"]["dt"] * ecfg["decimation"]
    edge_pass(feed, ecfg, robot, step_dt)
    plan = compile_plan(ecfg, robot)
    s64 = OracleEnv(ecfg, robot.joint_names, robot.body_names, N, feed.__getitem__, feed.gravity_dir, dtype=torch.float64)
    s32 = OracleEnv(ecfg, robot.joint_names, robot.body_names, N, feed.__getitem__, feed.gravity_dir)
    env = None
    W = plan.obs_dim_total
    if product:
        gfeed = StateFeed.from_tensors(robot, [feed.snapshot(i) for i in range(snaps)], "cuda:0", feed.gravity_dir)
        env = ManagerBasedRLEnv(fx, state_feed=gfeed, terrain=terrain, terrain_cell=0.1 if rough else 0.0)
        env.defer_step_tail = tail == "deferred"
        env.materialize_ray_hits = rough
        if check is not None:
            check["kernel"] = env._lib.imx_observations_kernel_name(env._plan_h).decode()
            check["DC"] = computed_columns(s64, env.plan)
            check["G"] = 16 if N <= 8192 else (32 if N <= 16384 else 64)
            check["items"] = len(env.plan.termination_terms) + len([t for t in env.plan.reward_terms])
        max_len = env.max_episode_length
    else:
        max_len = s64.max_episode_length
    u0 = torch.rand(N, W, generator=gen)
    ep = torch.randint(0, max_len, (N,), generator=gen)
    ep[::7] = max_len - 1
    ep[-1] = max_len - 1  # a time-out in the last group
    if product:
        env._noise_u = u0.cuda()
        env.reset()
        env.episode_length_buf = ep.cuda()
    for orc in (s64, s32):
        orc.reset_action_terms()
        orc.episode_length_buf[:] = ep
    hits = env._ray_hits.cpu() if (product and rough) else None
    for orc in (s64, s32):
        if hits is not None:
            orc.ray_hits_w = hits.to(orc.dtype)
            if env.plan.scan_stateful:
                orc.sensor_pos_w = _sensor_pos(env, orc.dtype)
        elif rough:
            orc.ray_hits_w = torch.zeros(N, plan.num_rays, 3, dtype=orc.dtype)
        orc.compute_observation_groups(u0)
    seen = dict(term_true={n: 0 for n, _ in s64.term_cfgs}, term_false={n: 0 for n, _ in s64.term_cfgs},
                rew_nonzero={n: 0 for n, _ in s64.rew_cfgs}, moving=[0, 0], first_contact=[0, 0], resets=0, near=0, steps=0)
    near = torch.zeros(N, dtype=torch.bool)
    fc_p1 = f32(step_dt + 1.0e-8)
    for k in range(steps):
        a = torch.randn(N, s64.A, generator=gen).clamp(-3, 3) * (1.0 if k % 2 == 0 else 0.3)
        a[idx_mod(N, 16, 15)] = 0.0
        u = torch.rand(N, W, generator=gen)
        for orc in (s64, s32):
            orc.process_action(a)
        feed.advance()
        if product:
            env._noise_u.copy_(u)
            obs_dict, rew, term, tout, extras = env.step(a.cuda())
            torch.cuda.synchronize()
            hits = env._ray_hits.cpu() if rough else None
        for orc in (s64, s32):
            if hits is not None:
                orc.ray_hits_w = hits.to(orc.dtype)
                if env.plan.scan_stateful:
                    orc.sensor_pos_w = _sensor_pos(env, orc.dtype)
        if product and rough and k == 0:
            _check_hits(env, feed, terrain, scanner)
        o64, o32 = s64.post_physics_step(u), s32.post_physics_step(u)
        near |= _near_envs(s64, o64, o32, step_dt)
        rows = ~near
        assert int(near.sum()) <= int(STEP_NEAR_FRACTION * N), f"{int(near.sum())} of {N} envs sit on a threshold"
        if not product:  # dry run: the fp32 oracle stands in for the kernels
            rew, term, tout = o32["reward"], o32["terminated"], o32["time_outs"]
            got = _oracle_outputs(s32, o32)
        else:
            got = _env_outputs(env, obs_dict, rew, extras)
        tag = f"{name}{'/' + kind if kind else ''} N={N} step {k}"
        # -- masks
        exp_term = torch.where(near, o32["terminated"], o64["terminated"])
        exp_tout = torch.where(near, o32["time_outs"], o64["time_outs"])
        assert torch.equal(term.cpu(), exp_term), f"{tag}: terminated differs at envs {(term.cpu() != exp_term).nonzero().flatten()[:8].tolist()}"
        assert torch.equal(tout.cpu(), exp_tout), f"{tag}: time_outs"
        exp_ids = torch.where(near, o32["reset_buf"], o64["reset_buf"]).nonzero().flatten()
        assert torch.equal(got["reset_env_ids"], exp_ids), f"{tag}: reset_env_ids ({len(got['reset_env_ids'])} vs {len(exp_ids)})"
        for i, (n, _) in enumerate(s64.term_cfgs):
            exp = torch.where(near, s32.term_dones[n], s64.term_dones[n])
            assert torch.equal(got["term_dones"][i], exp), f"{tag}: term_dones[{n}] differs at envs {(got['term_dones'][i] != exp).nonzero().flatten()[:8].tolist()}"
            seen["term_true"][n] += int(exp.sum())
            seen["term_false"][n] += int((~exp).sum())
        # -- rewards: every term's raw value, the sum, the episode sums
        for i, (n, t) in enumerate(s64.rew_cfgs):
            if t["weight"] == 0.0:
                continue
            w = f32(t["weight"])
            assert_close_step(got["step_reward"][:, i] / w, o64["step_reward"][:, i] / w, o32["step_reward"][:, i].double() / w,
                              f"{tag}: reward term {n}", rows)
            assert_close_step(got["episode_sums"][i], s64.episode_sums[n], s32.episode_sums[n], f"{tag}: episode sum {n}", rows)
            seen["rew_nonzero"][n] += int((o64["step_reward"][:, i] != 0).sum())
        assert_close_step(rew, o64["reward"], o32["reward"], f"{tag}: reward", rows)
        assert_close_step(got["processed_actions"], s64.processed_actions, s32.processed_actions, f"{tag}: processed actions", rows)
        # -- observations: every term's block in every group
        for g in s64.obs_groups:
            gname = g["name"]
            r64, r32, gg = o64["obs_groups"][gname], o32["obs_groups"][gname], got["obs"][gname]
            if isinstance(r64, dict):
                for tn in r64:
                    assert_close_step(gg[tn], r64[tn], r32[tn], f"{tag}: obs {gname}/{tn}", rows)
                continue
            if r64.dim() == 3:
                assert_close_step(gg, r64, r32, f"{tag}: obs {gname}", rows)
                continue
            c = 0
            for (tn, _), wd in zip(g["terms"], s64.group_term_widths[gname]):
                assert_close_step(gg[:, c:c + wd], r64[:, c:c + wd], r32[:, c:c + wd], f"{tag}: obs {gname}/{tn} cols {c}..{c + wd}", rows)
                c += wd
            assert c == r64.shape[1]
        # -- the step tail: reset count, ordered ids (above), Episode_* log
        ids64 = o64["reset_env_ids"]
        assert got["reset_count"] == len(exp_ids), f"{tag}: reset count"
        for key, v64 in o64["log"].items():
            v = float(got["log"][key])
            v32 = o32["log"][key]
            if key.startswith("Episode_Termination/"):
                assert v == (v32 if bool(near.any()) else v64), f"{tag}: {key} {v} vs {v64}"
                continue
            es = o64["episode_sums"][key[len("Episode_Reward/"):]][o64["reset_env_ids"]] if len(o64["reset_env_ids"]) else None
            floor = STEP_SUM_FLOOR * float(es.abs().mean()) / f32(s64.max_episode_length_s) if es is not None else 0.0
            bound = max(FLOAT_TOL * abs(v64), STEP_TORCH_FACTOR * abs(v32 - v64), floor)
            if bool(near.any()):
                bound = max(bound, FLOAT_TOL * max(abs(v32), 1.0) + abs(v32 - v64))
            assert abs(v - v64) <= bound, f"{tag}: {key} {v!r} vs fp64 {v64!r} (err {abs(v - v64):.3e}, bound {bound:.3e})"
        seen["resets"] += len(ids64)
        seen["near"] = int(near.sum())
        seen["steps"] += 1
        cmd = feed["command"]
        mv = cmd[:, :2].double().norm(dim=1) > f32(0.1)
        seen["moving"][0] += int((~mv).sum())
        seen["moving"][1] += int(mv.sum())
        cct = feed["current_contact_time"]
        fc = (cct > 0) & (cct < fc_p1)
        seen["first_contact"][0] += int((~fc).sum())
        seen["first_contact"][1] += int(fc.sum())
    if env is not None:
        env.close()
    if check is not None:
        check.update(seen)
    return seen


def idx_mod(N, m, r):
    return torch.arange(N) % m == r


def _sensor_pos(env, dtype):
    z = env._scan_state[:, 5].cpu().to(dtype)
    out = torch.zeros(z.shape[0], 3, dtype=dtype)
    out[:, 2] = z
    return out


def _check_hits(env, feed, terrain, scanner):
    """A slice of the HIP hits against the fp64 brute force over every triangle (the oracle takes the HIP hits)."""
    from oracle.raycast import raycast_f64

    ne, R = min(64, env.num_envs), env.plan.num_rays
    local = torch.from_numpy(env.plan.ray_starts_local).unsqueeze(0).repeat(ne, 1, 1)
    q = feed["root_quat_w"][:ne].repeat(1, R).reshape(ne, R, 4)
    rot = quat_apply_yaw if scanner.get("attach_yaw_only") else quat_apply
    starts = rot(q, local) + feed["root_pos_w"][:ne].unsqueeze(1)
    dirs = torch.tensor(env.plan.ray_direction, dtype=torch.float32).reshape(1, 1, 3).expand(ne, R, 3)
    if not scanner.get("attach_yaw_only"):
        dirs = quat_apply(q, dirs.contiguous())
    if env.plan.scan_stateful:  # drifting sensor: its hits are pinned by tests/test_env_gpu.py against the real reference
        return
    h64, _, _ = raycast_f64(terrain[0], terrain[1], starts.reshape(-1, 3).numpy(), dirs.reshape(-1, 3).numpy())
    assert_close(env._ray_hits[:ne].cpu().reshape(-1, 3), torch.from_numpy(h64), FLOAT_TOL, "ray hits vs fp64 brute force")


def _env_outputs(env, obs_dict, rew, extras):
    K = len(env.plan.reward_terms)
    return dict(step_reward=env._step_reward.cpu()[:, :K], episode_sums=env._episode_sums.cpu()[:K],
                term_dones=[env.termination_manager.get_term(n).cpu() for n in env.termination_manager.active_terms],
                processed_actions=env._processed_action.cpu()[:, :env.plan.action_dim],
                obs={g: (v.cpu() if torch.is_tensor(v) else {k: x.cpu() for k, x in v.items()}) for g, v in obs_dict.items()},
                reset_env_ids=env.reset_env_ids.cpu(), reset_count=int(env._counters[0].item()),
                log={k: float(v) for k, v in extras["log"].items()})


def _oracle_outputs(orc, out):
    return dict(step_reward=out["step_reward"], episode_sums=[orc.episode_sums[n] for n, _ in orc.rew_cfgs],
                term_dones=[orc.term_dones[n].clone() for n, _ in orc.term_cfgs], processed_actions=orc.processed_actions.clone(),
                obs=out["obs_groups"], reset_env_ids=out["reset_env_ids"], reset_count=len(out["reset_env_ids"]), log=out["log"])
