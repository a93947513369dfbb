"""Random sweep of the reset / interval orchestration launch (k_reset_orchestrate inside env.step() with the env's own EventManager /
CommandManager / CurriculumManager) against oracle/orchestration_oracle.py (pinned by the real-manager fixture): the fixture's cfg, scene
and state snapshots, but RANDOM draw tables, actions, episode lengths and step counts -- other reset patterns, timer phases, curriculum
moves and resampling sequences than the 48 recorded steps.  Simulator writes, trigger state, timers, levels / origins exact or 1e-5.
``one_case_pose`` is the same sweep over the Franka Reach cfg with the env's own UniformPoseCommand (``has_command = 2``).
``one_case_manip`` sweeps the manipulation launch (imx_reset_orchestrate_manip) on the Lift cfg against tests/_manip_orch_oracle.py:
random ranges, object defaults, thresholds and reset masks.
Test infrastructure, run on the GPU box:  python tools/fuzz_orchestration.py [cases] [seed] [pose|manip]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from _util import FLOAT_TOL, OrchGolden, assert_close
from isaaclab_amd.env import ManagerBasedRLEnv
from isaaclab_amd.events import TerrainImporterState
from oracle.orchestration_oracle import OrchestrationOracle

G = OrchGolden()


def random_draws(gen, rng):
    d = {}
    ref = G.draws(1)
    for n in G.term_names:
        d[n] = torch.rand(ref[n].shape, generator=gen)
    d["interval"] = torch.rand(ref["interval"].shape, generator=gen)
    d["command"] = torch.rand(ref["command"].shape, generator=gen)
    hi = int(G.t("draws/rand_levels").max()) + 1
    d["rand_levels"] = torch.randint(0, max(hi, 1), ref["rand_levels"].shape, generator=gen, dtype=ref["rand_levels"].dtype)
    return d


def feed_draws(env, d):
    for i, n in enumerate(G.interval_names):
        env.event_manager.get_term(n).interval_uniforms = d["interval"][i].cuda().contiguous()
    for n in G.term_names:
        env.event_manager.get_term(n).uniforms = d[n].cuda().contiguous()
    env._orch_draws["command"] = d["command"].cuda().contiguous()
    env._orch_draws["rand_levels"] = d["rand_levels"].cuda().contiguous()


def one_case(seed: int) -> str:
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    g, N, meta = G, G.N, G.meta
    ti = TerrainImporterState(g.t("terrain/origins").cuda(), g.t("terrain/levels0").cuda(), g.t("terrain/types").cuda(), meta["terrain"]["size_x"])
    env = ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"), own_managers=True, terrain_importer=ti)
    init = g.t("interval/time_left_init") * float(rng.choice([1.0, 0.3, 0.05]))  # other timer phases than the fixture's
    for i, n in enumerate(g.interval_names):
        t = env.event_manager.get_term(n)
        t.time_left.copy_((init[i][:1].repeat(2) if t.is_global_time else init[i]).cuda())
    orc = OrchestrationOracle(g.fixture["env"], N, g.robot.num_joints, g.robot.body_names, meta["step_dt"], meta["max_episode_length_s"],
                              g.t("static/default_root_state"), g.t("static/default_joint_pos"), g.t("static/default_joint_vel"),
                              g.t("static/soft_joint_pos_limits"), g.t("static/soft_joint_vel_limits"), g.t("terrain/origins"),
                              g.t("terrain/levels0"), g.t("terrain/types"), meta["terrain"]["size_x"], init)
    cpu_feed = g.feed("cpu")
    ev, ct = env.event_manager, env.command_term

    def state():
        return {k: cpu_feed[k] for k in ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w")}

    def check(tag):
        torch.cuda.synchronize()
        for k, v in env.sim_writes.items():
            assert_close(v, orc.sim_writes[k], FLOAT_TOL, f"{tag} sim_writes[{k}]")
        assert torch.equal(ti.terrain_levels.cpu(), orc.levels), f"{tag} terrain levels"
        assert torch.equal(ti.env_origins.cpu(), orc.env_origins), f"{tag} env origins"
        c = orc.cmd
        for k, a, b in (("command", ct.vel_command_b, c.vel_command_b), ("time_left", ct.time_left, c.time_left), ("heading", ct.heading_target, c.heading_target),
                        ("error_vel_xy", ct.metrics["error_vel_xy"], c.metrics["error_vel_xy"]), ("error_vel_yaw", ct.metrics["error_vel_yaw"], c.metrics["error_vel_yaw"])):
            assert_close(a, b, FLOAT_TOL, f"{tag} command {k}")
        assert torch.equal(ct.command_counter.cpu(), c.command_counter) and torch.equal(ct.is_standing_env.cpu(), c.is_standing_env), f"{tag} command flags"
        step = int(env._counters[2])
        tl = torch.stack([(t.time_left[(step + 1) & 1].expand(N) if t.is_global_time else t.time_left) for t in (ev.get_term(n) for n in g.interval_names)])
        assert_close(tl, torch.stack([orc.time_left[n].expand(N) for n in g.interval_names]), 1e-6, f"{tag} interval timers")
        assert torch.equal(torch.stack([ev.get_term(n).last_triggered_step for n in g.reset_names]).cpu(), torch.stack([orc.last_triggered[n] for n in g.reset_names])), f"{tag} last triggered"
        assert torch.equal(torch.stack([ev.get_term(n).triggered_once for n in g.reset_names]).cpu(), torch.stack([orc.triggered_once[n] for n in g.reset_names])), f"{tag} triggered once"

    d = random_draws(gen, rng)
    feed_draws(env, d)
    env.reset()
    orc.cmd._draw[:] = 0
    orc.reset_idx(torch.arange(N), state(), 0, d, d["command"], d["rand_levels"])
    check("reset")
    ep = torch.randint(0, env.max_episode_length, (N,), generator=gen)
    ep[:: int(rng.choice([2, 3, 7]))] = env.max_episode_length - int(rng.integers(1, 4))
    env.episode_length_buf = ep
    steps = int(rng.integers(5, 40))
    resets = pushes = 0
    scale = float(rng.choice([0.2, 1.0, 3.0]))
    for s in range(steps):
        d = random_draws(gen, rng)
        feed_draws(env, d)
        env.step((torch.randn(N, env.plan.action_dim, generator=gen) * scale).clamp(-3, 3).cuda())
        cpu_feed.advance()
        ids = env.reset_env_ids.cpu()
        orc.cmd._draw[:] = 0
        if len(ids):
            orc.reset_idx(ids, state(), s + 1, d, d["command"], d["rand_levels"])
            resets += len(ids)
        fired = orc.step_tail(state(), d, d["interval"], d["command"])
        pushes += sum(len(v) for v in fired.values())
        check(f"step {s}")
    env.close()
    return f"steps={steps} resets={resets} pushes={pushes} mean level {float(orc.levels.float().mean()):.2f}"


_RG = None


def one_case_pose(seed: int) -> str:
    """The same launch with ``has_command = 2``: the Franka Reach cfg of tests/golden/reach_orchestration.json (UniformPoseCommand +
    reset_joints_by_scale) with RANDOM draw tables, actions, episode lengths and step counts, against tests/_pose_command_oracle.py and
    oracle/events_oracle.py.  A separate entry point: ``one_case`` consumes its generators exactly as before."""
    global _RG
    from _pose_command_cases import ReachOrchGolden, w_margin_ok
    from _pose_command_oracle import PoseCommandOracle
    from oracle import events_oracle as evo

    g = _RG = _RG or ReachOrchGolden()
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    N, J, meta = g.N, g.robot.num_joints, g.meta
    fx = g.fixture
    ccfg = dict(fx["env"]["commands"]["ee_pose"])
    if rng.integers(0, 2):  # the other branch of _resample_command: every angle free, quat_unique
        ccfg["make_quat_unique"] = True
        ccfg["ranges"] = dict(ccfg["ranges"], roll=(-3.14, 3.14), pitch=(-3.14, 3.14))
    lo = float(rng.choice([0.5, 2.0, 5.0])) * meta["step_dt"]  # 0.5: reset and timer resample in one step (draw 1)
    ccfg["resampling_time_range"] = (lo, lo * float(rng.choice([1.0, 2.0, 3.0])))
    fx = dict(fx, env=dict(fx["env"], commands={"ee_pose": ccfg}))
    env = ManagerBasedRLEnv(fx, state_feed=g.feed("cuda:0"), own_managers=True)
    cpu_feed = g.feed("cpu")
    ct, term = env.command_term, env.event_manager.get_term("reset_robot_joints")
    orc = PoseCommandOracle(ccfg, N, meta["step_dt"], ct.body_idx)
    p = fx["env"]["events"]["reset_robot_joints"]["params"]
    djp, djv, plim, vlim = (g.t("static/" + n) for n in ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits"))
    joint_pos, joint_vel = torch.zeros(N, J), torch.zeros(N, J)

    def draws():
        d = {"reset_robot_joints": torch.rand(N, 2 * J, generator=gen), "command": torch.rand(2, N, 7, generator=gen)}
        while ccfg.get("make_quat_unique") and not w_margin_ok(ccfg, d["command"]):
            d["command"] = torch.rand(2, N, 7, generator=gen)
        term.uniforms = d["reset_robot_joints"].cuda().contiguous()
        env._orch_draws["command"] = d["command"].cuda().contiguous()
        return d

    def run_oracle(mask, d, do_compute):
        ids = mask.nonzero().flatten()
        if len(ids):  # reset_joints_by_scale (events.py:987-1021); no min_step_count_between_reset: every reset env is valid
            u = d["reset_robot_joints"]
            joint_pos[ids], joint_vel[ids] = evo.reset_joints(djp[ids], djv[ids], plim[ids], vlim[ids], tuple(p["position_range"]),
                                                              tuple(p["velocity_range"]), u[ids, :J], u[ids, J:2 * J], by_offset=False)
        f = cpu_feed
        orc.reset_and_compute(meta["step_dt"], f["root_pos_w"], f["root_quat_w"], f["body_pos_w"], f["body_quat_w"], mask, d["command"],
                              do_compute=do_compute)

    def check(tag):
        torch.cuda.synchronize()
        assert_close(env.sim_writes["joint_pos"], joint_pos, FLOAT_TOL, f"{tag} sim_writes[joint_pos]")
        assert_close(env.sim_writes["joint_vel"], joint_vel, FLOAT_TOL, f"{tag} sim_writes[joint_vel]")
        for k, a, b in (("command", ct.command, orc.command), ("pose_command_w", ct.pose_command_w, orc.pose_command_w),
                        ("time_left", ct.time_left, orc.time_left), ("position_error", ct.metrics["position_error"], orc.metrics["position_error"]),
                        ("orientation_error", ct.metrics["orientation_error"], orc.metrics["orientation_error"])):
            assert_close(a, b, FLOAT_TOL, f"{tag} {k}")
        assert torch.equal(ct.command_counter.cpu(), orc.command_counter), f"{tag} command counter"

    d = draws()
    env.reset()
    run_oracle(torch.ones(N, dtype=torch.bool), d, False)
    check("reset")
    ep = torch.randint(0, env.max_episode_length, (N,), generator=gen)
    ep[:: int(rng.choice([2, 3, 7]))] = env.max_episode_length - int(rng.integers(1, 4))
    env.episode_length_buf = ep
    steps = int(rng.integers(5, 40))
    resets = twice = 0
    for s in range(steps):
        d = draws()
        _, _, _, _, extras = env.step((torch.randn(N, env.plan.action_dim, generator=gen)).clamp(-3, 3).cuda())
        cpu_feed.advance()
        mask = torch.zeros(N, dtype=torch.bool)
        mask[env.reset_env_ids.cpu()] = True
        logged = {m: float(torch.mean(v[mask])) for m, v in orc.metrics.items()} if mask.any() else {}
        run_oracle(mask, d, True)
        resets += int(mask.sum())
        twice += int((orc._draw == 2).sum())
        check(f"step {s}")
        for m, v in logged.items():  # CommandTerm.reset logs the mean over the reset envs before zeroing
            got = float(extras["log"][f"Metrics/ee_pose/{m}"])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (s, m, got, v)
    env.close()
    return f"steps={steps} resets={resets} resampled twice in a step={twice} unique={bool(ccfg.get('make_quat_unique'))} resample={ccfg['resampling_time_range']}"


_MG = None


def one_case_manip(seed: int) -> str:
    """``imx_reset_orchestrate_manip`` alone (``env._orchestrate`` on a mask of the case's own) on the Lift cfg of
    tests/golden/lift_manip_orchestration.json: reset_scene_to_default, reset_root_state_uniform on the object and two modify_reward_weight
    terms with RANDOM pose / velocity ranges on all six axes, object defaults (rotated), env origins, thresholds, step counts and reset
    masks (all false and all true among them), N not a multiple of 64.  Rows that did not reset must keep their bits (NaN-filled)."""
    global _MG
    import copy

    import _manip_orch_oracle as mo
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    g = _MG = _MG or mo.ManipOrchGolden("lift")
    rng = np.random.default_rng(seed)
    N = int(rng.choice([1, 63, 64, 65, 100, 257]))
    fx = copy.deepcopy(g.fixture)
    e = fx["env"]
    pr = {a: tuple(sorted(rng.uniform(-1.5, 1.5, 2).tolist())) for a in mo.AXES}
    vr = {a: tuple(sorted(rng.uniform(-1.0, 1.0, 2).tolist())) for a in mo.AXES}
    e["events"]["reset_object_position"]["params"].update(pose_range=pr, velocity_range=vr)
    q = rng.normal(size=4)
    e["scene"]["object"]["init_state"].update(pos=rng.normal(size=3).tolist(), rot=(q / np.linalg.norm(q)).tolist(),
                                              lin_vel=rng.normal(size=3).tolist(), ang_vel=rng.normal(size=3).tolist())
    thr = [int(x) for x in rng.integers(0, 30, 2)]
    new_w = [float(x) for x in rng.uniform(-2, 2, 2)]
    for (name, c), t_, w_ in zip(e["curriculum"].items(), thr, new_w):
        c["params"].update(num_steps=t_, weight=w_)
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=int(rng.integers(0, 1 << 30)), num_snapshots=2)
    env = ManagerBasedRLEnv(fx, state_feed=feed, own_managers=True, reward_curriculum=True, num_envs=N)
    st = {k: feed[k].cpu().numpy() for k in ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits", "env_origins")}
    st["default_root_state"], st["default_object_root_state"] = env.default_root_state.cpu().numpy(), env.default_object_root_state.cpu().numpy()
    events = {k: v for k, v in e["events"].items() if v is not None and v.get("mode") == "reset"}
    cur = [(c["params"]["term_name"], np.float32(c["params"]["weight"]).item(), c["params"]["num_steps"]) for c in e["curriculum"].values()]
    weights = {n: np.float32(t["weight"]).item() for n, t in e["rewards"].items() if t is not None}
    nan = torch.tensor(0x7FC0BEEF, dtype=torch.int32).view(torch.float32).item()
    keys = ("root_pose", "root_vel", "joint_pos", "joint_vel", "object_root_pose", "object_root_vel")
    sw = {}
    for k in keys:
        env.sim_writes[k].fill_(nan)
        sw[k] = env.sim_writes[k].cpu().numpy().copy()
    trig = {"last": np.zeros((2, N), np.int64), "once": np.zeros((2, N), bool)}
    kinds = ["none", "all", "some", "last", "some", "none", "some"]
    switched = 0
    for it, kind in enumerate(kinds):
        step = int(rng.integers(0, 40))
        mask = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "last": np.arange(N) == N - 1}.get(kind)
        mask = rng.random(N) < 0.3 if mask is None else mask
        u = rng.random((N, 12), np.float32)
        env._counters[2] = step
        env.event_manager.get_term("reset_object_position").uniforms = torch.from_numpy(u).cuda()
        env._orchestrate(torch.from_numpy(mask).cuda(), do_step=False)
        ids = np.nonzero(mask)[0]
        before = dict(weights)
        weights = mo.modify_reward_weight(weights, step, len(ids) > 0, cur)
        switched += sum(weights[n] != before[n] for n in weights)
        if len(ids):
            mo.apply_reset_events(events, ids, step, sw, trig, st, {"reset_object_position": u}, "object")
        torch.cuda.synchronize()
        for k in keys:
            got = env.sim_writes[k].cpu().numpy()
            assert np.array_equal(got[~mask].view(np.int32), sw[k][~mask].view(np.int32)), f"{it} {kind}: sim_writes[{k}] changed a row that did not reset"
            assert_close(got[mask], sw[k][mask], FLOAT_TOL, f"{it} {kind} sim_writes[{k}]")
            sw[k][mask] = got[mask]  # (the kernel's own bits from here on: the next comparison of untouched rows is exact)
        for k_, t in enumerate(env.event_manager.terms):
            assert np.array_equal(t.last_triggered_step.cpu().numpy(), trig["last"][k_]) and np.array_equal(t.triggered_once.cpu().numpy(), trig["once"][k_]), (it, t.name)
        for n, w in weights.items():
            got = float(env.reward_manager.get_term_cfg(n).weight)
            assert np.float32(got) == np.float32(w), (it, kind, step, n, got, w)
    env.close()
    return f"N={N} thresholds={thr} weight switches={switched}"


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    pose = "pose" in sys.argv[3:]
    one_case = one_case_manip if "manip" in sys.argv[3:] else one_case_pose if pose else one_case
    bad = 0
    for c in range(first, first + cases):
        try:
            print(f"case {c}: ok   {one_case(c)}", flush=True)
        except AssertionError as e:
            bad += 1
            print(f"case {c}: FAIL {str(e)[:400]}", flush=True)
    print(f"{cases - bad} / {cases} cases agree")
    sys.exit(1 if bad else 0)
