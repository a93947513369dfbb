"""GPU: the pose-2d command producers (``imx_pose2d_command``) against the fixtures of the REAL ``UniformPose2dCommand`` /
``TerrainBasedPose2dCommand``, the orchestration launch ``imx_reset_orchestrate_pose2d`` against the REAL ``_reset_idx`` + CommandManager +
EventManager of ``NavigationEnvCfg`` (tests/golden/navigation_orchestration*.npz, tools/gen_golden_pose2d_command.py), and the env that
runs it (``command_term=<a producers.UniformPose2dCommand>``)."""

import ctypes

import numpy as np
import pytest
import torch

from _pose2d_cases import OUT_KEYS, VARIANTS, NavOrchGolden, Pose2dGolden, assert_outputs_close, term_outputs, wrap_to_pi, zero_struct
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ the stand-alone kernel
@pytest.mark.parametrize("n", [300, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_matches_reference(variant, n):
    """All 12 steps in parity mode, the fixture cut to its first n envs (wave and 256-thread block edges): counters bit for bit, floats
    within FLOAT_TOL (the figure of tests/test_pose_command_gpu.py), heading_command_w on the circle.  error_pos stays zero."""
    g = Pose2dGolden(variant)
    term = g.producer(DEV, n)
    assert list(term.metrics) == ["error_pos", "error_heading"]
    for k in range(g.steps):
        d = {a: (b.to(DEV) if b is not None else None) for a, b in g.inputs(k, n).items()}
        term.compute(g.step_dt, d["reset_mask"], d["uniforms"], d["patch_ids"], d["root_pos_w"], d["root_quat_w"])
        assert list(term.metrics) == g.meta["metrics"]
        got, ref = term_outputs(term), g.expected(k, n)
        for name in OUT_KEYS:  # every figure is printed before it is held to its bound
            if name != "command_counter":
                a, b = got[name].cpu().double(), ref[name].double()
                e = wrap_to_pi(a - b).abs() if name == "heading_command_w" else (a - b).abs()
                print(f"{variant} n={n} step {k} {name}: max err {float(e.max()):.3e}")
        assert_outputs_close(got, ref, FLOAT_TOL, f"{variant} n={n} step {k}")
    assert float(term.metrics["error_pos"].abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["U0", "U1", "T1"])
def test_in_kernel_draws(variant):
    """No tables: the counter-based generator.  Same seed and step give the same run; the values lie inside the cfg's ranges, differ
    across envs, and a terrain-based target is always one of the P patches of the env's own cell (id < P)."""
    g = Pose2dGolden(variant)
    N = 257
    d = {a: (b.to(DEV) if b is not None else None) for a, b in g.inputs(0, N).items()}
    runs = []
    for seed in (5, 5, 6):
        term = g.producer(DEV, N, seed=seed)
        for _ in range(3):  # every env is reset in each call, then computed: two draws per env and call
            term.compute(g.step_dt, torch.ones(N, dtype=torch.bool, device=DEV), None, None, d["root_pos_w"], d["root_quat_w"])
        runs.append({k: v.clone() for k, v in term_outputs(term).items()})
    for k in OUT_KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: same seed, same run"
    assert not torch.equal(runs[0]["pos_command_w"], runs[2]["pos_command_w"])
    out, cfg, c = runs[0], g.cfg, g.constants(N)
    lo, hi = cfg["resampling_time_range"]
    tl = out["time_left"].cpu()
    assert float(tl.min()) >= lo - g.step_dt - 1e-6 and float(tl.max()) <= hi - g.step_dt + 1e-6 and len(tl.unique()) > N // 2
    assert bool((out["command_counter"] == 1).all())
    pw = out["pos_command_w"].cpu()
    if g.kind == 0:
        assert torch.equal(pw[:, 2], c["env_origins"][:, 2] + c["default_root_z"])
        off = pw[:, :2] - c["env_origins"][:, :2]
        for j, name in enumerate(("pos_x", "pos_y")):
            r = cfg["ranges"][name]
            assert float(off[:, j].min()) >= r[0] - 1e-5 and float(off[:, j].max()) <= r[1] + 1e-5 and len(off[:, j].unique()) > N // 2
    else:  # the target is a patch of the env's own terrain cell
        cell = c["valid_targets"][c["terrain_levels"], c["terrain_types"]]  # (N, P, 3)
        cell = cell + torch.cat([torch.zeros(N, 2), c["default_root_z"][:, None]], dim=1)[:, None, :]
        hit = (cell == pw[:, None, :]).all(dim=-1)
        assert bool(hit.any(dim=-1).all()), "a target outside the env's cell: a patch id >= P or a wrong cell"
        assert len(hit.float().argmax(dim=-1).unique()) == cell.shape[1], "every patch id is drawn"
    hw = out["heading_command_w"].cpu()
    if not cfg["simple_heading"]:
        r = cfg["ranges"]["heading"]
        assert float(hw.min()) >= r[0] - 1e-6 and float(hw.max()) <= r[1] + 1e-6 and len(hw.unique()) > N // 2
    else:
        assert float(hw.abs().max()) <= np.pi + 1e-6


def test_producer_reset_and_compute_stand_alone():
    """``reset(env_ids)`` / ``compute(dt)`` with ``robot=``: reset resamples only those envs and returns the reference's log entries."""
    import types

    from isaaclab_amd import producers

    g = Pose2dGolden("U0")
    N = 65
    d = {a: (b.to(DEV) if b is not None else None) for a, b in g.inputs(0, N).items()}
    robot = types.SimpleNamespace(data=types.SimpleNamespace(root_pos_w=d["root_pos_w"], root_quat_w=d["root_quat_w"]))
    c = {k: v.to(DEV) for k, v in g.constants(N).items()}
    term = producers.UniformPose2dCommand(g.cfg, N, g.step_dt, DEV, seed=3, robot=robot, **c)
    log = term.reset()
    assert list(log) == ["error_pos", "error_heading"] and bool((term.command_counter == 1).all())
    assert float(term.command.abs().max()) == 0.0  # (the command is written by compute)
    term.compute(g.step_dt)
    assert float(term.command.abs().max()) > 0.0 and list(term.metrics)[-1] == "error_pos_2d"
    before = term.pos_command_w.clone()
    ids = torch.tensor([0, 7, 64], device=DEV)
    log = term.reset(ids)
    assert list(log) == ["error_pos", "error_heading", "error_pos_2d"] and log["error_pos"] == 0.0 and log["error_pos_2d"] > 0.0
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[ids] = False
    assert torch.equal(term.pos_command_w[keep], before[keep]) and bool((term.pos_command_w[ids] != before[ids]).any(dim=-1).all())
    assert float(term.metrics["error_pos_2d"][ids].abs().max()) == 0.0 and bool((term.command_counter[ids] == 1).all())


# ------------------------------------------------------------------------------------------------ the orchestration launch
def _orch(N, t, **over):
    from isaaclab_amd._lib import ImxOrch

    o = ImxOrch(num_envs=N, num_joints=1, num_bodies=1, dt=0.2, do_step=1, env_origins_d=t["org"].data_ptr(), has_command=0,
                root_pos_w_d=t["rp"].data_ptr(), root_quat_w_d=t["rq"].data_ptr(), step_counter_d=t["step"].data_ptr(), ev_part_d=t["part"].data_ptr())
    for k, v in over.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("variant", ["U0", "U1", "T1"])
@pytest.mark.parametrize("tables", [True, False])
def test_orchestration_launch_equals_the_stand_alone_kernel(variant, tables):
    """The same inputs, reset masks and draws (the recorded tables, or the in-kernel generator on the same seed and step) through
    ``imx_reset_orchestrate_pose2d`` (no event terms) and through ``imx_pose2d_command``: every buffer bit for bit, kind 0 and kind 1; the
    launch's ev_part columns 0 / 1 hold the metric sums over the reset envs."""
    from isaaclab_amd import _lib

    g = Pose2dGolden(variant)
    N, L = g.N, _lib.lib()
    a, b = g.producer(DEV, seed=9), g.producer(DEV, seed=9)
    t = dict(org=g.constants()["env_origins"].to(DEV), step=torch.zeros(1, dtype=torch.int32, device=DEV),
             part=torch.zeros(int(L.imx_orch_part_floats(N)), device=DEV))
    seed = 0x5EED
    for k in range(4):
        d = {x: (y.to(DEV) if y is not None else None) for x, y in g.inputs(k).items()}
        U, ids = (d["uniforms"], d["patch_ids"]) if tables else (None, None)
        mask = d["reset_mask"].to(torch.uint8)
        t.update(rp=d["root_pos_w"], rq=d["root_quat_w"])
        t["step"].fill_(k + 1)
        before = (a._error_pos_2d.clone(), a.metrics["error_heading"].clone())
        o = _orch(N, t, dt=g.step_dt, reset_mask_d=mask.data_ptr(), seed=seed)
        ca, cb = a.struct(U, ids), b.struct(U, ids)
        _lib.check(L.imx_reset_orchestrate_pose2d(ctypes.byref(o), ctypes.byref(ca), _lib.current_stream(torch.device(DEV))))
        _lib.check(L.imx_pose2d_command(N, ctypes.byref(cb), g.step_dt, 1, d["root_pos_w"].data_ptr(), d["root_quat_w"].data_ptr(), mask.data_ptr(),
                                        seed ^ 0xC0FFEE, t["step"].data_ptr(), _lib.current_stream(torch.device(DEV))))
        torch.cuda.synchronize()
        for x, y, name in ((a.command, b.command, "command"), (a.pos_command_w, b.pos_command_w, "pos_command_w"),
                           (a.heading_command_w, b.heading_command_w, "heading_command_w"), (a.time_left, b.time_left, "time_left"),
                           (a.command_counter, b.command_counter, "command_counter"), (a._error_pos_2d, b._error_pos_2d, "error_pos_2d"),
                           (a.metrics["error_heading"], b.metrics["error_heading"], "error_heading")):
            assert torch.equal(x, y), f"{variant} step {k} {name}: the orchestration launch and the stand-alone kernel differ"
        part = t["part"].view(-1, 4).cpu()
        m = d["reset_mask"].cpu()
        assert_close(part[:, 3].sum(), m.sum().float(), 0.0, "reset count")
        for col, v in enumerate(before):
            assert_close(part[:, col].sum(), v.cpu()[m].double().sum().float(), FLOAT_TOL, f"ev_part column {col}")
        if tables:
            a.mark_computed()
            assert_outputs_close(term_outputs(a), g.expected(k), FLOAT_TOL, f"{variant} launch step {k}")


def test_entry_points_name_what_is_missing():
    """One call each on valid zero buffers, N = 8: every NULL pointer or bad value is refused and named; nothing is launched."""
    from isaaclab_amd import _lib

    N, L = 8, _lib.lib()
    stream = _lib.current_stream(torch.device(DEV))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    t = dict(org=z(N, 3), rp=z(N, 3), rq=z(N, 4), step=z(1, dt=torch.int32), part=z(int(L.imx_orch_part_floats(N))),
             lv=z(N, dt=torch.long), ty=z(N, dt=torch.long), to=z(2, 2, 3), vc=z(N, 3))
    t["rq"][:, 0] = 1.0

    def alone(c, **over):
        kw = dict(N=N, root_pos=t["rp"].data_ptr(), root_quat=t["rq"].data_ptr())
        kw.update(over)
        return L.imx_pose2d_command(kw["N"], ctypes.byref(c) if c is not None else None, 0.2, 1, kw["root_pos"], kw["root_quat"], None, 0, None, stream)

    def launch(c, **over):
        o = _orch(N, t, **over)
        return L.imx_reset_orchestrate_pose2d(ctypes.byref(o), ctypes.byref(c) if c is not None else None, stream)

    def refused(rc, word):
        msg = L.imx_last_error().decode()
        assert rc != 0 and word in msg, (word, msg)

    untouched = []  # the buffers of every struct a refused call was given
    cases = [(0, dict(kind=2), "kind"), (0, dict(kind=-1), "kind"), (0, dict(env_origins_d=None), "env_origins"),
             (0, dict(default_root_z_d=None), "default_root_z"), (0, dict(command_d=None), "command missing"),
             (0, dict(pos_command_w_d=None), "pos_command_w"), (0, dict(heading_command_w_d=None), "heading_command_w"),
             (0, dict(time_left_d=None), "time_left"), (0, dict(command_counter_d=None), "command_counter"),
             (0, dict(metric_error_pos_2d_d=None), "error_pos_2d"), (0, dict(metric_error_heading_d=None), "error_heading"),
             (1, dict(valid_targets_d=None), "valid_targets"), (1, dict(terrain_levels_d=None), "terrain_levels"),
             (1, dict(terrain_types_d=None), "terrain_types"), (1, dict(num_patches=0), "num_patches"), (1, dict(num_levels=-1), "num_levels")]
    for kind, over, word in cases:
        for run, who in ((alone, "imx_pose2d_command"), (launch, "imx_reset_orchestrate_pose2d")):
            c, keep = zero_struct(N, DEV, kind)
            untouched.append(keep)
            for k, v in over.items():
                setattr(c, k, v)
            refused(run(c), word)
            assert who in L.imx_last_error().decode()
    for run in (alone, launch):
        c, keep = zero_struct(N, DEV)
        untouched.append(keep)
        c.cfg[1] = 0.0
        refused(run(c), "resampling_time_range")
        refused(run(None), "null imx_pose2d_command_t")
    c, keep = zero_struct(N, DEV)
    untouched.append(keep)
    refused(alone(c, N=0), "N out of range")
    refused(alone(c, root_pos=None), "root_pos_w")
    refused(alone(c, root_quat=None), "root_quat_w")
    refused(launch(c, root_pos_w_d=None), "root_pos_w")
    refused(launch(c, root_quat_w_d=None), "root_quat_w")
    refused(launch(c, env_origins_d=None), "env_origins")
    refused(launch(c, num_envs=0), "num_envs")
    for hc in (1, 2, 3):
        refused(launch(c, has_command=hc), "has_command")
    refused(launch(c, terrain_levels_d=t["lv"].data_ptr(), terrain_types_d=t["ty"].data_ptr(), terrain_origins_d=t["to"].data_ptr(),
                   terrain_rows=2, terrain_cols=2, vel_command_b_d=t["vc"].data_ptr()), "terrain curriculum")
    # the other entry point still refuses a fourth has_command value
    o = _orch(N, t, has_command=3)
    assert L.imx_reset_orchestrate(ctypes.byref(o), stream) != 0 and "has_command" in L.imx_last_error().decode()
    torch.cuda.synchronize()
    assert len(untouched) == 2 * 16 + 2 + 1
    assert all(float(v.abs().sum()) == 0.0 for keep in untouched for v in keep.values()), "a refused call wrote to a buffer"
    # complete: every env is reset (no mask), resampled once and computed -- by both entry points
    for run in (alone, launch):
        for kind in (0, 1):
            c, keep = zero_struct(N, DEV, kind)
            assert run(c) == 0, L.imx_last_error().decode()
            torch.cuda.synchronize()
            assert bool((keep["command_counter_d"] == 1).all()) and bool(torch.isfinite(keep["command_d"]).all())


# ------------------------------------------------------------------------------------------------ the env
def _nav_orch_env(g, **kw):
    from isaaclab_amd import producers
    from isaaclab_amd.env import ManagerBasedRLEnv

    ccfg = g.fixture["env"]["commands"]["pose_command"]
    term = producers.UniformPose2dCommand(ccfg, g.N, g.meta["step_dt"], DEV, seed=5)
    return ManagerBasedRLEnv(g.fixture, state_feed=g.feed(DEV), command_term=term, events_cfg=True, **kw), term


def test_navigation_env_matches_the_real_managers():
    """``reset()`` then 40 ``step()``s of the Navigation env with a ``producers.UniformPose2dCommand`` as its command term and the cfg's own
    ``reset_base`` event -- ONE ``imx_reset_orchestrate_pose2d`` launch per step -- against the REAL ``_reset_idx`` +
    ``CommandManager.compute`` of ``NavigationEnvCfg``, fed the recorded draws: masks, reset ids, counters and trigger state exact;
    command, pos_command_w, heading_command_w (on the circle), timer, metrics, reward, obs, reset_base's sim_writes and every log entry
    within FLOAT_TOL; ``extras["log"]`` shows exactly the reference's keys at every recorded point."""
    g = NavOrchGolden()
    env, ct = _nav_orch_env(g)
    assert env.command_manager.active_terms == ["pose_command"] and env.command_manager.get_term("pose_command") is ct
    assert env.command_manager.get_command("pose_command") is ct.command and tuple(ct.command.shape) == (g.N, 4)
    assert env.event_manager.active_terms == g.meta["event_terms"] == {"reset": ["reset_base"]} and env.curriculum_manager is None
    assert torch.equal(ct.env_origins.cpu(), g.t("static/env_origins")) and torch.equal(ct.default_root_z.cpu(), g.t("static/default_root_state")[:, 2])
    ev = env.event_manager

    def feed_draws(slot):
        ev.get_term("reset_base").uniforms = g.t("draws/reset_base")[slot].to(DEV).contiguous()
        env._orch_draws["command"] = g.t("draws/command")[slot].to(DEV).contiguous()

    def check(tag, extras):
        torch.cuda.synchronize()
        for k in ("root_pose", "root_vel"):
            assert_close(env.sim_writes[k], g.t(f"{tag}/sim_writes/{k}"), FLOAT_TOL, f"{tag} sim_writes[{k}]")
        got = {"command": ct.command, "pos_command_w": ct.pos_command_w, "heading_command_w": ct.heading_command_w, "time_left": ct.time_left,
               "error_pos_2d": ct._error_pos_2d, "error_heading": ct.metrics["error_heading"], "command_counter": ct.command_counter}
        ref = {"command": g.t(f"{tag}/command"), "pos_command_w": g.t(f"{tag}/pos_command_w"), "heading_command_w": g.t(f"{tag}/heading_command_w"),
               "time_left": g.t(f"{tag}/command_time_left"), "error_heading": g.t(f"{tag}/metric_error_heading"), "command_counter": g.t(f"{tag}/command_counter"),
               "error_pos_2d": g.t(f"{tag}/metric_error_pos_2d") if f"{tag}/metric_error_pos_2d" in g.z.files else torch.zeros(g.N)}
        assert_outputs_close(got, ref, FLOAT_TOL, tag)
        assert [f"{tag}/metric_{m}" in g.z.files for m in ("error_pos", "error_heading", "error_pos_2d")] == [True, True, "error_pos_2d" in ct.metrics]
        assert float(ct.metrics["error_pos"].abs().max()) == 0.0
        t = ev.get_term("reset_base")
        assert torch.equal(t.last_triggered_step.cpu()[None], g.t(f"{tag}/reset_last_triggered_step")), tag
        assert torch.equal(t.triggered_once.cpu()[None], g.t(f"{tag}/reset_triggered_once")), tag
        want = g.log(tag)
        metric_keys = lambda d: sorted(k for k in d if k.startswith("Metrics/"))  # noqa: E731
        assert metric_keys(extras["log"]) == metric_keys(want) and set(want) <= set(extras["log"]), (tag, sorted(extras["log"]), sorted(want))
        for key, v in want.items():
            got_v = float(extras["log"][key])
            print(f"{tag} {key}: {got_v:.7g} (reference {v:.7g})")
            assert abs(got_v - v) <= FLOAT_TOL * max(1.0, abs(v)), (tag, key, got_v, v)

    feed_draws(0)
    obs, extras = env.reset()
    assert_close(obs["policy"], g.t("reset/obs"), FLOAT_TOL, "reset obs")
    check("reset", extras)
    assert "Metrics/pose_command/error_pos_2d" not in extras["log"] and extras["log"]["Metrics/pose_command/error_pos"] == 0.0
    env.episode_length_buf = g.t("reset/episode_length_buf")
    resets = 0
    for k in range(g.steps):
        tag = f"step{k}"
        feed_draws(k + 1)
        obs, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").to(DEV))
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")) and torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs"))
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids"))
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf"))
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(obs["policy"], g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        assert torch.equal(obs["policy"][:, 6:10], ct.command), "the observation's pose_command columns are the term's command"
        check(tag, extras)
        assert ("Metrics/pose_command/error_pos_2d" in extras["log"]) == (k >= 1)
        resets += len(g.t(f"{tag}/reset_env_ids"))
    assert resets == g.meta["n_resets"] and 60 <= resets <= 200 and g.meta["n_timer_resamplings"] > 100
    env.close()


def _rollout(use_graph):
    from isaaclab_amd import producers
    from isaaclab_amd.env import ManagerBasedRLEnv
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper
    from isaaclab_amd.state_feed import StateFeed

    g = NavOrchGolden()
    torch.manual_seed(31)
    N = 64
    ccfg = dict(g.fixture["env"]["commands"]["pose_command"], resampling_time_range=(0.4, 1.2))
    term = producers.UniformPose2dCommand(ccfg, N, g.meta["step_dt"], DEV, seed=31)
    feed = StateFeed(g.robot, N, DEV, seed=31, num_snapshots=4)
    u = ManagerBasedRLEnv(g.fixture, state_feed=feed, command_term=term, events_cfg=True, seed=31, noise_seed=31)
    env = RslRlVecEnvWrapper(u)
    runner = OnPolicyRunner(env, dict(g.fixture["agent"], num_steps_per_env=8), log_dir=None, device=DEV, use_graph=use_graph)
    runner.train_mode()
    env.episode_length_buf = u.max_episode_length - 1 - torch.randint(0, 16, (N,), generator=torch.Generator().manual_seed(2)).to(DEV)
    for _ in range(2 if use_graph else 3):  # (the captured runner's first collect is its eager warm-up)
        runner.collect()
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = {k: getattr(st, k).clone().cpu() for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob")}
    res.update(command=term.command.clone().cpu(), pos_command_w=term.pos_command_w.clone().cpu(), time_left=term.time_left.clone().cpu(),
               command_counter=term.command_counter.clone().cpu(), heading_command_w=term.heading_command_w.clone().cpu(),
               root_pose=u.sim_writes["root_pose"].clone().cpu(), joint_pos_target=u._ll_joint_pos_target.clone().cpu())
    env.close()
    return res


def test_captured_rollout_equals_eager_with_the_pose2d_term():
    """8 steps per collect at N = 64: the orchestration launch with the pose-2d command inside the rollout's hipGraph, the Navigation
    task's ten low-level steps per env step unchanged.  Bit for bit."""
    a, c = _rollout(True), _rollout(False)
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], c[k]), f"{k}: graph and eager differ"
    assert a["observations"].shape == (8, 64, 10) and float(a["dones"].sum()) > 0 and int(a["command_counter"].max()) >= 1
    assert float(a["root_pose"].abs().sum()) > 0.0 and float(a["joint_pos_target"].abs().sum()) > 0.0


def test_env_refusals():
    """What stays refused, and what this term is refused with.  The two pinned refusals of tests/test_navigation_gpu.py hold unchanged."""
    from isaaclab_amd import producers
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.state_feed import StateFeed

    g = NavOrchGolden()
    N = 8
    ccfg = g.fixture["env"]["commands"]["pose_command"]
    feed = lambda robot=g.robot: StateFeed(robot, N, DEV, seed=3, num_snapshots=2)  # noqa: E731
    mk = lambda **kw: producers.UniformPose2dCommand(ccfg, N, g.meta["step_dt"], DEV, **kw)  # noqa: E731
    for kw in (dict(command_term="pose_command"), dict(own_managers=True)):
        with pytest.raises(NotImplementedError, match=r"command_term='pose_command'.*UniformPose2dCommand.*no fused producer yet"):
            ManagerBasedRLEnv(g.fixture, state_feed=feed(), **kw)
    for kw in (dict(use_curriculum=True), dict(reward_curriculum=True)):
        with pytest.raises(NotImplementedError, match="UniformPose2dCommand beside use_curriculum=True / reward_curriculum=True"):
            ManagerBasedRLEnv(g.fixture, state_feed=feed(), command_term=mk(), **kw)
    with pytest.raises(ValueError, match="not both"):
        ManagerBasedRLEnv(g.fixture, state_feed=feed(), command_term=mk(), use_command_term=True)
    with pytest.raises(ValueError, match="the term has 7 envs"):
        ManagerBasedRLEnv(g.fixture, state_feed=feed(), command_term=producers.UniformPose2dCommand(ccfg, 7, 0.2, DEV))
    with pytest.raises(ValueError, match="the term's env_origins differs"):
        ManagerBasedRLEnv(g.fixture, state_feed=feed(), command_term=mk(env_origins=torch.full((N, 3), 123.0, device=DEV)), events_cfg=True)
    with pytest.raises(ValueError, match="the term's default_root_z differs"):
        ManagerBasedRLEnv(g.fixture, state_feed=feed(), command_term=mk(default_root_z=9.0), events_cfg=True)
    # a cfg whose plan command is not 4 wide
    vel = load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")
    from isaaclab_amd.robots import ROBOTS

    with pytest.raises(ValueError, match="the term's command is 4 wide, the plan's 3"):
        ManagerBasedRLEnv(vel, state_feed=feed(ROBOTS[vel["robot"]]), command_term=mk())
    # accepted: the env fills in its own origins and default root height
    f = feed()
    env = ManagerBasedRLEnv(g.fixture, state_feed=f, command_term=mk(default_root_z=float(g.t("static/default_root_state")[0, 2])), events_cfg=True)
    assert torch.equal(env.command_term.env_origins, f["env_origins"]) and env._orch_pose2d is None
    env.reset()
    assert env._orch_pose2d is not None and env._orch_manip is None and bool((env.command_term.command_counter == 1).all())
    env.close()
