"""GPU: the env's own ``UniformPoseCommand`` -- the stand-alone kernel (imx_pose_command) against the fixture of the REAL class and
against the CPU restatement, its in-kernel draws, the orchestration launch with ``has_command = 2`` against the REAL ``_reset_idx`` /
CommandManager / EventManager of the Franka Reach cfg, the env wiring (``command_term=``), a captured rollout, and a few fixed-seed cases
of the random sweeps (tools/fuzz_producers.py::case_pose_command, tools/fuzz_orchestration.py::one_case_pose)."""

import copy
import os
import sys

import numpy as np
import pytest
import torch

from _pose_command_cases import OUT_KEYS, PoseGolden, ReachOrchGolden, pose_case, random_cfg, random_inputs, term_outputs
from _util import FLOAT_TOL, assert_close

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


# ------------------------------------------------------------------------------------------------ the stand-alone kernel
@pytest.mark.parametrize("variant", ["A", "B"])
def test_pose_command_hip_matches_reference(variant):
    """Parity mode against the REAL ``UniformPoseCommand`` (N = 300: one full 256-lane block and a ragged one; 12 steps)."""
    from isaaclab_amd.producers import UniformPoseCommand

    g = PoseGolden(variant)
    term = UniformPoseCommand(g.cfg, g.N, g.step_dt, "cuda:0", robot=g_robot(g))
    assert term.body_idx == g.body_idx
    for k in range(g.steps):
        d = {n: v.cuda() for n, v in g.inputs(k).items()}
        term.compute(g.step_dt, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"], d["reset_mask"], d["uniforms"])
        got, ref = term_outputs(term), g.expected(k)
        assert torch.equal(got["command_counter"].cpu(), ref["command_counter"]), (k, "command_counter")
        for name in OUT_KEYS:
            if name != "command_counter":
                assert_close(got[name], ref[name], FLOAT_TOL, f"{variant} step {k} {name}")


def g_robot(g):
    from isaaclab_amd.robots import ROBOTS

    return ROBOTS[g.meta["robot"]]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_pose_command_hip_matches_restatement(N):
    """Reset mask all / none / mixed, do_compute 0 and 1, and a resampling range whose low end is <= dt: a reset env's timer runs out in
    the same call, so draw 1 of the table is used."""
    rng = np.random.default_rng(N)
    step_dt = 1.0 / 30.0
    plan = [("all", True), ("mixed", True), ("none", True), ("mixed", False), ("none", False), ("all", False), ("mixed", True), ("none", True)]
    for low, unique in ((True, True), (False, False), (True, False)):
        msg = pose_case(N, 11, int(rng.integers(0, 11)), random_cfg(rng, step_dt, low, unique), step_dt, plan, int(rng.integers(0, 1 << 30)))
        if low and N >= 63:
            assert not msg.endswith("twice=0"), msg  # both resamplings of one call happened somewhere


def test_pose_command_in_kernel_draws():
    """No table: the counter-based generator.  Positions inside the ranges, unit quaternions, w >= 0 under make_quat_unique, the same
    seed repeats the run, consecutive calls differ."""
    from isaaclab_amd.producers import UniformPoseCommand
    from isaaclab_amd.robots import FRANKA_PANDA

    N, step_dt = 1000, 1.0 / 30.0
    cfg = dict(PoseGolden("B").cfg)
    r = cfg["ranges"]
    d = {k: v.cuda() for k, v in random_inputs(N, FRANKA_PANDA.num_bodies, torch.Generator().manual_seed(5), "all").items()}
    runs = []
    for trial in range(2):
        term = UniformPoseCommand(cfg, N, step_dt, "cuda:0", seed=77, robot=FRANKA_PANDA)
        cmds = []
        for k in range(3):
            term.compute(step_dt, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"], d["reset_mask"], None)
            c = term.command.clone()
            for j, n in enumerate(("pos_x", "pos_y", "pos_z")):
                assert float(c[:, j].min()) >= r[n][0] - 1e-6 and float(c[:, j].max()) <= r[n][1] + 1e-6, n
            assert float((c[:, 3:].norm(dim=-1) - 1.0).abs().max()) <= 1e-6
            assert float(c[:, 3].min()) >= 0.0
            lo, hi = cfg["resampling_time_range"]
            assert float(term.time_left.min()) > -step_dt and float(term.time_left.max()) <= hi + 1e-6
            assert bool((term.command_counter >= 1).all()) and bool(torch.isfinite(term.metrics["orientation_error"]).all())
            cmds.append(c)
        assert not torch.equal(cmds[0], cmds[1]) and not torch.equal(cmds[1], cmds[2])
        assert float(cmds[0][:, 0].std()) > 0.02  # the envs do not share one draw
        runs.append(torch.stack(cmds))
    assert torch.equal(runs[0], runs[1]), "same seed, same run"
    other = UniformPoseCommand(cfg, N, step_dt, "cuda:0", seed=78, robot=FRANKA_PANDA)
    other.compute(step_dt, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"], d["reset_mask"], None)
    assert not torch.equal(other.command, runs[0][0])


def test_pose_command_refuses_bad_arguments():
    from isaaclab_amd import _lib
    from isaaclab_amd.producers import UniformPoseCommand
    from isaaclab_amd.robots import FRANKA_PANDA

    cfg = PoseGolden("A").cfg
    N = 8
    d = {k: v.cuda() for k, v in random_inputs(N, FRANKA_PANDA.num_bodies, torch.Generator().manual_seed(1), "all").items()}
    term = UniformPoseCommand(cfg, N, 1.0 / 30.0, "cuda:0", robot=FRANKA_PANDA)
    with pytest.raises(ValueError, match="body_pos_w"):
        term.compute(1.0 / 30.0, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"][:, :5].contiguous(), d["body_quat_w"])
    term.body_idx = FRANKA_PANDA.num_bodies
    with pytest.raises(_lib.ImxError, match="body_idx"):
        term.compute(1.0 / 30.0, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"])
    bad = UniformPoseCommand(dict(cfg, resampling_time_range=(0.0, 0.0)), N, 1.0 / 30.0, "cuda:0", robot=FRANKA_PANDA)
    with pytest.raises(_lib.ImxError, match="resampling_time_range"):
        bad.compute(1.0 / 30.0, d["root_pos_w"], d["root_quat_w"], d["body_pos_w"], d["body_quat_w"])


# ------------------------------------------------------------------------------------------------ the orchestration launch
def _reach_orch_env(g, **kw):
    from isaaclab_amd.env import ManagerBasedRLEnv

    return ManagerBasedRLEnv(g.fixture, state_feed=g.feed("cuda:0"), own_managers=True, **kw)


def _feed_draws(env, g, slot):
    d = g.draws(slot)
    env.event_manager.get_term("reset_robot_joints").uniforms = d["reset_robot_joints"].cuda().contiguous()
    env._orch_draws["command"] = d["command"].cuda().contiguous()


def test_reach_orchestration_matches_the_real_managers():
    """``reset()`` then 40 ``step()``s with the env's OWN EventManager and CommandManager (``own_managers=True`` picks the
    UniformPoseCommand by its class_type: ``has_command = 2`` in the one orchestration launch) against the REAL ``_reset_idx`` +
    ``CommandManager.compute`` of the Franka Reach cfg, fed the recorded draws: masks, ids, counters and trigger state exact; command,
    pose_command_w, timer, metrics, reward, obs, sim_writes and every log entry within 1e-5."""
    g = ReachOrchGolden()
    env = _reach_orch_env(g)
    assert env.command_manager.active_terms == ["ee_pose"] and env.command_manager.get_term("ee_pose") is env.command_term
    assert env.event_manager.active_terms == g.meta["event_terms"] and env.curriculum_manager is None
    assert list(env.command_term.metrics) == g.meta["metrics"] and env.command_term.body_idx == g.body_idx
    ev, ct = env.event_manager, env.command_term

    def check(tag, extras):
        torch.cuda.synchronize()
        for k, v in env.sim_writes.items():
            assert_close(v, g.t(f"{tag}/sim_writes/{k}"), FLOAT_TOL, f"{tag} sim_writes[{k}]")
        for k, a in (("command", ct.command), ("pose_command_w", ct.pose_command_w), ("command_time_left", ct.time_left),
                     ("metric_position_error", ct.metrics["position_error"]), ("metric_orientation_error", ct.metrics["orientation_error"])):
            assert_close(a, g.t(f"{tag}/{k}"), FLOAT_TOL, f"{tag} {k}")
        assert torch.equal(ct.command_counter.cpu(), g.t(f"{tag}/command_counter")), f"{tag} command counter"
        t = ev.get_term("reset_robot_joints")
        assert torch.equal(t.last_triggered_step.cpu()[None], g.t(f"{tag}/reset_last_triggered_step")), tag
        assert torch.equal(t.triggered_once.cpu()[None], g.t(f"{tag}/reset_triggered_once")), tag
        for key, v in g.log(tag).items():
            got = float(extras["log"][key])
            assert abs(got - v) <= FLOAT_TOL * max(1.0, abs(v)), (tag, key, got, v)

    _feed_draws(env, g, 0)
    obs, extras = env.reset()
    assert_close(obs["policy"], g.t("reset/obs"), FLOAT_TOL, "reset obs")
    check("reset", extras)
    env.episode_length_buf = g.t("reset/episode_length_buf")
    seen, resets = set(), 0
    for k in range(g.steps):
        tag = f"step{k}"
        _feed_draws(env, g, k + 1)
        obs, rew, terminated, time_outs, extras = env.step(g.t(f"{tag}/action").cuda())
        assert torch.equal(terminated.cpu(), g.t(f"{tag}/terminated")) and torch.equal(time_outs.cpu(), g.t(f"{tag}/time_outs"))
        assert torch.equal(env.reset_env_ids.cpu(), g.t(f"{tag}/reset_env_ids"))
        assert torch.equal(env.episode_length_buf.cpu(), g.t(f"{tag}/episode_length_buf"))
        assert_close(rew, g.t(f"{tag}/reward"), FLOAT_TOL, f"{tag} reward")
        assert_close(obs["policy"], g.t(f"{tag}/obs"), FLOAT_TOL, f"{tag} obs")
        check(tag, extras)
        seen |= set(g.log(tag))
        resets += len(g.t(f"{tag}/reset_env_ids"))
    assert {"Metrics/ee_pose/position_error", "Metrics/ee_pose/orientation_error"} <= seen
    assert resets == g.meta["n_resets"] and 60 <= resets <= 200
    env.close()


# ------------------------------------------------------------------------------------------------ env wiring
@pytest.mark.parametrize("task", ["Isaac-Reach-Franka-v0", "Isaac-Reach-UR10-v0"])
def test_command_term_keyword_on_the_shipped_reach_fixtures(task):
    """``command_term="ee_pose", events_cfg=True``: the observation's pose_command columns are the env's own term's command after
    ``reset()`` and after a step; ``env.reset(env_ids)`` resamples only those envs."""
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.producers import UniformPoseCommand
    from isaaclab_amd.robots import ROBOTS
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg(task)
    fx["env"]["observations"]["policy"]["enable_corruption"] = False
    robot = ROBOTS[fx["robot"]]
    N, J = 300, robot.num_joints
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(robot, N, "cuda:0", seed=3, num_snapshots=3), command_term="ee_pose", events_cfg=True, seed=11)
    ct = env.command_term
    assert isinstance(ct, UniformPoseCommand) and ct.body_name == fx["env"]["commands"]["ee_pose"]["body_name"]
    assert env.command_manager.get_term("ee_pose") is ct and env.command_manager.get_command("ee_pose") is ct.command
    with pytest.raises(KeyError):
        env.command_manager.get_term("base_velocity")
    assert f"Metrics/ee_pose/position_error" in env._log_index and "Metrics/ee_pose/orientation_error" in env._log_index
    assert not any("error_vel" in k for k in env._log_index)
    cols = slice(2 * J, 2 * J + 7)  # joint_pos, joint_vel, pose_command, actions
    obs, _ = env.reset()
    assert torch.equal(obs["policy"][:, cols], ct.command) and bool((ct.command_counter == 1).all())
    r = fx["env"]["commands"]["ee_pose"]["ranges"]
    assert float(ct.command[:, 0].min()) >= r["pos_x"][0] - 1e-6 and float(ct.command[:, 0].max()) <= r["pos_x"][1] + 1e-6
    obs, _, _, _, extras = env.step(torch.zeros(N, env.plan.action_dim, device="cuda:0"))
    assert torch.equal(obs["policy"][:, cols], ct.command)
    assert bool(torch.isfinite(ct.metrics["position_error"]).all()) and float(ct.metrics["position_error"].max()) > 0.0
    assert float((ct.pose_command_w[:, 3:].norm(dim=-1) - 1.0).abs().max()) < 1e-5
    before, counters = ct.command.clone(), ct.command_counter.clone()
    ids = torch.tensor([0, 7, 64, 255, 299], device="cuda:0")
    obs, extras = env.reset(env_ids=ids)
    keep = torch.ones(N, dtype=torch.bool, device="cuda:0")
    keep[ids] = False
    assert torch.equal(ct.command[keep], before[keep]) and torch.equal(ct.command_counter[keep], counters[keep])
    assert bool((ct.command[ids, :3] != before[ids, :3]).any(dim=-1).all()) and bool((ct.command_counter[ids] == 1).all())
    assert "Metrics/ee_pose/position_error" in extras["log"]
    env.close()


def test_command_term_guards():
    from _util import OrchGolden
    from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg
    from isaaclab_amd.events import TerrainImporterState
    from isaaclab_amd.producers import UniformPoseCommand, UniformVelocityCommand
    from isaaclab_amd.robots import FRANKA_PANDA
    from isaaclab_amd.state_feed import StateFeed

    fx = load_task_cfg("Isaac-Reach-Franka-v0")
    N = 64
    feed = StateFeed(FRANKA_PANDA, N, "cuda:0", seed=3, num_snapshots=2)
    with pytest.raises(ValueError, match="nope"):
        ManagerBasedRLEnv(fx, state_feed=feed, command_term="nope")
    with pytest.raises(NotImplementedError, match="command_term="):  # the boolean stays the velocity-only switch
        ManagerBasedRLEnv(fx, state_feed=feed, use_command_term=True)
    with pytest.raises(ValueError, match="not both"):
        ManagerBasedRLEnv(fx, state_feed=feed, use_command_term=True, command_term="ee_pose")
    with pytest.raises(NotImplementedError, match="modify_reward_weight"):  # out of scope: the Reach curriculum terms
        ManagerBasedRLEnv(fx, state_feed=feed, own_managers=True)
    with pytest.raises(ValueError, match="wide"):  # a velocity term on a 7-wide plan
        vcfg = load_task_cfg("Isaac-Velocity-Flat-Anymal-C-v0")["env"]["commands"]["base_velocity"]
        ManagerBasedRLEnv(fx, state_feed=feed, command_term=UniformVelocityCommand(vcfg, N, 1.0 / 30.0, "cuda:0"))
    # a pose cfg plus a terrain curriculum: terrain_levels_vel reads a velocity command
    og = OrchGolden()
    fx2 = copy.deepcopy(fx)
    fx2["env"]["curriculum"] = {"terrain_levels": og.fixture["env"]["curriculum"]["terrain_levels"]}
    ti = TerrainImporterState(og.t("terrain/origins").cuda(), og.t("terrain/levels0").cuda(), og.t("terrain/types").cuda(), og.meta["terrain"]["size_x"])
    with pytest.raises(ValueError, match="velocity command"):
        ManagerBasedRLEnv(fx2, state_feed=feed, command_term="ee_pose", use_curriculum=True, terrain_importer=ti)
    # a ready object is taken as it is
    term = UniformPoseCommand(fx["env"]["commands"]["ee_pose"], N, 1.0 / 30.0, "cuda:0", seed=5, robot=FRANKA_PANDA)
    env = ManagerBasedRLEnv(fx, state_feed=feed, command_term=term)
    assert env.command_term is term and env.command_manager.active_terms == ["ee_pose"]
    env.reset()
    assert bool((term.command_counter == 1).all())
    env.close()
    # the velocity command by name builds the class the boolean builds
    vel = ManagerBasedRLEnv(og.fixture, state_feed=og.feed("cuda:0"), command_term="base_velocity")
    assert isinstance(vel.command_term, UniformVelocityCommand) and "Metrics/base_velocity/error_vel_xy" in vel._log_index
    vel.close()


def test_orchestration_launch_names_what_a_pose_command_lacks():
    """The host check of ``has_command == 2``: each missing piece is named; a terrain curriculum next to it is refused."""
    import ctypes

    from isaaclab_amd import _lib
    from isaaclab_amd._lib import ImxOrch

    N, NB = 8, 3
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(org=z(N, 3), b=z(N, 7), w=z(N, 7), tl=z(N), cnt=z(N, dt=torch.long), m0=z(N), m1=z(N), rp=z(N, 3), rq=z(N, 4), bp=z(N, NB, 3),
             bq=z(N, NB, 4), lv=z(N, dt=torch.long), ty=z(N, dt=torch.long), to=z(2, 2, 3), vc=z(N, 3))
    t["b"][:, 3] = 1.0
    t["rq"][:, 0] = 1.0
    t["bq"][..., 0] = 1.0

    def orch(**over):
        o = ImxOrch(num_envs=N, num_joints=1, num_bodies=NB, dt=0.02, do_step=1, env_origins_d=t["org"].data_ptr(), has_command=2,
                    pose_command_b_d=t["b"].data_ptr(), pose_command_w_d=t["w"].data_ptr(), command_time_left_d=t["tl"].data_ptr(),
                    command_counter_d=t["cnt"].data_ptr(), metric_error_vel_xy_d=t["m0"].data_ptr(), metric_error_vel_yaw_d=t["m1"].data_ptr(),
                    root_pos_w_d=t["rp"].data_ptr(), root_quat_w_d=t["rq"].data_ptr(), body_pos_w_d=t["bp"].data_ptr(),
                    body_quat_w_d=t["bq"].data_ptr(), pose_body_idx=1)
        o.command_cfg[0], o.command_cfg[1] = 0.1, 0.2
        for k, v in over.items():
            setattr(o, k, v)
        return o

    def run(o):
        return _lib.lib().imx_reset_orchestrate(ctypes.byref(o), _lib.current_stream(torch.device("cuda:0")))

    for over, word in ((dict(pose_command_b_d=None), "pose_command_b"), (dict(pose_command_w_d=None), "pose_command_w"),
                       (dict(command_counter_d=None), "timer or counter"), (dict(metric_error_vel_yaw_d=None), "metric"),
                       (dict(body_quat_w_d=None), "body_pos_w and body_quat_w"), (dict(root_pos_w_d=None), "root_pos_w"),
                       (dict(pose_body_idx=NB), "pose_body_idx"), (dict(pose_body_idx=-1), "pose_body_idx"), (dict(has_command=3), "has_command"),
                       (dict(terrain_levels_d=t["lv"].data_ptr(), terrain_types_d=t["ty"].data_ptr(), terrain_origins_d=t["to"].data_ptr(),
                             terrain_rows=2, terrain_cols=2, vel_command_b_d=t["vc"].data_ptr()), "terrain curriculum")):
        assert run(orch(**over)) != 0, word
        assert word in _lib.lib().imx_last_error().decode(), (word, _lib.lib().imx_last_error().decode())
    o = orch()
    o.command_cfg[1] = 0.0
    assert run(o) != 0 and "resampling_time_range" in _lib.lib().imx_last_error().decode()
    assert run(orch()) == 0  # complete: every env is reset (no mask) and resampled once, then computed
    torch.cuda.synchronize()
    assert bool((t["cnt"] >= 1).all()) and bool(torch.isfinite(t["m1"]).all())


# ------------------------------------------------------------------------------------------------ captured rollout
def test_runner_logs_pose_metrics_in_a_captured_rollout(tmp_path):
    """OnPolicyRunner.learn over the Reach env with its own managers: the orchestration launch with the pose command is replayed inside
    the rollout's hipGraph; ``Metrics/ee_pose/*`` reach the scalar log and the command keeps being resampled between replays."""
    from isaaclab_amd.rsl_rl import OnPolicyRunner, RslRlVecEnvWrapper

    g = ReachOrchGolden()
    env = _reach_orch_env(g, seed=3)
    venv = RslRlVecEnvWrapper(env)
    # (41 snapshots in the recorded feed: the graph bakes one pass over them)
    runner = OnPolicyRunner(venv, dict(g.fixture["agent"], num_steps_per_env=g.steps + 1), log_dir=str(tmp_path), device="cuda:0", use_graph=True)
    assert runner._fusable()
    venv.episode_length_buf = g.t("reset/episode_length_buf")
    os.environ["IMX_RUNNER_QUIET"] = "1"
    try:
        runner.learn(1)
        torch.cuda.synchronize()
        first = (env.command_term.command.clone(), env.command_term.command_counter.clone(), env.command_term.time_left.clone())
        runner.learn(1)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("IMX_RUNNER_QUIET", None)
    last = runner.writer.last
    for key in ("Metrics/ee_pose/position_error", "Metrics/ee_pose/orientation_error"):
        assert key in last and np.isfinite(last[key]) and last[key] >= 0.0, key
    assert last["Metrics/ee_pose/position_error"] > 0.0
    ct = env.command_term
    assert not torch.equal(ct.command_counter, first[1]) and not torch.equal(ct.command, first[0])
    lo, hi = g.fixture["env"]["commands"]["ee_pose"]["resampling_time_range"]
    assert float(ct.time_left.max()) <= hi + 1e-6 and float(ct.time_left.min()) > -env.step_dt
    assert float((ct.command[:, 3:].norm(dim=-1) - 1.0).abs().max()) <= 1e-6
    env.close()


# ------------------------------------------------------------------------------------------------ fixed-seed cases of the sweeps
def test_pose_command_producer_sweep():
    import fuzz_producers as fp

    rng = np.random.default_rng(31)
    for _ in range(8):
        fp.case_pose_command(rng)


@pytest.mark.parametrize("seed", range(500, 508))
def test_pose_orchestration_sweep(seed):
    import fuzz_orchestration

    fuzz_orchestration.one_case_pose(seed)
