"""Isaac-Repose-Cube-Allegro-v0 without a GPU: the CPU restatement of its in-hand terms and of its command term (tests/_inhand_oracle.py)
and the command's per-env device function run as host C++ (tools/inhand_command_host.cpp) against the fixtures of the REAL classes
(tests/golden/Isaac-Repose-Cube-Allegro-v0.npz, inhand_command.npz; tools/gen_golden_inhand.py)."""

import subprocess

import numpy as np
import pytest
import torch

import _inhand_cases as ic
import _inhand_oracle as io
from _util import FLOAT_TOL, assert_close


def test_golden_takes_every_branch_and_keeps_its_margins():
    g = ic.golden()
    b = dict(g.meta["branches"])
    assert g.N == 64 and g.steps == 5 and g.meta["obs_dim"] == ic.D and g.meta["action_dim"] == ic.A
    assert b.pop("min_angle_margin") >= 0.99 * ic.ANGLE_MARGIN and b.pop("min_distance_margin") >= ic.DIST_MARGIN
    assert all(v > 0 for v in b.values()), b
    # what the recorded branch counts say is what the recorded tensors hold
    snaps = [{n: g.t("static/env_origins") if n == "env_origins" else g.t(f"step{t}/in/{n}") for n in ic.NAMES} for t in range(g.steps)]
    again = ic.branch_counts(snaps)
    assert {k: again[k] for k in b} == b
    mc = g.meta["margin_check"]
    assert mc["pairs"] == 4096 and mc["flipped_comparisons"] == 0 and mc["max_fp32_fp64_difference_rad"] < 1.0e-6
    # every termination of the task fires somewhere, and so does each side of the bonus
    for name in ("time_out", "max_consecutive_success", "object_out_of_reach"):
        assert sum(int(g.t(f"step{t}/term_dones/{name}").sum()) for t in range(g.steps)) > 0, name
    bonus = torch.cat([g.t(f"step{t}/step_reward")[:, 1] for t in range(g.steps)])
    assert bool((bonus == 250.0).any()) and bool((bonus == 0.0).any()) and bool(((bonus == 0.0) | (bonus == 250.0)).all())


def test_term_restatement_reproduces_the_reference_fixture():
    """Masks bit for bit; the two rewards and the object / goal observation columns (noise and scale applied as the manager does:
    value + std z, then scale) within 1e-5."""
    g = ic.golden()
    obs_cfg = g.fixture["env"]["observations"]["policy"]
    for t in range(g.steps):
        s = {n: g.t("static/env_origins") if n == "env_origins" else g.t(f"step{t}/in/{n}") for n in ic.NAMES}
        r = io.terms(s, ic.SUCCESS_THRESHOLD, ic.ROT_EPS, float(ic.NUM_SUCCESS), ic.REACH)
        assert torch.equal(r["max_consecutive_success"], g.t(f"step{t}/term_dones/max_consecutive_success")), t
        assert torch.equal(r["object_out_of_reach"], g.t(f"step{t}/term_dones/object_out_of_reach")), t
        sr = g.t(f"step{t}/step_reward")
        assert torch.equal(r["success_bonus"] * 250.0, sr[:, 1]), t
        assert_close(r["track_orientation_inv_l2"], sr[:, 0], FLOAT_TOL, f"step{t} track_orientation_inv_l2")
        obs, z = g.t(f"step{t}/obs"), g.t(f"step{t}/noise_u")
        for name in ("object_pos", "object_quat", "object_lin_vel", "object_ang_vel", "goal_pose", "goal_quat_diff"):
            lo, hi = ic.COLS[name]
            v, c = r[name], obs_cfg[name]
            if c.get("noise"):
                v = v + (c["noise"]["mean"] + c["noise"]["std"] * z[:, lo:hi])
            if c.get("scale") is not None:
                v = v * c["scale"]
            assert_close(v, obs[:, lo:hi], FLOAT_TOL, f"step{t} {name}")


def _oracle(g):
    return io.CommandOracle(g.cfg, g.N, g.const("pos_command_e"), g.const("pos_command_w"))


def test_command_restatement_reproduces_the_reference_fixture():
    g = ic.CommandGolden()
    assert g.N == 64 and g.calls == 7 and g.cfg["make_quat_unique"] is True and g.cfg["update_goal_on_success"] is True
    assert g.meta["metrics"] == ["orientation_error", "position_error", "consecutive_success"]
    assert g.meta["min_threshold_margin_rad"] >= 0.9e-4 and g.meta["goals_reached"] > 50 and g.meta["timer_resamplings"] > 10
    orc = _oracle(g)
    assert torch.equal(orc.pos_command_e, g.const("default_object_pos") + torch.tensor(g.cfg["init_pos_offset"]))
    assert torch.equal(orc.pos_command_w, orc.pos_command_e + g.const("env_origins"))
    for t in range(g.calls):
        d = g.inputs(t)
        orc.call(g.step_dt, t > 0, d["reset_mask"], d["uniforms"], d["object_root_pos_w"], d["object_root_quat_w"])
        got = dict(command=orc.command, time_left=orc.time_left, command_counter=orc.command_counter, **orc.metrics)
        ic.assert_command_close(got, g.expected(t), 1.0e-5, f"oracle call {t}")
    last = g.expected(g.calls - 1)
    assert float(last["consecutive_success"].max()) >= 3.0 and int(last["command_counter"].max()) >= 3
    assert bool((torch.cat([g.expected(t)["command"][:, 3] for t in range(g.calls)]) >= 0).all())  # make_quat_unique


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    import _task_space_cases as tsc

    if tsc.host_compiler() is None:
        pytest.skip("no C++ compiler (c++, g++, clang++ or $CXX) on this machine")
    return tsc.build_host_program("inhand_command_host", str(tmp_path_factory.mktemp("inhand_command_host")))


def test_device_function_as_host_code_matches_reference(host_program, tmp_path):
    """inhand_command_env (csrc/imx_inhand_command.h), compiled as plain C++, over all seven calls with the recorded draws: counters
    and consecutive_success bit for bit, floats within 1e-5."""
    g = ic.CommandGolden()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    g.host_file(fin)
    subprocess.check_call([host_program, fin, fout])
    for t, got in enumerate(g.read_host_output(fout)):
        ic.assert_command_close(got, g.expected(t), 1.0e-5, f"host call {t}")


def test_host_program_refuses_bad_files(host_program, tmp_path):
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 64)
    assert subprocess.run([host_program, str(bad), str(tmp_path / "o")], capture_output=True).returncode == 2
    g = ic.CommandGolden()
    fin = tmp_path / "in.bin"
    g.host_file(str(fin))
    fin.write_bytes(fin.read_bytes()[:-100])  # the last call is truncated
    r = subprocess.run([host_program, str(fin), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 2 and "truncated" in r.stderr


def test_object_state_is_served_on_request_and_changes_no_other_tensor():
    from isaaclab_amd.robots import ALLEGRO_HAND, FRANKA_PANDA
    from isaaclab_amd.state_feed import OBJECT_STATE, StateFeed

    a, b = StateFeed(FRANKA_PANDA, 16, seed=7, num_snapshots=2), StateFeed(FRANKA_PANDA, 16, seed=7, num_snapshots=2)
    assert not any(n in a.names() for n in OBJECT_STATE)
    before = {n: b._stack[n].clone() for n in b._stack}
    b.ensure_object_state()
    assert set(b._stack) == set(before) | set(OBJECT_STATE)
    for n, t in before.items():
        assert torch.equal(b._stack[n], t) and torch.equal(a._stack[n], t), n
    q = b["object_root_quat_w"]
    assert q.shape == (16, 4) and torch.allclose(q.norm(dim=-1), torch.ones(16), atol=1e-6)
    assert b["object_root_lin_vel_w"].shape == (16, 3) and b["object_root_ang_vel_w"].shape == (16, 3)
    cs = b["command_consecutive_success"]
    assert cs.shape == (16,) and cs.dtype == torch.float32 and torch.equal(cs, cs.round()) and float(cs.min()) >= 0 and float(cs.max()) < 60
    with pytest.raises(KeyError, match="object_root_quat_w"):
        StateFeed.from_tensors(FRANKA_PANDA, [a.snapshot(0)]).ensure_object_state()
    StateFeed.from_tensors(FRANKA_PANDA, [b.snapshot(0)]).ensure_object_state()
    # the Allegro hand's object lies next to the hand: most of the envs within the task's 0.3 m reach, some beyond
    f = StateFeed(ALLEGRO_HAND, 4096, seed=3, num_snapshots=1)
    d = (f["object_root_pos_w"] - f["root_pos_w"]).norm(dim=-1)
    assert 0.02 < float((d > ic.REACH).float().mean()) < 0.5
    assert f["command"].shape == (4096, 7)
    print("fraction beyond reach", float((d > ic.REACH).float().mean()))
