"""Random env cfgs through the term compiler and the HIP env step, against the CPU oracle consuming the same cfg: the rough-terrain
Anymal-C scene with random subsets (order kept) of the reward / termination / observation terms of the kitchen-sink fixture (every mdp
term the path knows, two observation groups), random weights (incl. 0), scale / clip / uniform, gaussian and constant noise (add, scale, abs), modifier chains (scale, bias, clip,
DigitalFilter, Integrator), per-term and
per-group history, episode length, the six joint action classes in random combinations (processed actions compared).  Masks / ids bit-exact, floats 1e-5.  Test infrastructure, run on
the GPU box:  python tools/fuzz_cfg.py [cases] [first_seed]

``--fp64``: the same random cfgs per term against the oracle in float64 on an edge-shaped feed (tests/_step_cases.py, the env-step rule of
tests/_util.py), at env counts across the group-size and wave-order boundaries and both step-tail modes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from cfg_cases import mutate
from _util import FLOAT_TOL, assert_close
from isaaclab_amd.env import ManagerBasedRLEnv
from isaaclab_amd.robots import ROBOTS
from isaaclab_amd.state_feed import StateFeed
from isaaclab_amd.terrain import make_rough_terrain
from oracle.mdp_oracle import OracleEnv


def one_case(case_seed: int) -> str:
    rng = np.random.default_rng(case_seed)
    fx, what = mutate(rng)
    N = int(rng.choice([1, 63, 64, 65, 257, 1000, 2049]))
    steps = int(rng.integers(2, 6))
    robot = ROBOTS[fx["robot"]]
    v, t, e = make_rough_terrain(2, 3, tile=8.0, border=5.0, seed=int(rng.integers(0, 100)))
    terrain, ext = (v, t), (e[0] - 1.0, e[1] - 1.0)
    cpu_feed = StateFeed(robot, N, "cpu", seed=int(rng.integers(0, 10000)), num_snapshots=3, extent_xy=ext)
    gpu_feed = StateFeed.from_tensors(robot, [cpu_feed.snapshot(i) for i in range(3)], "cuda:0", cpu_feed.gravity_dir)
    try:
        env = ManagerBasedRLEnv(fx, state_feed=gpu_feed, terrain=terrain, terrain_cell=0.1)
    except NotImplementedError as exc:  # combinations the product refuses by name at construction
        return f"REFUSED ({str(exc)[:90]})"
    env.materialize_ray_hits = True
    orc = OracleEnv(fx["env"], robot.joint_names, robot.body_names, N, cpu_feed.__getitem__, cpu_feed.gravity_dir)
    gen = torch.Generator().manual_seed(int(rng.integers(0, 10000)))
    ep = torch.randint(0, env.max_episode_length, (N,), generator=gen)
    ep[::5] = env.max_episode_length - 1
    groups = list(fx["env"]["observations"])
    W = sum(int(np.prod(env.observation_manager.group_obs_dim[g])) for g in groups)  # wide enough for every group's columns
    env._noise_u = torch.rand(N, W, generator=gen).cuda()
    obs0, _ = env.reset()
    orc.reset_action_terms()  # ActionManager.reset of env.reset(): the EMA term's previous applied action <- the joint positions
    if env.plan.num_rays:
        orc.ray_hits_w = env._ray_hits.cpu()
    ref0 = orc.compute_observation_groups(env._noise_u.cpu())
    for gname in groups:
        assert_close(obs0[gname], ref0[gname], FLOAT_TOL, f"reset obs[{gname}]")
    env.episode_length_buf = ep
    orc.episode_length_buf[:] = ep
    nreset = 0
    for _ in range(steps):
        a = torch.randn(N, env.plan.action_dim, generator=gen).clamp(-3, 3)
        u = torch.rand(N, W, generator=gen)
        env._noise_u.copy_(u)
        obs_dict, rew, term, tout, extras = env.step(a.cuda())
        orc.process_action(a)
        pa, po = env._processed_action.cpu(), orc.processed_actions
        badc = ((pa - po).abs() > FLOAT_TOL * po.abs().clamp(min=1.0)).any(0).nonzero().flatten().tolist()
        if badc:
            raise AssertionError(f"processed actions step {_}: columns {badc} differ (max {float((pa - po).abs().max()):.3e}); terms "
                                 + json.dumps({n: {k: v for k, v in a.items() if k in ('class_type', 'scale', 'offset', 'clip', 'alpha', 'joint_names', 'use_zero_offset', 'use_default_offset', 'rescale_to_limits')}
                                               for n, a in fx["env"]["actions"].items()}))
        cpu_feed.advance()
        if env.plan.num_rays:
            orc.ray_hits_w = env._ray_hits.cpu()
        out = orc.post_physics_step(u)
        assert torch.equal(term.cpu(), out["terminated"]) and torch.equal(tout.cpu(), out["time_outs"]), "masks"
        assert torch.equal(env.reset_env_ids.cpu(), out["reset_env_ids"]), "reset ids"
        nreset += len(out["reset_env_ids"])
        # the reward is a sum of weighted terms that the random weights can make large and cancelling (seen: +8608 - 2485 ... -> 122.46): the
        # fp32 rounding of the TERMS (1e-7 relative each, agreed to the last digits) bounds the error of the sum, not the size of the sum
        scale = (out["step_reward"].abs().sum(1) * float(env.step_dt)).clamp(min=1.0)
        rerr = (rew.cpu() - out["reward"]).abs() / scale
        assert float(rerr.max()) <= FLOAT_TOL, f"reward: {float(rerr.max()):.2e} of the summed term magnitudes (env {int(rerr.argmax())})"
        assert_close(env.reward_manager._step_reward, out["step_reward"], FLOAT_TOL, "per-term step reward")
        for gname in groups:
            got, ref = obs_dict[gname].cpu(), out["obs_groups"][gname]
            bad = ((got - ref).abs() > FLOAT_TOL * ref.abs().clamp(min=1.0)).any(0).nonzero().flatten().tolist()
            if bad:
                grp = fx["env"]["observations"][gname]
                desc = [(k, (v.get("noise") or {}).get("operation"), v.get("history_length"), v.get("scale"), v.get("clip")) for k, v in grp.items() if isinstance(v, dict)]
                raise AssertionError(f"obs[{gname}] step {_}: columns {bad[:6]}..{bad[-1]} ({len(bad)} of {got.shape[1]}) differ, max {float((got - ref).abs().max()):.3e}; "
                                     f"group history {grp.get('history_length')} corruption {grp.get('enable_corruption')} terms {desc}")
        assert torch.equal(env.episode_length_buf.cpu(), orc.episode_length_buf), "episode length"
        for key, val in out["log"].items():
            assert abs(float(extras["log"][key]) - val) <= 1e-5 * max(1.0, abs(val)), key
    env.close()
    return f"N={N} steps={steps} resets={nreset}: {what}"


def one_case_fp64(case_seed: int) -> str:
    from _step_cases import run_case
    from isaaclab_amd.plan import compile_plan

    rng = np.random.default_rng(case_seed)
    fx, what = mutate(rng)
    N = int(rng.choice([1, 2, 17, 63, 64, 65, 257, 1000, 2049, 8192, 8193, 16385]))
    steps = int(rng.integers(3, 5))
    tail = str(rng.choice(["deferred", "in_kernel"]))
    try:
        compile_plan(fx["env"], ROBOTS[fx["robot"]])
    except NotImplementedError as exc:  # combinations the product refuses by name at construction
        return f"REFUSED ({str(exc)[:90]})"
    seen = run_case(fx, N, seed=case_seed, steps=steps, tail=tail)
    return f"N={N} steps={steps} tail={tail} resets={seen['resets']} near={seen['near']}: {what}"


if __name__ == "__main__":
    fp64 = "--fp64" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--fp64"]
    cases = int(args[0]) if len(args) > 0 else 40
    first = int(args[1]) if len(args) > 1 else 0
    run = one_case_fp64 if fp64 else one_case
    bad = 0
    for c in range(first, first + cases):
        try:
            print(f"case {c}: ok   {run(c)}", flush=True)
        except (AssertionError, NotImplementedError, ValueError, KeyError, RuntimeError) as e:
            bad += 1
            print(f"case {c}: FAIL {type(e).__name__}: {str(e)[:1500]}", flush=True)
    print(f"{cases - bad} / {cases} cases agree")
    sys.exit(1 if bad else 0)
