"""Timing of the orchestration launch around the env's own UniformPoseCommand (profiles/pose_command_timing.txt).  Run on an MI355X:

    python tools/time_pose_command.py [--parent-lib PATH/libimx.so] [--envs 4096] [--steps 2000] [--rounds 6] [--out FILE]

(a) ``k_reset_orchestrate`` on the Isaac-Velocity-Flat-Anymal-C-v0-orch env (the velocity command: ``has_command = 1``): with
    ``--parent-lib`` the parent commit's library and this one ALTERNATE, ``--steps`` launches between two HIP events each, ``--rounds``
    times; without it the library is measured against itself.  The parent reads the head of ``imx_orch_t`` only (the new fields are at
    its end), so both libraries are handed the same descriptor.  Reported: every sample, the medians, and the parent's own spread
    (max - min of its samples) that the difference of the medians is held against.
(b) The same launch with the pose command (``has_command = 2``) and ``k_pose_command`` alone on Isaac-Reach-Franka-v0: first
    measurements, no target.
Each figure is microseconds per launch from HIP events around back-to-back launches (host launch cost included on both sides).
"""

from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaaclab_amd import _lib  # noqa: E402
from isaaclab_amd.env import ManagerBasedRLEnv  # noqa: E402


def events_us(fn, launches: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def reset_some(env, frac=0.02, seed=0):
    g = torch.Generator().manual_seed(seed)
    env.reset_buf.copy_((torch.rand(env.num_envs, generator=g) < frac).to(env.device))


def orch_fn(env):
    def f():
        env.feed.advance()
        env._orchestrate(env.reset_buf, do_step=True)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("command: python tools/time_pose_command.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}; {a.envs} envs; {a.steps} launches per sample; {a.rounds} rounds; 2 % of the envs reset per launch")
    new = _lib.lib()
    libs = {"this": new}
    if a.parent_lib:
        par = ctypes.CDLL(a.parent_lib)
        par.imx_reset_orchestrate.restype = ctypes.c_int
        par.imx_reset_orchestrate.argtypes = [ctypes.POINTER(_lib.ImxOrch), ctypes.c_void_p]
        libs = {"parent": par, "this": new}

    # ---- (a) the velocity command's launch, parent against this library
    env = ManagerBasedRLEnv("Isaac-Velocity-Flat-Anymal-C-v0-orch", num_envs=a.envs, own_managers=True, seed=1)
    env.reset()
    reset_some(env)
    f = orch_fn(env)
    samples = {k: [] for k in (["parent", "this"] if a.parent_lib else ["this", "this again"])}
    for name in samples:
        env._lib = libs.get(name, new)
        events_us(f, 200)  # warm-up of each code object
    for _ in range(a.rounds):
        for name in samples:
            env._lib = libs.get(name, new)
            samples[name].append(events_us(f, a.steps))
    env._lib = new
    say()
    say("(a) k_reset_orchestrate, Isaac-Velocity-Flat-Anymal-C-v0-orch (velocity command), us per launch, alternated")
    for name, v in samples.items():
        say(f"    {name:<11} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}")
    base, other = list(samples)
    spread = max(samples[base]) - min(samples[base])
    diff = statistics.median(samples[other]) - statistics.median(samples[base])
    say(f"    median({other}) - median({base}) = {diff:+.3f} us; spread of {base} against itself (max - min) = {spread:.3f} us"
        f" -> {'within' if diff <= spread else 'OUTSIDE'} the spread")
    env.close()

    # ---- (b) the pose command: the orchestration launch and the stand-alone kernel
    env = ManagerBasedRLEnv("Isaac-Reach-Franka-v0", num_envs=a.envs, command_term="ee_pose", events_cfg=True, seed=1)
    env.reset()
    reset_some(env)
    f = orch_fn(env)
    events_us(f, 200)
    orch = [events_us(f, a.steps) for _ in range(a.rounds)]
    ct, fd = env.command_term, env.feed

    def alone():
        fd.advance()
        ct.compute(env.step_dt, fd["root_pos_w"], fd["root_quat_w"], fd["body_pos_w"], fd["body_quat_w"], env.reset_buf)

    events_us(alone, 200)
    solo = [events_us(alone, a.steps) for _ in range(a.rounds)]
    say()
    say("(b) Isaac-Reach-Franka-v0 (pose command, reset_joints_by_scale), us per launch -- first measurements, no target")
    for name, v in (("k_reset_orchestrate<pose>", orch), ("k_pose_command alone", solo)):
        say(f"    {name:<26} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}")
    env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
