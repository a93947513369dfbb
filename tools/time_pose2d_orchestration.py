"""Timing of the orchestration launch with the pose-2d command (Isaac-Navigation-Flat-Anymal-C-v0).  Run on an MI355X:

    python tools/time_pose2d_orchestration.py [--parent-lib PATH/libimx.so] [--envs 4096] [--steps 2000] [--rounds 6] [--out FILE]

(a) The NEW entry point (``imx_reset_orchestrate_pose2d``), recorded and not judged: the Navigation env with a
    ``producers.UniformPose2dCommand`` as ``command_term=`` and ``events_cfg=True`` (``reset_base``), next to the Reach ``command_term`` +
    events launch of the same library as the nearest existing launch.
(b) The OLD entry point (``imx_reset_orchestrate``), which must not get slower: ``k_reset_orchestrate<false>`` on the
    Isaac-Velocity-Flat-Anymal-C-v0-orch env (``own_managers=True``) and ``k_reset_orchestrate<true>`` on Isaac-Reach-Franka-v0 with
    ``command_term="ee_pose", events_cfg=True``.  With ``--parent-lib`` the parent commit's library and this one ALTERNATE on the same
    env and descriptor, ``--steps`` launches between two HIP events each, ``--rounds`` times; the parent is also run against itself.
    Reported: every sample, the medians, and whether this library's median lies inside the parent's own min-max spread.
(c) ``k_pose2d_command`` alone: ``imx_pose2d_command`` called on the term's struct, one launch per call, every launch a compute with 2 %
    of the envs reset; beside it the same through ``producers.UniformPose2dCommand.compute``, which makes two launches per call.
Each figure is microseconds per launch from HIP events around back-to-back launches (host launch cost included on both sides); 2 % of the
envs reset per launch.
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

from isaaclab_amd import _lib, producers  # noqa: E402
from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg  # noqa: E402
from isaaclab_amd.robots import ROBOTS  # noqa: E402
from isaaclab_amd.state_feed import StateFeed  # noqa: E402
from tools.time_pose_command import events_us, orch_fn, reset_some  # noqa: E402


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

    def row(name, v, extra=""):
        say(f"    {name:<26} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}{extra}")

    say("command: python tools/time_pose2d_orchestration.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}; {a.envs} envs; {a.steps} launches per sample; {a.rounds} rounds; 2 % of the envs reset per launch")
    new = _lib.lib()
    libs = {"this": new}
    if a.parent_lib:
        par = ctypes.CDLL(a.parent_lib)
        par.imx_reset_orchestrate.restype = ctypes.c_int
        par.imx_reset_orchestrate.argtypes = [ctypes.POINTER(_lib.ImxOrch), ctypes.c_void_p]
        libs["parent"] = libs["parent again"] = par
    series = ["parent", "this", "parent again"] if a.parent_lib else ["this", "this again"]
    medians = {}

    def old_path(title, env):
        env.reset()
        reset_some(env)
        assert env._orch_manip is None and env._orch_pose2d is None
        f = orch_fn(env)
        samples = {k: [] for k in series}
        for name in samples:
            env._lib = libs.get(name, new)
            events_us(f, 200)  # warm-up of each code object
        for _ in range(a.rounds):
            for name in samples:
                env._lib = libs.get(name, new)
                samples[name].append(events_us(f, a.steps))
        env._lib = new
        say()
        say(f"(b) {title}, us per launch, alternated")
        for name, v in samples.items():
            row(name, v)
        if a.parent_lib:
            own = samples["parent"] + samples["parent again"]
            med = statistics.median(samples["this"])
            say(f"    median(this) = {med:.3f} us; the parent's own samples span {min(own):.3f} .. {max(own):.3f} us"
                f" -> {'inside' if min(own) <= med <= max(own) else 'below' if med < min(own) else 'ABOVE'} the parent's min-max spread")
        medians[title] = statistics.median(samples["this"])
        env.close()

    old_path("k_reset_orchestrate<false>, Isaac-Velocity-Flat-Anymal-C-v0-orch own_managers (old entry point)",
             ManagerBasedRLEnv("Isaac-Velocity-Flat-Anymal-C-v0-orch", num_envs=a.envs, own_managers=True, seed=1))
    reach_old = "k_reset_orchestrate<true>, Isaac-Reach-Franka-v0 command_term + events (old entry point)"
    old_path(reach_old, ManagerBasedRLEnv("Isaac-Reach-Franka-v0", num_envs=a.envs, command_term="ee_pose", events_cfg=True, seed=1))

    say()
    say("(a) k_reset_orchestrate_pose2d (new entry point), Isaac-Navigation-Flat-Anymal-C-v0 command_term=<UniformPose2dCommand> + events, "
        "us per launch -- recorded, not judged")
    fx = load_task_cfg(os.path.join(ROOT, "tests", "golden", "Isaac-Navigation-Flat-Anymal-C-v0.json"))
    ccfg = dict(fx["env"]["commands"]["pose_command"], resampling_time_range=(0.4, 1.2))  # (2-6 steps: the timer path runs too)
    robot = ROBOTS[fx["robot"]]
    step_dt = fx["env"]["sim"]["dt"] * fx["env"]["decimation"]
    term = producers.UniformPose2dCommand(ccfg, a.envs, step_dt, "cuda:0", seed=1)
    env = ManagerBasedRLEnv(fx, state_feed=StateFeed(robot, a.envs, "cuda:0", seed=1, num_snapshots=4), command_term=term, events_cfg=True, seed=1)
    env.reset()
    reset_some(env)
    assert env._orch_pose2d is not None
    f = orch_fn(env)
    events_us(f, 200)
    v = [events_us(f, a.steps) for _ in range(a.rounds)]
    row("Navigation, pose-2d term", v, f"   ({statistics.median(v) - medians[reach_old]:+.3f} us against this library's Reach figure of (b))")

    say()
    say("(c) k_pose2d_command alone: imx_pose2d_command called on the term's struct, one launch per call, us per launch")
    feed = env.feed
    mask = env.reset_buf.to(torch.uint8)
    c, stream = term.struct(), _lib.current_stream(torch.device("cuda:0"))
    root_pos, root_quat, step_d = feed["root_pos_w"].data_ptr(), feed["root_quat_w"].data_ptr(), env._counters[2:3].data_ptr()

    def alone():
        _lib.check(new.imx_pose2d_command(a.envs, ctypes.byref(c), step_dt, 1, root_pos, root_quat, mask.data_ptr(), 1, step_d, stream))

    events_us(alone, 200)
    row("k_pose2d_command", [events_us(alone, a.steps) for _ in range(a.rounds)])
    say("    the same through producers.UniformPose2dCommand.compute (two launches per call: the step counter's increment and the kernel)")

    def through_producer():
        term.compute(step_dt, mask, None, None, feed["root_pos_w"], feed["root_quat_w"])

    events_us(through_producer, 200)
    row("UniformPose2dCommand.compute", [events_us(through_producer, a.steps) for _ in range(a.rounds)])
    env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
