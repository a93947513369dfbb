"""Timing of the orchestration launch on the manipulation tasks.  Run on an MI355X:

    python tools/time_manip_orchestration.py [--parent-lib PATH/libimx.so] [--envs 4096] [--steps 2000] [--rounds 6] [--out FILE]

(a) The OLD entry point (``imx_reset_orchestrate``), which must not get slower: ``k_reset_orchestrate<false>`` on the
    Isaac-Velocity-Flat-Anymal-C-v0-orch env (``own_managers=True``) and ``k_reset_orchestrate<true>`` on Isaac-Reach-Franka-v0 with
    ``command_term="ee_pose", events_cfg=True``.  With ``--parent-lib`` the parent commit's library and this one ALTERNATE on the same
    env and descriptor (``imx_orch_t`` and ``imx_event_term_t`` have the parent's layout), ``--steps`` launches between two HIP events
    each, ``--rounds`` times; the parent is also run against itself.  Reported: every sample, the medians, and the parent's own spread
    (max - min over both of its series) that the difference of the medians is held against.
(b) The manipulation entry point (``imx_reset_orchestrate_manip``): Isaac-Reach-Franka-v0 and Isaac-Lift-Cube-Franka-v0
    with ``own_managers=True, reward_curriculum=True``, next to the figure of (a) on Reach.
(c) The launch on a scene with a second articulation (``imx_reset_orchestrate_scene``), reported and not judged: the
    Isaac-Open-Drawer-Franka-v0 fixture with ``own_managers=True``.  The parent has no such entry point.
With ``--parent-lib`` the rows of (b) alternate with the parent's ``imx_reset_orchestrate_manip`` too and are held against its spread.
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

from isaaclab_amd import _lib  # noqa: E402
from isaaclab_amd.env import ManagerBasedRLEnv, load_task_cfg  # noqa: E402
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

    say("command: python tools/time_manip_orchestration.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}; {a.envs} envs; {a.steps} launches per sample; {a.rounds} rounds; 2 % of the envs reset per launch")
    new = _lib.lib()
    libs = {"this": new}
    if a.parent_lib:
        par = ctypes.CDLL(a.parent_lib)
        par.imx_reset_orchestrate.restype = ctypes.c_int
        par.imx_reset_orchestrate.argtypes = [ctypes.POINTER(_lib.ImxOrch), ctypes.c_void_p]
        par.imx_reset_orchestrate_manip.restype = ctypes.c_int
        par.imx_reset_orchestrate_manip.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        libs["parent"] = libs["parent again"] = par
    series = ["parent", "this", "parent again"] if a.parent_lib else ["this", "this again"]
    medians = {}

    def old_path(title, env):
        env.reset()
        reset_some(env)
        assert env._orch_manip is None
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
        say(f"(a) {title}, us per launch, alternated")
        for name, v in samples.items():
            say(f"    {name:<13} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}")
        if a.parent_lib:
            own = samples["parent"] + samples["parent again"]
            spread = max(own) - min(own)
            diff = statistics.median(samples["this"]) - statistics.median(own)
            say(f"    median(this) - median(parent, both series) = {diff:+.3f} us; spread of the parent against itself (max - min) = {spread:.3f} us"
                f" -> {'within' if abs(diff) <= spread else 'OUTSIDE'} the spread")
        medians[title] = statistics.median(samples["this"])
        env.close()

    old_path("k_reset_orchestrate<false>, Isaac-Velocity-Flat-Anymal-C-v0-orch own_managers (old entry point)",
             ManagerBasedRLEnv("Isaac-Velocity-Flat-Anymal-C-v0-orch", num_envs=a.envs, own_managers=True, seed=1))
    reach_old = "k_reset_orchestrate<true>, Isaac-Reach-Franka-v0 command_term + events (old entry point)"
    old_path(reach_old, ManagerBasedRLEnv("Isaac-Reach-Franka-v0", num_envs=a.envs, command_term="ee_pose", events_cfg=True, seed=1))

    say()
    say("(b) k_reset_orchestrate_manip (imx_reset_orchestrate_manip), own_managers + reward_curriculum, us per launch"
        + (", alternated with the parent's" if a.parent_lib else " -- reported, not judged"))
    lift = os.path.join(ROOT, "tests", "golden", "Isaac-Lift-Cube-Franka-v0.json")
    for title, cfg in (("Isaac-Reach-Franka-v0", "Isaac-Reach-Franka-v0"), ("Isaac-Lift-Cube-Franka-v0", load_task_cfg(lift))):
        env = ManagerBasedRLEnv(cfg, num_envs=a.envs, own_managers=True, reward_curriculum=True, seed=1)
        env.reset()
        reset_some(env)
        assert env._orch_manip is not None
        f = orch_fn(env)
        samples = {k: [] for k in series}
        for name in samples:
            env._lib = libs.get(name, new)
            events_us(f, 200)
        for _ in range(a.rounds):
            for name in samples:
                env._lib = libs.get(name, new)
                samples[name].append(events_us(f, a.steps))
        env._lib = new
        v = samples["this"]
        say(f"    {title:<26} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}"
            f"   ({statistics.median(v) - medians[reach_old]:+.3f} us over this library's Reach figure of (a))")
        if a.parent_lib:
            own = samples["parent"] + samples["parent again"]
            spread, diff = max(own) - min(own), statistics.median(v) - statistics.median(own)
            say(f"        parent, both series: median {statistics.median(own):7.3f}  min {min(own):7.3f}  max {max(own):7.3f}; median(this) - median(parent) = "
                f"{diff:+.3f} us; spread {spread:.3f} us -> {'within' if abs(diff) <= spread else 'OUTSIDE'} the spread")
        env.close()

    say()
    say("(c) k_reset_orchestrate_scene (imx_reset_orchestrate_scene), Isaac-Open-Drawer-Franka-v0 own_managers, us per launch -- reported, not judged")
    drawer = os.path.join(ROOT, "tests", "golden", "Isaac-Open-Drawer-Franka-v0.json")
    env = ManagerBasedRLEnv(load_task_cfg(drawer), num_envs=a.envs, own_managers=True, seed=1)
    env.reset()
    reset_some(env)
    assert env._orch_articulation is not None
    f = orch_fn(env)
    events_us(f, 200)
    v = [events_us(f, a.steps) for _ in range(a.rounds)]
    say(f"    {'Isaac-Open-Drawer-Franka-v0':<26} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}")
    env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
