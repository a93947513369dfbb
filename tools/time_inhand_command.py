"""Timing of ``k_inhand_command`` (the stand-alone InHandReOrientationCommand producer).  Run on an MI355X:

    python tools/time_inhand_command.py [--envs 4096] [--steps 2000] [--rounds 6] [--out FILE]

``imx_inhand_command`` called on the term's struct, one launch per call, every launch a compute with 2 % of the envs reset and the
object held 0.05 .. 0.15 rad from the goal (about half of the goals are reached and resampled); beside it the same through
``producers.InHandReOrientationCommand.compute``.  Each figure is microseconds per launch from HIP events around back-to-back launches
(host launch cost included).  Recorded, not judged.
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
from tools.time_pose_command import events_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, dev = a.envs, torch.device("cuda:0")
    say("command: python tools/time_inhand_command.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}; {N} envs; {a.steps} launches per sample; {a.rounds} rounds; 2 % of the envs reset per launch")
    cfg = {"resampling_time_range": (1.0e6, 1.0e6), "init_pos_offset": (0.0, 0.0, -0.04), "make_quat_unique": False,
           "orientation_success_threshold": 0.1, "update_goal_on_success": True}
    g = torch.Generator().manual_seed(0)
    term = producers.InHandReOrientationCommand(cfg, N, 1.0 / 30.0, dev, seed=1, env_origins=torch.zeros(N, 3, device=dev),
                                                default_object_pos=(0.0, -0.19, 0.56))
    term.reset()
    mask = (torch.rand(N, generator=g) < 0.02).to(dev)
    pos = (term.pos_command_w + torch.randn(N, 3, generator=g).to(dev) * 0.02).contiguous()
    # the object a small rotation about x away from the goal of the moment (the goal moves on where it is reached: the mix stays)
    ang = (torch.rand(N, generator=g) * 0.1 + 0.05).to(dev)
    rot = torch.stack([torch.cos(ang / 2), torch.sin(ang / 2), torch.zeros_like(ang), torch.zeros_like(ang)], dim=-1)
    quat = rot.contiguous()  # (against the identity-like start; later goals are anywhere: those launches take the not-reached path)
    L, st = _lib.lib(), _lib.current_stream(dev)
    c = term.struct()
    c.object_root_pos_w_d, c.object_root_quat_w_d, c.reset_mask_d = pos.data_ptr(), quat.data_ptr(), mask.data_ptr()

    def raw():
        _lib.check(L.imx_inhand_command(ctypes.byref(c), N, 1.0 / 30.0, 1, st))

    def through_class():
        term.compute(1.0 / 30.0, pos, quat, reset_mask=mask)

    for name, f in (("imx_inhand_command", raw), ("InHandReOrientationCommand.compute", through_class)):
        events_us(f, 200)
        v = [events_us(f, a.steps) for _ in range(a.rounds)]
        say(f"    {name:<36} " + " ".join(f"{x:7.3f}" for x in v) + f"   median {statistics.median(v):7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  us per launch")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
