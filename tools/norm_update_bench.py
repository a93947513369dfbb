"""The two statistics launches of ``imx_empirical_normalization_update`` (one normaliser, and two in one call) against
``imx_empirical_normalization`` with ``update = 1`` (statistics + count + apply: three launches; the apply launch alone is timed beside
it), HIP events around a warm loop.

    python tools/norm_update_bench.py [--shapes 4096x235 4096x157] [--iters 200]

Prints one JSON line per shape, microseconds per call."""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x235", "4096x157"])
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()

    import torch

    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization, update_rows_together

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / args.iters

    for s in args.shapes:
        N, D = (int(v) for v in s.split("x"))
        x = torch.randn(N, D, device="cuda") * 3.0 + 5.0
        old, new, pair = (EmpiricalNormalization([D]).cuda() for _ in range(3))
        pair2 = EmpiricalNormalization([D]).cuda()
        print(json.dumps({"N": N, "D": D, "forward_update_apply_us": timed(lambda: old(x)), "apply_us": timed(lambda: old.apply(x)),
                          "update_rows_us": timed(lambda: new.update_rows(x)),
                          "two_groups_one_call_us": timed(lambda: update_rows_together((pair, x), (pair2, x))),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
