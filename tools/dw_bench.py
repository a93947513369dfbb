"""k_mlp_dw alone at the three calls the PPO update ships (M = 24576): warm, back-to-back launches with the reductions deferred.

    python tools/dw_bench.py [--lib PATH/libimx.so] [--groups 40] [--m 24576]

Each call is launched in groups of eight inside an open reduce batch (imx_reduce_batch_*: the reductions are only queued, as in the
update); HIP events bracket every group and the batched reduction is flushed after the end event, so the GPU never idles between
groups and the events see k_mlp_dw only.  100 launches warm the clocks first: a cold 55-launch loop misreads by 20 % (NOTES.md).
``--lib`` times another build of the library (an experiment, the parent commit) in place of the tree's own.
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isaaclab_amd import _lib

# (name, out, in, ldx, ELU, Dout)
CALLS = (("layer0 elu 512x235 ldx236 no-Dout", 512, 235, 236, True, False),
         ("layer1 elu 256x512 Dout", 256, 512, 512, True, True),
         ("layer2 plain 128x256", 128, 256, 256, False, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--groups", type=int, default=40, help="timed groups of eight launches per call (40 -> 320 launches)")
    ap.add_argument("--m", type=int, default=24576)
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    L = _lib.lib()
    check = _lib.check
    dev = torch.device("cuda:0")
    st = _lib.current_stream(dev)
    M = args.m
    print(f"library {_lib.LIB_PATH}; M = {M}; {8 * args.groups} timed launches per call")
    total = 0.0
    for name, N, K, ldx, elu, dout in CALLS:
        g = torch.Generator().manual_seed(N + K)
        dY = torch.randn(M, N, generator=g).to(dev)
        H = torch.nn.functional.elu(torch.randn(M, N, generator=g)).to(dev)
        X = torch.randn(M, ldx, generator=g).to(dev)
        D = torch.empty(M, N, device=dev) if dout else None
        dW, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        nb = int(L.imx_mlp_scratch_bytes(M, N, K))
        scr = torch.empty(nb, dtype=torch.uint8, device=dev)
        if elu:
            call = lambda: check(L.imx_mlp_dw_elu(M, N, K, dY.data_ptr(), N, H.data_ptr(), N, 1.0, D.data_ptr() if dout else None,
                                                  N if dout else 0, X.data_ptr(), ldx, dW.data_ptr(), db.data_ptr(), scr.data_ptr(), nb, st))
        else:
            call = lambda: check(L.imx_mlp_dw(M, N, K, dY.data_ptr(), N, X.data_ptr(), ldx, dW.data_ptr(), db.data_ptr(), scr.data_ptr(), nb, st))
        h = ctypes.c_void_p()
        check(L.imx_reduce_batch_create(ctypes.byref(h)))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        for i in range(-13, args.groups):  # 13 untimed groups = 104 warm launches
            check(L.imx_reduce_batch_begin(h))
            if i >= 0:
                ev[i][0].record()
            for _ in range(8):
                call()
            if i >= 0:
                ev[i][1].record()
            check(L.imx_reduce_batch_flush(h, st))
        torch.cuda.synchronize(dev)
        L.imx_reduce_batch_destroy(h)
        us = sorted(a.elapsed_time(b) * 1e3 / 8 for a, b in ev)
        mean = sum(us) / len(us)
        total += mean
        print(f"{name:36s} mean {mean:7.2f} us  median {us[len(us) // 2]:7.2f}  min {us[0]:7.2f}  max {us[-1]:7.2f}  "
              f"{2.0 * M * N * K / mean / 1e6:6.1f} TFLOP/s")
    print(f"sum of the three means {total:.2f} us")


if __name__ == "__main__":
    main()
