"""k_mlp_dw alone at the three calls the PPO update ships (M = 24576): warm, back-to-back launches with the reductions deferred.

    python tools/dw_bench.py [--lib PATH/libimx.so] [--groups 40] [--m 24576] [--wide]

Each call is launched in groups of eight inside an open reduce batch (imx_reduce_batch_*: the reductions are only queued, as in the
update); HIP events bracket every group and the batched reduction is flushed after the end event, so the GPU never idles between
groups and the events see k_mlp_dw only.  100 launches warm the clocks first: a cold 55-launch loop misreads by 20 % (NOTES.md).
``--lib`` times another build of the library (an experiment, the parent commit) in place of the tree's own.
``--wide``: the first layers of actor and critic instead (2 x 512x235 on the same X): two imx_mlp_dw_elu launches back to back, the
same two on two streams, and one stacked imx_mlp_dw_elu_wide launch (128 x 256 tile); microseconds per PAIR.
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


def wide_compare(L, M, groups, dev):
    """Per pair of first layers: narrow + narrow on one stream, on two streams, one stacked wide launch.  Four pairs per timed group."""
    check = _lib.check
    main_s = torch.cuda.current_stream(dev)
    side_s = torch.cuda.Stream(dev)
    N, K, ldx = 512, 235, 236
    g = torch.Generator().manual_seed(N + K)
    dY = [torch.randn(M, N, generator=g).to(dev) for _ in range(2)]
    H = torch.nn.functional.elu(torch.randn(M, 2 * N, generator=g)).to(dev)
    X = torch.randn(M, ldx, generator=g).to(dev)
    dW, db = torch.empty(2 * N, K, device=dev), torch.empty(2 * N, device=dev)
    nb = int(L.imx_mlp_scratch_bytes(M, N, K))
    scr = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(2)]
    nbw = int(L.imx_mlp_dw_wide_scratch_bytes(M, 2 * N, K))
    scrw = torch.empty(nbw, dtype=torch.uint8, device=dev)
    segs = (ctypes.c_void_p * 2)(dY[0].data_ptr(), dY[1].data_ptr())
    h = ctypes.c_void_p()
    check(L.imx_reduce_batch_create(ctypes.byref(h)))

    def narrow(net, stream):
        hh = H[:, net * N:(net + 1) * N]
        check(L.imx_mlp_dw_elu(M, N, K, dY[net].data_ptr(), N, hh.data_ptr(), 2 * N, 1.0, None, 0, X.data_ptr(), ldx, dW[net * N:].data_ptr(),
                               db[net * N:].data_ptr(), scr[net].data_ptr(), nb, stream))

    def one_stream():
        for _ in range(4):
            narrow(0, main_s.cuda_stream)
            narrow(1, main_s.cuda_stream)

    def two_streams():
        side_s.wait_stream(main_s)
        for _ in range(4):
            narrow(0, main_s.cuda_stream)
            narrow(1, side_s.cuda_stream)
        main_s.wait_stream(side_s)

    def wide():
        for _ in range(4):
            check(L.imx_mlp_dw_elu_wide(M, 2 * N, K, 2, segs, N, N, H.data_ptr(), 2 * N, 1.0, X.data_ptr(), ldx, dW.data_ptr(), db.data_ptr(),
                                        scrw.data_ptr(), nbw, h, main_s.cuda_stream))

    for name, body in (("2 x narrow 512x235, one stream", one_stream), ("2 x narrow 512x235, two streams", two_streams),
                       ("stacked wide 1024x235", wide)):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(groups)]
        for i in range(-13, groups):
            check(L.imx_reduce_batch_begin(h))
            if i >= 0:
                ev[i][0].record()
            body()
            if i >= 0:
                ev[i][1].record()
            check(L.imx_reduce_batch_flush(h, main_s.cuda_stream))
        torch.cuda.synchronize(dev)
        us = sorted(a.elapsed_time(b) * 1e3 / 4 for a, b in ev)
        mean = sum(us) / len(us)
        print(f"{name:36s} mean {mean:7.2f} us per pair  median {us[len(us) // 2]:7.2f}  min {us[0]:7.2f}  max {us[-1]:7.2f}  "
              f"{2.0 * M * 2 * N * K / mean / 1e6:6.1f} TFLOP/s")
    L.imx_reduce_batch_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--wide", action="store_true", help="first layers of actor and critic: two narrow launches against the stacked wide one")
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
    if args.wide:
        return wide_compare(L, M, args.groups, dev)
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
