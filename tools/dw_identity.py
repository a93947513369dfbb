"""Two builds of libimx.so side by side: are dW, db and Dout of imx_mlp_dw / imx_mlp_dw_elu the same bits?

    python tools/dw_identity.py OTHER/libimx.so [--lib THIS/libimx.so]

Runs the shapes of tests/test_dw_movers_gpu.py and the three calls the PPO update ships (M = 24576) through both libraries on the same
inputs and compares with torch.equal.  Exit status 1 on any difference.
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isaaclab_amd import _lib

NAN = float("nan")
MS = (31, 32, 96, 128, 161, 1056, 2048)
NKL = ((128, 128, 128), (128, 132, 132), (256, 235, 236), (256, 235, 235), (130, 37, 37), (128, 256, 256))
SHIPPED = ((24576, 512, 235, 236, True, False), (24576, 256, 512, 512, True, True), (24576, 128, 256, 256, False, False))


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("imx_mlp_dw", "imx_mlp_dw_elu", "imx_mlp_scratch_bytes", "imx_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return L


def run(L, M, N, K, dY, H, X, elu, dout):
    dW, db = torch.full((N, K), NAN, device="cuda"), torch.full((N,), NAN, device="cuda")
    D = torch.full((M, dY.stride(0)), NAN, device="cuda") if dout else None
    nb = int(L.imx_mlp_scratch_bytes(M, N, K))
    scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if elu:
        rc = L.imx_mlp_dw_elu(M, N, K, dY.data_ptr(), dY.stride(0), H.data_ptr(), H.stride(0), 1.0, D.data_ptr() if dout else None,
                              D.stride(0) if dout else 0, X.data_ptr(), X.stride(0), dW.data_ptr(), db.data_ptr(), scr.data_ptr(), nb, st)
    else:
        rc = L.imx_mlp_dw(M, N, K, dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(), db.data_ptr(), scr.data_ptr(), nb, st)
    if rc != 0:
        raise RuntimeError(L.imx_last_error().decode())
    torch.cuda.synchronize()
    return dW, db, (D[:, :N] if dout else torch.zeros(1, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    args = ap.parse_args()
    A, B = load(args.lib), load(args.other)
    cases = [(M, N, K, ldx, elu, elu) for M in MS for N, K, ldx in NKL for elu in (False, True)] + list(SHIPPED)
    bad = 0
    for M, N, K, ldx, elu, dout in cases:
        g = torch.Generator().manual_seed(M + N + K)
        ldy = N if M == 24576 else N + 4
        dY = torch.randn(M, ldy, generator=g).cuda()
        H = torch.nn.functional.elu(torch.randn(M, ldy, generator=g)).cuda()
        X = torch.randn(M, ldx, generator=g).cuda()
        ra, rb = run(A, M, N, K, dY, H, X, elu, dout), run(B, M, N, K, dY, H, X, elu, dout)
        same = all(torch.equal(x, y) for x, y in zip(ra, rb))
        bad += not same
        if not same or M == 24576:
            print(f"M={M} N={N} K={K} ldx={ldx} elu={elu} dout={dout}: {'same bits' if same else 'DIFFERENT'}")
    print(f"{len(cases)} calls, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
