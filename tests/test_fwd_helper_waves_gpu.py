"""GPU: the eight-wave first-layer forward (imx_mlp_fwd_elu for K > 128 and 16-byte aligned rows: four multiplier waves, four helper
waves that fill the tiles and run the epilogue out of an LDS staging tile) at the smallest shapes at which each of its mechanisms can
go wrong."""

import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu

ALPHA = 0.7
SHAPES = [
    (20, 128, 235, 236),    # single ragged tile, one column block
    (32, 128, 235, 236),    # exactly one full tile
    (33, 130, 235, 236),    # second tile of one row; column block with three waves that own no column
    (300, 128, 235, 236),   # two splits of five tiles: both tile buffers and both staging buffers wrap
    (300, 1024, 235, 236),  # the benchmark's width; eight column blocks share X rows
    (257, 161, 130, 132),   # NS = 96; ragged column block whose float count is not a multiple of four
    (200, 96, 256, 256),    # NS = 128; no column to zero
    (200, 64, 241, 244),    # NS = 128; 15 zeroed columns per row
    (129, 31, 223, 224),    # fewer columns than one wave
]


def _inputs(M, N, K, pitch):
    """x with NaN-filled row padding, w with NaN slack behind it, b -- the construction of test_fused_first_layer_forward_matches_torch."""
    g = torch.Generator().manual_seed(M + N + K)
    xb = torch.full((M, pitch), float("nan"))
    xb[:, :K] = torch.randn(M, K, generator=g)
    x = xb.cuda()[:, :K]
    wflat = torch.full((N * K + 8,), float("nan"))
    wflat[:N * K] = torch.randn(N * K, generator=g) / K ** 0.5
    w, b = wflat.cuda()[:N * K].view(N, K), torch.randn(N, generator=g).cuda()
    return x, w, b


def _launch(libimx, x, w, b, elu, y, ldy):
    from isaaclab_amd import _lib

    M, K = x.shape
    _lib.check(libimx.imx_mlp_fwd_elu(M, w.shape[0], K, x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), ALPHA, elu, y.data_ptr(), ldy,
                                      torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("M,N,K,pitch", SHAPES)
def test_helper_wave_forward_matches_fp64(libimx, M, N, K, pitch):
    x, w, b = _inputs(M, N, K, pitch)
    lin = torch.addmm(b.double(), x.double(), w.double().t())
    for elu in (1, 0):
        y = torch.full((M, N + 3), 7.0, device="cuda")
        _launch(libimx, x, w, b, elu, y, y.stride(0))
        ref = torch.nn.functional.elu(lin, alpha=ALPHA) if elu else lin
        assert_close(y[:, :N], ref.float(), 2e-5, f"eight-wave first layer (elu={elu})")
        assert bool((y[:, N:] == 7.0).all())  # nothing written beyond column N
        again = torch.full((M, N + 3), 7.0, device="cuda")
        _launch(libimx, x, w, b, elu, again, again.stride(0))
        assert torch.equal(y, again)  # two launches on the same inputs


def test_helper_wave_forward_into_a_strided_half(libimx):
    M, N, K, pitch = 300, 512, 235, 236
    x, w, b = _inputs(M, N, K, pitch)
    z = torch.full((M, 1024), 7.0, device="cuda")
    y = z[:, 512:]
    _launch(libimx, x, w, b, 1, y, z.stride(0))
    ref = torch.nn.functional.elu(torch.addmm(b.double(), x.double(), w.double().t()), alpha=ALPHA)
    assert_close(y, ref.float(), 2e-5, "eight-wave first layer into a strided half")
    assert bool((z[:, :512] == 7.0).all())  # the other half is untouched
