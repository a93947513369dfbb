"""GPU: the mover waves of k_mlp_dw (imx_mlp_dw / imx_mlp_dw_elu) at the smallest shapes where each of their paths can go wrong.

The movers have a steady-state path (16-byte rows, every stage of a split a full 32 rows: unpredicated loads, a lane past the row
re-reads an in-bounds vector) and the general predicated path (a ragged last stage, rows that are not 16-byte aligned).  With the
256 CUs of an MI355X the sample counts below give: 31 one ragged stage; 32 one full stage and no steady state; 96 a single split of
three stages; 128 two splits; 161 a ragged last stage in the last split only; 1056 a split count that is no multiple of 8 (plain
workgroup order); 2048 32 splits in XCD order.  Every row-pitch pad of dY, H and X holds NaN: a pad that reaches a stored output
shows as a NaN there.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
MS = (31, 32, 96, 128, 161, 1056, 2048)
NKL = ((128, 128, 128), (128, 132, 132), (256, 235, 236), (256, 235, 235), (130, 37, 37), (128, 256, 256))


def padded(data, ld, fill=NAN, rows=None, offset=0):
    """``data`` at row pitch ``ld`` (floats), pads and rows past the data holding ``fill``, the first row ``offset`` floats into the allocation."""
    M, n = data.shape
    rows = rows or M
    flat = torch.full((rows * ld + offset,), fill, device="cuda")
    view = flat[offset:].view(rows, ld)
    view[:M, :n] = data
    return view


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """Inputs (on the GPU) and references of one shape, computed once and shared: nobody writes to them."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    dY = torch.randn(M, N, generator=g).cuda()
    H = torch.nn.functional.elu(torch.randn(M, N, generator=g)).cuda()
    X = torch.randn(M, K, generator=g).cuda()
    dZ = torch.ops.aten.elu_backward(dY, 1.0, 1.0, 1.0, True, H)
    ref = {}
    for name, y in (("plain", dY), ("elu", dZ)):
        y64, x64 = y.double(), X.double()
        ref[name] = (y64.t() @ x64, float((y64.abs().t() @ x64.abs()).max()), y64.sum(0), float(y64.abs().sum(0).max()))
    return dY, H, X, dZ, ref


def dw(libimx, M, N, K, dY, X, H=None, Dout=None, want_db=True):
    """One call on row-pitched views (``.stride(0)`` is the pitch); returns (dW, db)."""
    from isaaclab_amd import _lib

    dW = torch.full((N, K), NAN, device="cuda")
    db = torch.full((N,), NAN, device="cuda") if want_db else None
    nbytes = int(libimx.imx_mlp_scratch_bytes(M, N, K))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dbp = db.data_ptr() if want_db else None
    if H is None:
        _lib.check(libimx.imx_mlp_dw(M, N, K, dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(), dbp, scratch.data_ptr(),
                                     nbytes, st))
    else:
        _lib.check(libimx.imx_mlp_dw_elu(M, N, K, dY.data_ptr(), dY.stride(0), H.data_ptr(), H.stride(0), 1.0,
                                         Dout.data_ptr() if Dout is not None else None, Dout.stride(0) if Dout is not None else 0, X.data_ptr(),
                                         X.stride(0), dW.data_ptr(), dbp, scratch.data_ptr(), nbytes, st))
    return dW, db


def other_pitch(ldx):
    """A pitch of the other alignment class: 16-byte rows <-> rows that are not."""
    return ldx + 1 if ldx % 4 == 0 else (ldx + 3) // 4 * 4


@pytest.mark.parametrize("N,K,ldx", NKL)
@pytest.mark.parametrize("M", MS)
def test_dw_plain_matches_fp64_with_poisoned_pads(libimx, M, N, K, ldx):
    """imx_mlp_dw against the fp64 product (2e-6 x max sum|a b|, 2e-6 x max sum|dY|), NaN in every pitch pad; the call on rows of the
    other alignment class gives the same bits."""
    dY, _, X, _, ref = case(M, N, K)
    ref_w, scale_w, ref_b, scale_b = ref["plain"]
    ldy = N + 4
    dW, db = dw(libimx, M, N, K, padded(dY, ldy), padded(X, ldx))
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    assert float((dW.double() - ref_w).abs().max()) <= 2e-6 * scale_w
    assert float((db.double() - ref_b).abs().max()) <= 2e-6 * scale_b
    # the pads do not reach the result: zeros in their place change nothing
    dW0, db0 = dw(libimx, M, N, K, padded(dY, ldy, 0.0), padded(X, ldx, 0.0))
    assert torch.equal(dW, dW0) and torch.equal(db, db0)
    # aligned and unaligned pitch on the same data (16-byte vector movers against the scalar ones): the same bits.  The bias sum
    # follows the dY movers' row ownership, so with the dY pitch changed only dW is the same bits and db is within its bound.
    dW1, db1 = dw(libimx, M, N, K, padded(dY, ldy), padded(X, other_pitch(ldx)))
    assert torch.equal(dW, dW1) and torch.equal(db, db1)
    dW2, db2 = dw(libimx, M, N, K, padded(dY, ldy + 1), padded(X, other_pitch(ldx)))
    assert torch.equal(dW, dW2)
    assert float((db2.double() - ref_b).abs().max()) <= 2e-6 * scale_b
    dW3, _ = dw(libimx, M, N, K, padded(dY, ldy + 1), padded(X, ldx), want_db=False)
    assert torch.equal(dW, dW3)


@pytest.mark.parametrize("N,K,ldx", NKL)
@pytest.mark.parametrize("M", MS)
def test_dw_elu_is_elu_backward_then_dw_with_poisoned_pads(libimx, M, N, K, ldx):
    """imx_mlp_dw_elu == aten elu_backward followed by imx_mlp_dw, bit for bit, NaN in every pitch pad; Dout is written for rows < M
    and columns < N and nowhere else."""
    dY, H, X, dZ, ref = case(M, N, K)
    ref_w, scale_w, ref_b, scale_b = ref["elu"]
    ldy, ldh, ldd = N + 4, N + 8, N + 4
    dW0, db0 = dw(libimx, M, N, K, padded(dZ, ldy), padded(X, ldx))
    D = torch.full((M + 3, ldd), NAN, device="cuda")
    dW, db = dw(libimx, M, N, K, padded(dY, ldy), padded(X, ldx), padded(H, ldh), D)
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    assert torch.equal(dW, dW0) and torch.equal(db, db0)
    assert float((dW.double() - ref_w).abs().max()) <= 2e-6 * scale_w
    assert float((db.double() - ref_b).abs().max()) <= 2e-6 * scale_b
    assert torch.equal(D[:M, :N], dZ)
    assert bool(torch.isnan(D[M:]).all()) and bool(torch.isnan(D[:, N:]).all())
    # no layer below (Dout not materialised), and the scalar movers on unaligned rows: the same bits
    dW1, db1 = dw(libimx, M, N, K, padded(dY, ldy), padded(X, ldx), padded(H, ldh))
    assert torch.equal(dW, dW1) and torch.equal(db, db1)
    D2 = torch.full((M + 3, ldd + 1), NAN, device="cuda")
    dW2, db2 = dw(libimx, M, N, K, padded(dY, ldy + 1), padded(X, other_pitch(ldx)), padded(H, ldh + 1), D2)
    assert torch.equal(dW, dW2) and torch.equal(D2[:M, :N], dZ)  # (db: the dY movers' row ownership differs, see the plain test)
    assert float((db2.double() - ref_b).abs().max()) <= 2e-6 * scale_b
    dW3, db3 = dw(libimx, M, N, K, padded(dY, ldy), padded(X, other_pitch(ldx)), padded(H, ldh))
    assert torch.equal(dW, dW3) and torch.equal(db, db3)
    assert bool(torch.isnan(D2[M:]).all()) and bool(torch.isnan(D2[:, N:]).all())


@pytest.mark.parametrize("M", (161, 2048))
def test_dw_x_offset_by_four_bytes(libimx, M):
    """X with 16-byte row pitch but a base 4 bytes off the boundary: the vector path must not be taken; same bits as the aligned call."""
    N, K, ldx = 256, 235, 236
    dY, H, X, dZ, ref = case(M, N, K)
    ref_w, scale_w, _, _ = ref["plain"]
    Xo = padded(X, ldx, offset=1)
    assert Xo.data_ptr() % 16 == 4
    dW, db = dw(libimx, M, N, K, padded(dY, N), Xo)
    assert float((dW.double() - ref_w).abs().max()) <= 2e-6 * scale_w
    dW0, db0 = dw(libimx, M, N, K, padded(dY, N), padded(X, ldx))
    assert torch.equal(dW, dW0) and torch.equal(db, db0)
    D = torch.full((M, N), NAN, device="cuda")
    dW1, db1 = dw(libimx, M, N, K, padded(dY, N), Xo, padded(H, N), D)
    dW2, db2 = dw(libimx, M, N, K, padded(dZ, N), padded(X, ldx))
    assert torch.equal(dW1, dW2) and torch.equal(db1, db2) and torch.equal(D, dZ)
