"""GPU: ``imx_mlp_dw_elu_wide`` (first-layer dW of actor and critic as one launch on a 128 x 256 tile) and the PPO minibatch that uses it.

The wide tile plans the same sample split as ``imx_mlp_dw_elu`` does on each column half of the layer, and every output element sees
its samples in the same order through the same f32 MFMA chain: dW and db are compared with ``torch.equal``.  Shapes where the two plans
differ (ragged N, one split) and the scalar load paths are checked against an fp64 product at the tolerance of
``test_kernels_gpu.py::test_mlp_dw_matches_fp64`` (2e-6 x the sum of |a b| of the largest dot product)."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.5  # what the output buffer holds behind dW / db before the call


def _inputs(M, N, K, ldx, seed):
    """dH, H = ELU(.), X with a row pitch of ldx floats whose pad columns (>= K) hold NaN: nothing read there may reach a stored value."""
    g = torch.Generator().manual_seed(seed)
    dH = torch.randn(M, N, generator=g).cuda()
    H = torch.nn.functional.elu(torch.randn(M, N, generator=g)).cuda()
    Xp = torch.full((M, ldx), float("nan"), device="cuda")
    Xp[:, :K] = torch.randn(M, K, generator=g).cuda()
    return dH, H, Xp


def _wide(libimx, M, N, K, segs, seg_cols, H, Xp, defer_to=None):
    """Runs the wide entry point; returns (dW, db, guard) -- views of ONE buffer laid out like the gradient bucket: dW, db, 64 guard floats."""
    from isaaclab_amd import _lib

    out = torch.full((N * K + N + 64,), SENTINEL, device="cuda")
    nbytes = int(libimx.imx_mlp_dw_wide_scratch_bytes(M, N, K))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * len(segs))(*[s.data_ptr() for s in segs])
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(libimx.imx_mlp_dw_elu_wide(M, N, K, len(segs), ptrs, seg_cols, segs[0].stride(0), H.data_ptr(), H.stride(0), 1.0,
                                          Xp.data_ptr(), Xp.stride(0), out.data_ptr(), out[N * K:].data_ptr(), scratch.data_ptr(), nbytes,
                                          defer_to, st))
    torch.cuda.synchronize()
    return out[:N * K].view(N, K), out[N * K:N * K + N], out[N * K + N:]


@pytest.mark.parametrize("M,N,K,ldx,nseg", [(2048, 256, 235, 236, 1),    # every stage full: the steady movers
                                            (2065, 256, 235, 236, 1),    # ragged last stage: the predicated path
                                            (4096, 1024, 235, 236, 2),   # two gradient segments, 8 tiles x 32 splits
                                            (2048, 256, 256, 256, 1),    # every column block interior
                                            (2048, 256, 132, 132, 1)])   # four columns into the second half
def test_wide_tile_equals_two_narrow_launches(libimx, M, N, K, ldx, nseg):
    """Wide launch over N out-features == imx_mlp_dw_elu on each half of them, bit for bit, dW and db."""
    from isaaclab_amd import _lib

    dH, H, Xp = _inputs(M, N, K, ldx, M + N + K)
    h = N // 2
    if nseg == 2:
        segs, seg_cols = [dH[:, :h].contiguous(), dH[:, h:].contiguous()], h
    else:
        segs, seg_cols = [dH], N
    dW, db, guard = _wide(libimx, M, N, K, segs, seg_cols, H, Xp)
    nb = int(libimx.imx_mlp_scratch_bytes(M, h, K))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for half in range(2):
        dWn, dbn = torch.empty(h, K, device="cuda"), torch.empty(h, device="cuda")
        dh, hh = dH[:, half * h:(half + 1) * h], H[:, half * h:(half + 1) * h]
        _lib.check(libimx.imx_mlp_dw_elu(M, h, K, dh.data_ptr(), dh.stride(0), hh.data_ptr(), hh.stride(0), 1.0, None, 0, Xp.data_ptr(),
                                         Xp.stride(0), dWn.data_ptr(), dbn.data_ptr(), scratch.data_ptr(), nb, st))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(dWn).any())
        assert torch.equal(dW[half * h:(half + 1) * h], dWn), f"dW, half {half}"
        assert torch.equal(db[half * h:(half + 1) * h], dbn), f"db, half {half}"
    assert bool((guard == SENTINEL).all())


@pytest.mark.parametrize("M,N,K,ldx", [(40, 128, 129, 132),      # one split, ragged
                                       (2048, 130, 235, 236),    # ragged N: scalar dH / H path, a second N-slab of two rows
                                       (2048, 256, 131, 131)])   # unaligned rows: scalar X path
def test_wide_tile_matches_fp64(libimx, M, N, K, ldx):
    dH, H, Xp = _inputs(M, N, K, ldx, M + N + K)
    dW, db, guard = _wide(libimx, M, N, K, [dH], N, H, Xp)
    X = Xp[:, :K].double()
    dZ = dH.double() * torch.where(H > 0, torch.ones_like(H, dtype=torch.float64), H.double() + 1.0)
    ref = dZ.t() @ X
    scale = float((dZ.abs().t() @ X.abs()).max())  # sum |a b|: the fp32 error scale of a dot product
    err, err_b = float((dW.double() - ref).abs().max()), float((db.double() - dZ.sum(0)).abs().max())
    print(f"dW err {err:.3e} (bound {2e-6 * scale:.3e}), db err {err_b:.3e} (bound {2e-6 * float(dZ.abs().sum(0).max()):.3e})")
    assert err <= 2e-6 * scale  # (a NaN from X's pad columns or a column left unwritten fails here too)
    assert err_b <= 2e-6 * float(dZ.abs().sum(0).max())
    assert bool((guard == SENTINEL).all())  # nothing behind column K - 1 of the last row, nothing behind db


def test_wide_tile_refuses_other_widths(libimx):
    M, N = 256, 128
    H = torch.zeros(M, N, device="cuda")
    dH = torch.zeros(M, N, device="cuda")
    out = torch.full((N * 260 + N,), SENTINEL, device="cuda")
    scratch = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptrs = (ctypes.c_void_p * 1)(dH.data_ptr())
    for K in (128, 257):
        X = torch.zeros(M, 260, device="cuda")
        assert libimx.imx_mlp_dw_wide_scratch_bytes(M, N, K) == 0
        rc = libimx.imx_mlp_dw_elu_wide(M, N, K, 1, ptrs, N, N, H.data_ptr(), N, 1.0, X.data_ptr(), 260, out.data_ptr(),
                                        out[N * K:].data_ptr(), scratch.data_ptr(), scratch.numel(), None, st)
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())  # refused, not launched


def _minibatch(two_streams, wide, monkeypatch, hidden=(128, 128, 128), expect_wide=None):
    from isaaclab_amd.rsl_rl import ppo as ppo_mod
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic

    monkeypatch.setattr(ppo_mod, "WIDE_DW0", wide)
    M, D, A = 2048, 235, 12
    torch.manual_seed(11)
    pol = ActorCritic(D, D, A, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), init_noise_std=0.7)
    alg = ppo_mod.PPO(pol, num_learning_epochs=1, num_mini_batches=1, schedule="adaptive", desired_kl=0.01, learning_rate=1e-3,
                      entropy_coef=0.005, max_grad_norm=1.0, device="cuda:0", two_streams=two_streams)
    assert alg._joint0 is not None
    g = torch.Generator().manual_seed(5)
    obs = torch.zeros(M, 236, device="cuda")[:, :D]  # 16-byte aligned rows, as the update's pitched gather makes them
    obs.copy_(torch.randn(M, D, generator=g))
    act = torch.randn(M, A, generator=g).cuda()
    old_mu = (0.3 * torch.randn(M, A, generator=g)).cuda()
    old_sigma = (torch.rand(M, A, generator=g) * 0.5 + 0.5).cuda()
    old_logp = torch.distributions.Normal(old_mu, old_sigma).log_prob(act).sum(-1, keepdim=True)
    adv, ret, old_val = (torch.randn(M, 1, generator=g).cuda() for _ in range(3))
    calls = []
    real = ppo_mod.lib().imx_mlp_dw_elu_wide
    monkeypatch.setattr(ppo_mod.lib(), "imx_mlp_dw_elu_wide", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        out8 = alg.minibatch_step(obs, obs, act, old_val, adv, ret, old_logp, old_mu, old_sigma).clone()
    torch.cuda.synchronize()
    assert len(calls) == (int(wide) if expect_wide is None else expect_wide)  # the switch selects the launch, nothing else does
    return alg.bucket.grad.clone(), out8, alg._stats.clone()


@pytest.mark.parametrize("two_streams", [True, False])
def test_minibatch_step_same_bits_with_the_stacked_launch(libimx, monkeypatch, two_streams):
    """PPO.minibatch_step with the stacked first-layer dW launch == the per-network launches: whole gradient bucket and loss statistics."""
    grad1, out1, stats1 = _minibatch(two_streams, True, monkeypatch)
    grad0, out0, stats0 = _minibatch(two_streams, False, monkeypatch)
    assert not bool(torch.isnan(grad1).any())
    assert float(grad1[:235 * 256].abs().max()) > 0.0  # the stacked layer's gradients were written
    assert torch.equal(grad1, grad0)
    assert torch.equal(out1, out0) and torch.equal(stats1, stats0)


def test_minibatch_step_other_first_layer_widths_keep_their_launches(libimx, monkeypatch):
    """192 out-features per network: a network's gradient segment would end inside a 128-row slab -- the per-network launches stay."""
    grad, out8, _ = _minibatch(True, True, monkeypatch, hidden=(192, 128), expect_wide=0)
    assert not bool(torch.isnan(grad).any()) and float(grad[:235 * 384].abs().max()) > 0.0
