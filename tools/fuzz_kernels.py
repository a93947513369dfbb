"""Random-shape sweep of the stand-alone kernels against torch (fp64) / the rsl_rl restatement: GAE, imx_mlp_fwd_elu, imx_mlp_infer (packed
and row layouts), imx_mlp_dw[_elu], the LSTM actuator, a whole PPO.update with random network shapes.  Test infrastructure, run on the GPU box:
    python tools/fuzz_kernels.py [cases per kernel] [seed] [kind ...]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from isaaclab_amd import _lib

L = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


def rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1.0)


def case_gae(rng):
    from isaaclab_amd.rsl_rl.storage import gae_returns
    from oracle.rsl_rl_oracle import compute_returns

    T, N = int(rng.integers(1, 70)), int(rng.choice([1, 3, 64, 65, 1000, 4096, 16385, 30000]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    rew, val, last = torch.randn(T, N, 1, generator=g), torch.randn(T, N, 1, generator=g), torch.randn(N, 1, generator=g)
    dones = (torch.rand(T, N, 1, generator=g) < float(rng.choice([0.0, 0.02, 0.3, 1.0]))).to(torch.uint8)
    gamma, lam, norm = float(rng.choice([0.9, 0.99, 0.998])), float(rng.choice([0.0, 0.95, 1.0])), bool(rng.integers(0, 2)) and T * N > 1
    r0, a0 = compute_returns(rew, val, dones, last, gamma, lam, norm)
    r1, a1 = gae_returns(rew.cuda(), val.cuda(), dones.cuda(), last.cuda(), gamma, lam, norm)
    e = max(rel(r1.cpu(), r0), rel(a1.cpu(), a0))
    return e <= 2e-5, f"T={T} N={N} gamma={gamma} lam={lam} norm={norm} err={e:.1e}"


def case_fwd_elu(rng):
    M, N, K = int(rng.choice([1, 31, 33, 500, 4097, 24576])), int(rng.choice([1, 31, 128, 200, 512, 1024])), int(rng.integers(1, 257))
    pitch = K + int(rng.choice([0, 0, 1, 3, 5]))
    w_off = int(rng.choice([0, 0, 1, 2]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    xb = torch.full((M, pitch), float("nan"))
    xb[:, :K] = torch.randn(M, K, generator=g)
    x = xb.cuda()[:, :K]
    wf = torch.full((N * K + 8,), float("nan"))
    wf[w_off:w_off + N * K] = torch.randn(N * K, generator=g) / K ** 0.5
    w, b = wf.cuda()[w_off:w_off + N * K].view(N, K), torch.randn(N, generator=g).cuda()
    elu, alpha = int(rng.integers(0, 2)), float(rng.choice([1.0, 0.5]))
    y = torch.full((M, N + 2), 7.0, device="cuda")
    _lib.check(L.imx_mlp_fwd_elu(M, N, K, x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), alpha, elu, y.data_ptr(), y.stride(0), st()))
    ref = torch.addmm(b.double(), x.double(), w.double().t())
    if elu:
        ref = torch.nn.functional.elu(ref, alpha=alpha)
    e = rel(y[:, :N], ref)
    return e <= 2e-5 and bool((y[:, N:] == 7.0).all()), f"M={M} N={N} K={K} pitch={pitch} w_off={w_off} elu={elu} err={e:.1e}"


def case_infer(rng):
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    M, D, A = int(rng.choice([1, 5, 33, 100, 2048, 4096, 5000])), int(rng.integers(1, 400)), int(rng.integers(1, 40))
    hidden = [int(rng.choice([32, 64, 96, 128, 200, 256, 512])) for _ in range(int(rng.integers(1, 4)))]
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol = ActorCritic(D, D, A, actor_hidden_dims=hidden, critic_hidden_dims=hidden, init_noise_std=1.0).cuda()
    for p in pol.parameters():
        if p.dim() == 1:
            p.data.normal_(0.0, 0.3)
    x = torch.randn(M, D, device="cuda")
    inf = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
    mu, val = torch.full((M, A), float("nan"), device="cuda"), torch.full((M, 1), float("nan"), device="cuda")
    inf(x, mu, val)
    packed, inf._wpk = inf._wpk, None
    mu_r, val_r = torch.full_like(mu, float("nan")), torch.full_like(val, float("nan"))
    inf(x, mu_r, val_r)
    inf._wpk = packed
    same = torch.equal(mu, mu_r) and torch.equal(val, val_r)
    with torch.no_grad():
        e = max(rel(mu, pol.actor.double()(x.double())), rel(val, pol.critic.double()(x.double())))
    return same and e <= 2e-5, f"M={M} D={D} A={A} hidden={hidden} packed==rows {same} err={e:.1e}"


def case_dw(rng):
    M, N, K = int(rng.choice([64, 100, 3000, 24576])), int(rng.choice([17, 128, 200, 256, 512])), int(rng.choice([5, 48, 128, 235, 256, 512]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    ldx = K + int(rng.choice([0, (-K) % 4]))
    X = torch.randn(M, ldx, generator=g).cuda()[:, :K]
    dH, Hs = torch.randn(M, N, generator=g).cuda(), torch.nn.functional.elu(torch.randn(M, N, generator=g)).cuda()
    act = int(rng.integers(0, 2))
    dW, db, dZ = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda"), torch.empty(M, N, device="cuda")
    nb = int(L.imx_mlp_scratch_bytes(M, N, K))
    scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
    if act:
        _lib.check(L.imx_mlp_dw_elu(M, N, K, dH.data_ptr(), N, Hs.data_ptr(), N, 1.0, dZ.data_ptr(), N, X.data_ptr(), X.stride(0), dW.data_ptr(),
                                    db.data_ptr(), scr.data_ptr(), nb, st()))
        dz = dH.double() * torch.where(Hs > 0, torch.ones_like(Hs), Hs + 1.0).double()
    else:
        _lib.check(L.imx_mlp_dw(M, N, K, dH.data_ptr(), N, X.data_ptr(), X.stride(0), dW.data_ptr(), db.data_ptr(), scr.data_ptr(), nb, st()))
        dz = dH.double()
    refW, refb = dz.t() @ X.double(), dz.sum(0)
    scale = float((dz.abs().t() @ X.double().abs()).max())
    e = max(float((dW.double() - refW).abs().max()) / scale, float((db.double() - refb).abs().max()) / float(dz.abs().sum(0).max()))
    ok = e <= 2e-6 and (not act or rel(dZ, dz) <= 1e-6)
    return ok, f"M={M} N={N} K={K} ldx={ldx} act={act} err={e:.1e}"


def case_lstm(rng):
    from isaaclab_amd.producers import ActuatorNetLSTM

    N, J = int(rng.choice([1, 7, 64, 1000, 4096])), int(rng.choice([1, 12, 23]))
    nl, d0 = int(rng.integers(1, 4)), int(rng.choice([0, 16, 32]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5)  # noqa: E731
    lstm = [(r(32, 2 if k == 0 else 8), r(32, 8), r(32), r(32)) for k in range(nl)]
    head = [(r(1, 8), r(1))] if d0 == 0 else [(r(d0, 8), r(d0)), (r(1, d0), r(1))]
    ref = torch.nn.LSTM(2, 8, nl, batch_first=True).double()
    with torch.no_grad():
        for k, (wi, wh, bi, bh) in enumerate(lstm):
            getattr(ref, f"weight_ih_l{k}").copy_(wi); getattr(ref, f"weight_hh_l{k}").copy_(wh)
            getattr(ref, f"bias_ih_l{k}").copy_(bi); getattr(ref, f"bias_hh_l{k}").copy_(bh)
    # (the library picks its kernel once per process: this is the one the process runs; tools/fuzz_producers.py lstm_net sweeps the
    # other two in child processes)
    steps = [tuple(torch.randn(N, J, generator=g) for _ in range(3)) for _ in range(3)]
    a = ActuatorNetLSTM(N, J, 80.0, 7.5, 120.0, lstm_layers=[tuple(t.cuda() for t in l_) for l_ in lstm],
                        head=[tuple(t.cuda() for t in h_) for h_ in head], head_activation="softsign", device="cuda:0")
    for q_des, q, qd in steps:
        a.compute(q_des.cuda(), q.cuda(), qd.cuda())
    h = c = torch.zeros(nl, N * J, 8, dtype=torch.float64)
    with torch.no_grad():
        for q_des, q, qd in steps:
            x = torch.stack([(q_des - q).flatten(), qd.flatten()], 1).double().unsqueeze(1)
            y, (h, c) = ref(x, (h, c))
            y = y[:, -1]
            if d0 == 0:
                out = y @ head[0][0].double().t() + head[0][1].double()
            else:
                out = torch.nn.functional.softsign(y @ head[0][0].double().t() + head[0][1].double()) @ head[1][0].double().t() + head[1][1].double()
    got = (a.computed_effort.cpu(), a.sea_hidden_state.cpu(), a.sea_cell_state.cpu())
    e = max(rel(got[0].reshape(-1, 1), out), rel(got[1], h), rel(got[2], c))
    return e <= 1e-5, f"N={N} J={J} lstm layers={nl} head={d0} err={e:.1e}"


def case_infer_act(rng):
    """imx_mlp_infer_act (PPO.act in the actor head's epilogue) against imx_mlp_infer + imx_policy_act: same seed and step counter ->
    bit-identical actions, log-probs, means, sigmas and stored observations; the critic's values identical too."""
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    M, D, A = int(rng.choice([1, 33, 100, 2048, 4096, 5000])), int(rng.integers(1, 400)), int(rng.integers(1, 41))
    hidden = [int(rng.choice([32, 64, 128, 256, 512])) for _ in range(int(rng.integers(1, 4)))]
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol = ActorCritic(D, D, A, actor_hidden_dims=hidden, critic_hidden_dims=hidden, init_noise_std=float(rng.choice([0.3, 1.0]))).cuda()
    x = torch.randn(M, D, device="cuda")
    inf = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
    seed, step = int(rng.integers(0, 1 << 40)), torch.tensor([int(rng.integers(0, 100000))], dtype=torch.int32, device="cuda")
    mu, val = torch.empty(M, A, device="cuda"), torch.empty(M, 1, device="cuda")
    inf(x, mu, val)
    ref = [torch.full((M, A), float("nan"), device="cuda") for _ in range(3)] + [torch.full((M,), float("nan"), device="cuda"),
                                                                                 torch.full((M, 1), float("nan"), device="cuda"), torch.full((M, D), float("nan"), device="cuda")]
    a0, m0, s0, lp0, v0, o0 = ref
    _lib.check(L.imx_policy_act(M, A, D, mu.data_ptr(), pol.std.data_ptr(), val.data_ptr(), x.data_ptr(), seed, step.data_ptr(), a0.data_ptr(),
                                lp0.data_ptr(), m0.data_ptr(), s0.data_ptr(), v0.data_ptr(), o0.data_ptr(), None, st()))
    a1, m1, s1, lp1, o1 = (torch.full_like(t, float("nan")) for t in (a0, m0, s0, lp0, o0))
    val1 = torch.full_like(val, float("nan"))
    act = _lib.ImxPolicyAct(std_d=pol.std.data_ptr(), seed=seed, step_counter_d=step.data_ptr(), actions_out_d=a1.data_ptr(), logp_out_d=lp1.data_ptr(),
                            mu_out_d=m1.data_ptr(), sigma_out_d=s1.data_ptr(), obs_out_d=o1.data_ptr(), plan=None, state=None, buf=None, pre_clip=float("inf"))
    inf(x, None, val1, act=act)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in ((a0, a1), (m0, m1), (s0, s1), (lp0, lp1), (o0, o1), (val, val1)))
    return same and bool(torch.isfinite(a1).all()), f"M={M} D={D} A={A} hidden={hidden} identical={same}"


def case_ppo_loss(rng):
    """imx_ppo_loss_fwd / imx_ppo_loss_bwd against the restatement's ppo_losses + autograd (shared and per-sample sigma)."""
    from oracle.rsl_rl_oracle import ppo_losses

    M, A = int(rng.choice([1, 7, 256, 257, 3000, 24576])), int(rng.integers(1, 41))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    per_sample = bool(rng.integers(0, 2))
    mu = torch.randn(M, A, generator=g).cuda().double().requires_grad_(True)
    sg = ((0.3 + torch.rand(M, A, generator=g)) if per_sample else (0.3 + torch.rand(A, generator=g)).expand(M, A).contiguous()).cuda().double().requires_grad_(True)
    val = torch.randn(M, 1, generator=g).cuda().double().requires_grad_(True)
    act, old_mu = torch.randn(M, A, generator=g).cuda(), torch.randn(M, A, generator=g).cuda()
    old_sg = (0.3 + torch.rand(M, A, generator=g)).cuda()
    old_logp = (-1.0 - torch.rand(M, 1, generator=g) * A).cuda()
    adv, ret, old_v = (torch.randn(M, 1, generator=g).cuda() for _ in range(3))
    clip, vcoef, ecoef, clipped = 0.2, float(rng.choice([1.0, 0.5])), float(rng.choice([0.0, 0.01])), int(rng.integers(0, 2))
    s_, v_, e_, kl = ppo_losses(mu, sg, act.double(), old_logp.double(), old_mu.double(), old_sg.double(), adv.double(), ret.double(), val, old_v.double(),
                                clip, bool(clipped))
    loss = s_ + vcoef * v_ - ecoef * e_
    loss.backward()
    mu32, sg32, val32 = mu.detach().float(), sg.detach().float(), val.detach().float()
    out8 = torch.empty(8, device="cuda")
    scr = torch.empty(int(L.imx_ppo_scratch_bytes(M)), dtype=torch.uint8, device="cuda")
    _lib.check(L.imx_ppo_loss_fwd(M, A, mu32.data_ptr(), sg32.data_ptr(), A, act.data_ptr(), old_logp.data_ptr(), old_mu.data_ptr(), old_sg.data_ptr(),
                                  adv.data_ptr(), ret.data_ptr(), val32.data_ptr(), old_v.data_ptr(), clip, clipped, vcoef, ecoef, out8.data_ptr(), None,
                                  scr.data_ptr(), st()))
    dmu, dsg, dv = torch.empty(M, A, device="cuda"), torch.empty(M, A, device="cuda"), torch.empty(M, 1, device="cuda")
    _lib.check(L.imx_ppo_loss_bwd(M, A, mu32.data_ptr(), sg32.data_ptr(), A, act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                                  val32.data_ptr(), old_v.data_ptr(), clip, clipped, vcoef, ecoef, 1.0, dmu.data_ptr(), dsg.data_ptr(), dv.data_ptr(), st()))
    refs = torch.stack([s_, v_, e_, kl, loss]).detach()
    e = max(rel(out8[:5], refs), rel(dmu, mu.grad), rel(dsg, sg.grad), rel(dv, val.grad))
    # (fp32 kernel against an fp64 reference of an exp() of a sum of A terms: 1e-4 relative on the largest entry)
    return e <= 1e-4, f"M={M} A={A} per_sample_sigma={per_sample} clipped={clipped} err={e:.1e}"


def case_update(rng):
    """A whole PPO.update against torch autograd + Adam (tests/test_kernels_gpu.py::test_whole_update_matches_torch_reference with the
    network shapes, observation widths, batch and epoch counts drawn at random)."""
    import copy

    import isaaclab_amd.rsl_rl.ppo as ppo_mod
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO
    from oracle.rsl_rl_oracle import adaptive_lr, ppo_losses

    T, N = int(rng.integers(2, 9)), int(rng.choice([8, 50, 96, 400]))
    D, A = int(rng.integers(3, 300)), int(rng.integers(1, 20))
    Dc = int(rng.choice([0, 0, int(rng.integers(3, 300))]))
    hidden = [int(rng.choice([32, 64, 128, 256])) for _ in range(int(rng.integers(1, 4)))]
    nmb, nep = int(rng.choice([1, 2, 4])), int(rng.integers(1, 3))
    while (T * N) % nmb:
        nmb -= 1
    ppo_mod.FUSED_HEAD = str(rng.choice(["0", "1"]))
    std_type = str(rng.choice(["scalar", "scalar", "log"]))
    schedule, clipped_v = str(rng.choice(["adaptive", "adaptive", "fixed"])), bool(rng.choice([True, True, False]))
    norm_mb, two_streams = bool(rng.choice([False, False, True])), bool(rng.choice([True, True, False]))
    ecoef, vcoef, gnorm = float(rng.choice([0.005, 0.0])), float(rng.choice([1.0, 0.5])), float(rng.choice([1.0, 0.3]))
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol = ActorCritic(D, Dc or D, A, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), init_noise_std=0.8, noise_std_type=std_type)
    ref_pol = copy.deepcopy(pol).cuda()
    ref_std = (lambda: ref_pol.std) if std_type == "scalar" else (lambda: torch.exp(ref_pol.log_std))
    kw = dict(num_learning_epochs=nep, num_mini_batches=nmb, schedule=schedule, desired_kl=0.01, learning_rate=1e-3, entropy_coef=ecoef,
              max_grad_norm=gnorm, clip_param=0.2, value_loss_coef=vcoef, use_clipped_value_loss=clipped_v,
              normalize_advantage_per_mini_batch=norm_mb, two_streams=two_streams)
    alg = PPO(pol, device="cuda:0", **kw)
    alg.init_storage("rl", N, T, (D,), (Dc,), (A,))
    stg = alg.storage
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    stg.observations.copy_(torch.randn(T, N, D, generator=g))
    if Dc:
        stg.privileged_observations.copy_(torch.randn(T, N, Dc, generator=g))
    cobs_all = stg.privileged_observations if Dc else stg.observations
    with torch.no_grad():
        mu = ref_pol.actor(stg.observations.flatten(0, 1)).view(T, N, A)
        val = ref_pol.critic(cobs_all.flatten(0, 1)).view(T, N, 1)
    sigma = ref_std().detach().expand(T, N, A).contiguous()
    act = mu + sigma * torch.randn(T, N, A, generator=g).cuda()
    stg.mu.copy_(mu); stg.sigma.copy_(sigma); stg.actions.copy_(act); stg.values.copy_(val)
    stg.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True))
    stg.returns.copy_(val + 0.3 * torch.randn(T, N, 1, generator=g).cuda())
    stg.advantages.copy_(torch.randn(T, N, 1, generator=g))
    stg.step = T
    flat = lambda x: x.flatten(0, 1)  # noqa: E731
    data = [flat(x).clone() for x in (stg.observations, stg.actions, stg.values, stg.advantages, stg.returns, stg.actions_log_prob, stg.mu, stg.sigma, cobs_all)]
    seed = int(rng.integers(0, 1 << 30))
    torch.manual_seed(seed)
    alg.update()
    torch.cuda.synchronize()
    torch.manual_seed(seed)
    Mb = T * N // nmb
    perm = torch.randperm(nmb * Mb, device="cuda:0")
    opt = torch.optim.Adam(ref_pol.parameters(), lr=kw["learning_rate"])
    lr = kw["learning_rate"]
    for _ in range(nep):
        for i in range(nmb):
            idx = perm[i * Mb:(i + 1) * Mb]
            obs, a_, v_old, adv, ret, logp_old, mu_old, sg_old, cobs = (x[idx] for x in data)
            if norm_mb:  # upstream: advantages normalised per minibatch (mean / unbiased std + 1e-8)
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            mu_b = ref_pol.actor(obs)
            s_, v_, e_, kl = ppo_losses(mu_b, ref_std().expand_as(mu_b), a_, logp_old, mu_old, sg_old, adv, ret, ref_pol.critic(cobs), v_old, 0.2, clipped_v)
            if schedule == "adaptive":
                lr = adaptive_lr(lr, float(kl.detach()), 0.01)
            for gr in opt.param_groups:
                gr["lr"] = lr
            loss = s_ + vcoef * v_ - ecoef * e_
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(ref_pol.parameters(), gnorm)
            opt.step()
    # Per parameter tensor: every element within 1e-4, except for a handful (<= 2 + 1e-4 of the tensor) that may be off by up to the
    # learning-rate steps taken -- on its first steps Adam moves a parameter by lr * g / (|g| + 1e-8) whatever |g| is, so the rounding
    # of a gradient element of magnitude ~1e-8 flips a visible fraction of lr (seen: 1 element of 25 856 off by 1.07e-3).  The defects
    # this sweep found moved EVERY element by 2e-3 .. 2e-2.
    err, outliers_ok = 0.0, True
    for (name, p), q in zip(pol.named_parameters(), ref_pol.parameters()):
        d = (p.detach() - q.detach()).abs()
        over = d > 1e-4 * max(1.0, nep * nmb / 4)
        n_over = int(over.sum())
        if n_over > 2 + int(1e-4 * d.numel()) or float(d.max()) > 2.5e-3 * nep * nmb:  # (lr = 1e-3; the adaptive schedule can raise it 1.5x per step)
            outliers_ok = False
        err = max(err, float(d[~over].max()) if n_over < d.numel() else float(d.max()))
        if os.getenv("FUZZ_VERBOSE"):
            print(f"      {name}: max |diff| {float(d.max()):.2e}, elements over 1e-4: {n_over} of {d.numel()}")
    lr_ok = abs(alg.learning_rate - lr) <= 1e-9 * max(1.0, lr)
    learning_rate = alg.learning_rate
    del alg, stg  # (streams, graphs and workspaces of hundreds of PPO objects add up over a sweep)
    import gc

    gc.collect()
    return lr_ok and outliers_ok and err <= 1e-4 * max(1.0, nep * nmb / 4), f"T={T} N={N} D={D} Dc={Dc} A={A} hidden={hidden} mb={nmb} ep={nep} fused_head={ppo_mod.FUSED_HEAD} std={std_type} {schedule} clipped_v={clipped_v} norm_mb={norm_mb} two_streams={two_streams} lr_ok={lr_ok} err={err:.1e}"


def case_update_graph(rng):
    """PPO.update captured as one hipGraph against the eager update (tests/test_kernels_gpu.py::test_update_graph_replay_equals_eager_update
    with random shapes): parameters, Adam state, learning rate and logged losses identical to the last bit over six updates."""
    import copy

    import isaaclab_amd.rsl_rl.ppo as ppo_mod
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    T, N = int(rng.integers(2, 9)), int(rng.choice([16, 96, 400]))
    D, A = int(rng.integers(3, 300)), int(rng.integers(1, 41))
    hidden = [int(rng.choice([32, 64, 128, 256])) for _ in range(int(rng.integers(1, 4)))]
    nmb, nep = int(rng.choice([1, 2, 4])), int(rng.integers(1, 3))
    while (T * N) % nmb:
        nmb -= 1
    ppo_mod.FUSED_HEAD = "0"
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol0 = ActorCritic(D, D, A, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), init_noise_std=1.0)
    kw = dict(num_learning_epochs=nep, num_mini_batches=nmb, schedule="adaptive", desired_kl=0.01, learning_rate=1e-3, entropy_coef=0.005,
              max_grad_norm=1.0, clip_param=0.2, value_loss_coef=1.0, use_clipped_value_loss=True)
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    obs, noise = torch.randn(T, N, D, generator=g), torch.randn(T, N, A, generator=g)
    ret_noise, adv = 0.3 * torch.randn(T, N, 1, generator=g), torch.randn(T, N, 1, generator=g)
    seed = int(rng.integers(0, 1 << 30))
    results = []
    for graph in (False, True):
        alg = PPO(copy.deepcopy(pol0), device="cuda:0", **kw)
        alg.update_graph = graph
        alg.init_storage("rl", N, T, (D,), (0,), (A,))
        torch.manual_seed(seed)
        stats = []
        for it in range(6):
            if graph and it == 4:
                alg._update_t = "graph"
            stg = alg.storage
            stg.observations.copy_(obs + 0.1 * it)
            with torch.no_grad():
                mu = alg.policy.actor(stg.observations.flatten(0, 1)).view(T, N, A)
                val = alg.policy.critic(stg.observations.flatten(0, 1)).view(T, N, 1)
            sigma = alg.policy.std.detach().expand(T, N, A).contiguous()
            act = mu + sigma * noise.cuda()
            stg.mu.copy_(mu); stg.sigma.copy_(sigma); stg.actions.copy_(act); stg.values.copy_(val)
            stg.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True))
            stg.returns.copy_(val + ret_noise.cuda())
            stg.advantages.copy_(adv)
            stg.step = T
            alg.update()
            stats.append(alg.loss_dict())
        torch.cuda.synchronize()
        results.append((alg.bucket.flat.clone(), alg.bucket.exp_avg.clone(), alg.bucket.exp_avg_sq.clone(), alg.learning_rate, stats))
    (p0, m0, v0, lr0, s0), (p1, m1, v1, lr1, s1) = results
    same = lr0 == lr1 and s0 == s1 and torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    del alg, stg
    import gc

    gc.collect()
    return same and bool(torch.isfinite(p1).all()), f"T={T} N={N} D={D} A={A} hidden={hidden} mb={nmb} ep={nep} identical={same}"


ODD_WIDTHS = [32, 33, 64, 100, 128, 200, 256, 400, 500]  # non-multiples of 32 take every ragged path (padded / packed images, K % 32 != 0 heads)


def case_update_shapes(rng):
    """PPO.minibatch_step on minibatch 0 of a seeded storage (the storage's own permutation / gather) against float64 autograd under the
    tolerance rule of tests/_util.py, then an update of ONE minibatch and epoch (gather of every row, loss, backward, clip, Adam) against
    torch autograd + Adam: hidden widths that are not multiples of 32, any ActorCritic activation, different actor / critic stacks, T*N
    up to 24 576 x 4.  One Adam step because later steps amplify rounding: Adam moves an element by ~lr whatever |g| is, and once the
    parameters differ by rounding a ReLU kink or a clip boundary crossed by one path and not the other flips such steps (seen at 4 steps
    with relu / identity nets: whole rows off by 1e-3 while every minibatch gradient passes the fp64 check).  The multi-step update is
    case_update's and tests/test_policy_shapes_gpu.py's."""
    import copy

    import isaaclab_amd.rsl_rl.ppo as ppo_mod
    from _util import check_minibatch_gradients, fill_storage, reference_update, update_params_agree
    from isaaclab_amd.rsl_rl.actor_critic import _ACT, ActorCritic
    from isaaclab_amd.rsl_rl.ppo import PPO

    T, N = int(rng.choice([1, 4, 16, 24])), int(rng.choice([1, 33, 1000, 4096]))
    D, A = int(rng.integers(1, 320)), int(rng.integers(1, 41))
    Dc = int(rng.choice([0, 0, int(rng.integers(1, 320))]))
    act_name = str(rng.choice(sorted(_ACT)))
    ah = [int(rng.choice(ODD_WIDTHS)) for _ in range(int(rng.integers(1, 4)))]
    ch = ah if rng.integers(0, 2) else [int(rng.choice(ODD_WIDTHS)) for _ in range(int(rng.integers(1, 4)))]
    nmb = int(rng.choice([1, 2, 4]))
    while (T * N) % nmb:
        nmb -= 1
    ppo_mod.FUSED_HEAD = str(rng.choice(["0", "1"]))
    two_streams = bool(rng.choice([True, True, False]))
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol = ActorCritic(D, Dc or D, A, actor_hidden_dims=ah, critic_hidden_dims=ch, activation=act_name, init_noise_std=float(rng.choice([0.5, 1.0])))
    ref_pol = copy.deepcopy(pol).cuda()
    kw = dict(num_learning_epochs=1, num_mini_batches=nmb, schedule="adaptive", desired_kl=0.01, learning_rate=1e-3, entropy_coef=0.005,
              max_grad_norm=1.0, clip_param=0.2, value_loss_coef=1.0, use_clipped_value_loss=True, two_streams=two_streams)
    alg = PPO(pol, device="cuda:0", **kw)
    alg.init_storage("rl", N, T, (D,), (Dc,), (A,))
    fill_storage(alg, int(rng.integers(0, 1 << 30)))
    desc = f"T={T} N={N} D={D} Dc={Dc} A={A} actor={ah} critic={ch} act={act_name} mb={nmb} fused_head={ppo_mod.FUSED_HEAD} two_streams={two_streams}"
    seed = int(rng.integers(0, 1 << 30))
    stg = alg.storage
    cobs_all = stg.privileged_observations if Dc else stg.observations
    data = [x.flatten(0, 1).clone() for x in (stg.observations, stg.actions, stg.values, stg.advantages, stg.returns, stg.actions_log_prob,
                                              stg.mu, stg.sigma, cobs_all)]
    try:
        torch.manual_seed(seed)
        stg.draw_permutation(nmb)
        check_minibatch_gradients(alg, stg.gather_minibatch(0, nmb), desc)
    except AssertionError as e:
        return False, str(e)
    alg.num_mini_batches = 1
    torch.manual_seed(seed)
    alg.update()
    torch.cuda.synchronize()
    torch.manual_seed(seed)
    lr = reference_update(ref_pol, data, torch.randperm(T * N, device="cuda:0"), 1, 1, kw)
    ok, err, msg = update_params_agree(pol, ref_pol, 1)
    lr_ok = abs(alg.learning_rate - lr) <= 1e-9 * max(1.0, lr)
    del alg, stg
    import gc

    gc.collect()
    return ok and lr_ok, f"{desc} lr_ok={lr_ok} err={err:.1e} {msg}"


def case_infer_act_shapes(rng):
    """imx_mlp_infer against float64 on a NaN-padded row pitch, packed == row-layout weights, imx_mlp_infer_act == imx_mlp_infer +
    imx_policy_act, with hidden widths that are not multiples of 32 (tests/_util.py helpers)."""
    from _util import check_fused_inference, check_infer_act
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic

    M, D, A = int(rng.choice([1, 33, 100, 2048, 4096, 4113])), int(rng.integers(1, 400)), int(rng.integers(1, 41))
    ah = [int(rng.choice(ODD_WIDTHS)) for _ in range(int(rng.integers(1, 4)))]
    ch = ah if rng.integers(0, 2) else [int(rng.choice(ODD_WIDTHS)) for _ in range(int(rng.integers(1, 4)))]
    torch.manual_seed(int(rng.integers(0, 1 << 30)))
    pol = ActorCritic(D, D, A, actor_hidden_dims=ah, critic_hidden_dims=ch, init_noise_std=float(rng.choice([0.3, 1.0]))).cuda()
    desc = f"M={M} D={D} A={A} actor={ah} critic={ch}"
    seed, step = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 100000))
    try:
        check_fused_inference(pol, M, seed % (1 << 30), desc)
        check_infer_act(pol, M, seed, step, desc)
    except AssertionError as e:
        return False, str(e)
    return True, desc


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad = 0
    kinds = (("gae", case_gae), ("fwd_elu", case_fwd_elu), ("infer", case_infer), ("dw", case_dw), ("lstm", case_lstm), ("infer_act", case_infer_act),
             ("ppo_loss", case_ppo_loss), ("update", case_update), ("update_graph", case_update_graph), ("update_shapes", case_update_shapes),
             ("infer_act_shapes", case_infer_act_shapes))
    only = sys.argv[3:]  # optional: the kinds to run (default: all)
    for name, fn in kinds:
        if only and name not in only:
            continue
        rng = np.random.default_rng(seed)
        nbad, worst = 0, ""
        for c in range(cases):
            try:
                ok, msg = fn(rng)
            except Exception as exc:  # an error return of the library is a finding too
                ok, msg = False, f"{type(exc).__name__}: {exc}"
            if not ok:
                nbad += 1
                print(f"{name} case {c}: FAIL {msg}", flush=True)
            worst = msg
        bad += nbad
        print(f"{name}: {cases - nbad} / {cases} cases agree (last: {worst})", flush=True)
    sys.exit(1 if bad else 0)
