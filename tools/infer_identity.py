"""Two builds of libimx.so side by side: do the rollout inference launches leave the same bits?

    python tools/infer_identity.py OTHER/libimx.so [--lib THIS/libimx.so]

Runs imx_mlp_infer, imx_mlp_infer_act, imx_mlp_infer_act2 and imx_mlp_infer_act2n through both libraries on the same inputs (row-pitched,
NaN in the pad columns) at M = 17, 77 (16-row tiles), 2081 and 4096 (32-row tiles; packed and row-layout weights): plain, with an
ImxPolicyAct without a plan, with the flat Anymal-C plan (affine joint terms) and with the Lift-Cube plan (a binary joint term).  Every
output buffer (40 sentinel rows past M included) and the env's action buffers are compared as bit patterns.  Exit status 1 on any
difference.
"""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

from isaaclab_amd import _lib

ENTRIES = ("imx_mlp_infer", "imx_mlp_infer_act", "imx_mlp_infer_act2", "imx_mlp_infer_act2n")
MS = (17, 77, 2081, 4096)
NAN = float("nan")


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES + ("imx_last_error",):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return L


def rows(M, D, seed):
    xb = torch.full((M, D + 5), NAN)
    xb[:, :D] = torch.randn(M, D, generator=torch.Generator().manual_seed(seed)) * 2.0
    return xb.cuda()[:, :D]


def env_for(plan, M):
    if plan == "affine":
        from isaaclab_amd.env import ManagerBasedRLEnv

        env = ManagerBasedRLEnv("Isaac-Velocity-Flat-Anymal-C-v0", num_envs=M, device="cuda:0")
    else:
        import _lift_cases as lc
        from isaaclab_amd.env import ManagerBasedRLEnv
        from isaaclab_amd.robots import FRANKA_PANDA
        from isaaclab_amd.state_feed import StateFeed

        feed = StateFeed(FRANKA_PANDA, M, "cuda:0", seed=5, num_snapshots=2)
        lc.lift_tweak(feed, FRANKA_PANDA.body_names.index(lc.EE_BODY), torch.Generator().manual_seed(5))
        env = ManagerBasedRLEnv(lc.load_fixture(), state_feed=feed, noise_seed=11)
        assert env.plan.processed_action_dim != env.plan.action_dim
    env.reset()
    g = torch.Generator().manual_seed(4)
    env._action.copy_(torch.randn(env._action.shape, generator=g))
    env._prev_action.copy_(torch.randn(env._prev_action.shape, generator=g))
    return env


def run(L, entry, inf, x, cx, norms, packed, with_act, env, std):
    """One launch into fresh buffers; returns every buffer it may have written."""
    M, A = x.shape[0], inf.out_features[0]
    S = lambda *sh: torch.full((M + 40, *sh), -7777.0, device="cuda")  # noqa: E731
    o = dict(mu=S(A), values=S(1), actions=S(A), logp=S(), sigma=S(A), obs=S(x.shape[1]), cobs=S(cx.shape[1]))
    bufs = (env._action, env._prev_action, env._processed_action) if env is not None else ()
    start = [b.clone() for b in bufs]
    act, stp = None, torch.tensor([3], dtype=torch.int32, device="cuda")
    if with_act:
        act = _lib.ImxPolicyAct(std_d=std.data_ptr(), seed=99, step_counter_d=stp.data_ptr(), actions_out_d=o["actions"].data_ptr(),
                                logp_out_d=o["logp"].data_ptr(), mu_out_d=o["mu"].data_ptr(), sigma_out_d=o["sigma"].data_ptr(),
                                obs_out_d=o["obs"].data_ptr(), plan=env._plan_h.value if env is not None else None,
                                state=ctypes.pointer(env._state()) if env is not None else None,
                                buf=ctypes.pointer(env._bufs) if env is not None else None, pre_clip=0.9 if env is not None else math.inf)
    outs = (ctypes.c_void_p * 2)(None if with_act else o["mu"].data_ptr(), o["values"].data_ptr())
    wpk = inf._wpk if packed else None
    net = (inf._n, inf._nl, inf._dims, inf._w, inf._pitch)
    st = torch.cuda.current_stream().cuda_stream
    a = ctypes.byref(act) if act is not None else None
    if entry == "imx_mlp_infer":
        rc = L.imx_mlp_infer(M, x.data_ptr(), x.stride(0), *net, inf._b, inf._alpha, outs, st)
    elif entry == "imx_mlp_infer_act":
        rc = L.imx_mlp_infer_act(M, x.data_ptr(), x.stride(0), *net, wpk, inf._b, inf._alpha, outs, a, st)
    else:
        xs, ld = (ctypes.c_void_p * 2)(x.data_ptr(), cx.data_ptr()), (ctypes.c_int64 * 2)(x.stride(0), cx.stride(0))
        cobs = o["cobs"].data_ptr() if with_act else None
        if entry == "imx_mlp_infer_act2":
            rc = L.imx_mlp_infer_act2(M, xs, ld, *net, wpk, inf._b, inf._alpha, outs, a, cobs, st)
        else:
            triples = (_lib.ImxInferNorm * 2)(*[n.infer_norm() for n in norms])
            rc = L.imx_mlp_infer_act2n(M, xs, ld, *net, wpk, inf._b, inf._alpha, outs, a, cobs, triples, st)
    if rc != 0:
        raise RuntimeError(L.imx_last_error().decode())
    torch.cuda.synchronize()
    for name, b, b0 in zip(("action", "prev_action", "processed_action"), bufs, start):
        o[name] = b.clone()
        b.copy_(b0)
    return o


def main():
    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    args = ap.parse_args()
    LA, LB = load(args.lib), load(args.other)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    calls = bad = 0
    for M in MS:
        big = (M + 31) // 32 * 2 * 2 > cus  # the dispatch rule for two networks
        for plan in ("none", "affine", "binary"):
            env = env_for(plan, M) if plan != "none" else None
            A = env.plan.action_dim if env is not None else 12
            for entry in ENTRIES:
                if entry == "imx_mlp_infer" and plan != "none":
                    continue
                Dp, Dc = (235, 235) if entry in ENTRIES[:2] else (48, 235)  # (the first two entry points: one input for both networks)
                torch.manual_seed(M + A)
                pol = ActorCritic(Dp, Dc, A, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[256, 96], init_noise_std=0.7).cuda()
                inf = FusedInference(_mlp_layers(pol.actor), _mlp_layers(pol.critic))  # (for its argument arrays)
                assert inf.ok and inf._wpk is not None
                x, cx = rows(M, Dp, M), rows(M, Dc, M + 1)
                norms = [EmpiricalNormalization([D]).cuda() for D in (Dp, Dc)]
                for n in norms:
                    n._mean.copy_(torch.randn(n._mean.shape) * 2.0)
                    n._std.copy_(torch.rand(n._std.shape) + 0.5)
                acts = (False,) if entry == "imx_mlp_infer" else ((False, True) if plan == "none" else (True,))
                for with_act in acts:
                    for packed in ((True, False) if big and entry != "imx_mlp_infer" else (True,)):
                        ra, rb = (run(L, entry, inf, x, cx, norms, packed, with_act, env, pol.std) for L in (LA, LB))
                        diff = [k for k in ra if not torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32))]
                        untouched = all(bool((ra[k][M:] == -7777.0).all()) for k in ("mu", "values", "actions", "logp", "sigma", "obs", "cobs"))
                        calls += 1
                        bad += bool(diff) or not untouched
                        print(f"M={M} {'32' if big else '16'}-row {entry} plan={plan} act={with_act} packed={packed}: "
                              f"{'same bits' if not diff else 'DIFFERENT ' + ','.join(diff)}{'' if untouched else ' ROWS PAST M WRITTEN'}")
            if env is not None:
                env.close()
    print(f"{calls} launches per library, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
