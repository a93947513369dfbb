"""CPU: ``imx_mlp_infer_act2`` -- rollout inference for two networks that do not share their input (an env with a "critic" observation
group) -- is declared in include/imx.h, exported and bound; every argument it refuses is refused on the host, before any launch, with the
argument named in ``imx_last_error``; no ABI struct moved; ``FusedInference`` makes a two-input instance of such a pair of stacks and
says so when it is called the wrong way."""

import ctypes
import re

import pytest

from isaaclab_amd import _abi, _lib

NAME = "imx_mlp_infer_act2"
# addresses that are never read: every call below is refused by the host-side checks
PTR, PTR16, ODD = 0x10000, 0x20000, 0x20004


def arr(t, *v):
    return (t * len(v))(*v)


def call(L, *, M=64, X=(PTR, PTR), ldx=(48, 235), nnets=2, nlayers=(2, 2), dims=(48, 64, 12, 235, 64, 1), packed=None, critic_out=None,
         weight=PTR16, pitch=None):
    nw = sum(nlayers[:max(nnets, 0)]) if nnets in (1, 2) else 2
    w = arr(ctypes.c_void_p, *([weight] * nw))
    b = arr(ctypes.c_void_p, *([PTR] * nw))
    out = arr(ctypes.c_void_p, PTR, PTR)
    if pitch is None:  # zero-padded rows, a multiple of 32 floats
        widths, i = [], 0
        for k in range(nnets if nnets in (1, 2) else 0):
            widths += [(d + 31) // 32 * 32 for d in dims[i:i + nlayers[k]]]
            i += nlayers[k] + 1
        pitch = widths or [32] * nw
    return L.imx_mlp_infer_act2(M, None if X is None else arr(ctypes.c_void_p, *X), None if ldx is None else arr(ctypes.c_int64, *ldx), nnets,
                                arr(ctypes.c_int, *nlayers), arr(ctypes.c_int, *dims), w, arr(ctypes.c_int, *pitch),
                                None if packed is None else arr(ctypes.c_void_p, *packed), b, arr(ctypes.c_float, 1.0, 1.0), out, None,
                                critic_out, None)


def test_the_entry_point_is_declared_exported_and_bound(libimx):
    with open(_abi.HEADER) as f:
        header = f.read()
    assert re.search(r"\bint\s+imx_mlp_infer_act2\s*\(", header)
    res, args, names = _abi.FUNCTIONS[NAME]
    assert names == ["M", "X_d", "ldx", "nnets", "nlayers", "dims", "weights_d", "weight_pitch", "packed_weights_d", "biases_d", "elu_alpha",
                     "out_d", "act", "critic_obs_out_d", "stream"]
    assert args[1] == ("float", 2, 0) and args[2] == ("int64_t", 1, 0) and args[12] == ("imx_policy_act_t", 1, 0) and args[13] == ("float", 1, 0)
    assert NAME in _lib.EXPORTS and hasattr(libimx, NAME)
    fn = getattr(libimx, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[0] is ctypes.c_int64 and fn.argtypes[12] == ctypes.POINTER(_lib.ImxPolicyAct)
    # the two entry points beside it keep their signatures
    assert len(_abi.FUNCTIONS["imx_mlp_infer"][1]) == 12 and len(_abi.FUNCTIONS["imx_mlp_infer_act"][1]) == 14
    assert _abi.FUNCTIONS["imx_mlp_infer_act"][1][1] == ("float", 1, 0) and _abi.FUNCTIONS["imx_mlp_infer_act"][1][2] == ("int64_t", 0, 0)


@pytest.mark.parametrize("kwargs,named", [
    (dict(X=(0, PTR)), r"X_d\[0\]"),
    (dict(X=(PTR, 0)), r"X_d\[1\]"),
    (dict(X=None), r"X_d"),
    (dict(ldx=None), r"ldx"),
    (dict(ldx=(47, 235)), r"ldx\[0\] = 47 .* 48"),
    (dict(ldx=(48, 234)), r"ldx\[1\] = 234 .* 235"),
    (dict(dims=(0, 64, 12, 235, 64, 1), ldx=(48, 235)), r"dims.* 0 .*1\.\.512"),
    (dict(dims=(48, 64, 12, 513, 64, 1), ldx=(48, 513)), r"dims.* 513 .*1\.\.512"),
    (dict(dims=(48, 64, 12, -3, 64, 1)), r"dims.* -3 .*1\.\.512"),
    (dict(nnets=1, critic_out=PTR), r"critic_obs_out_d .*nnets == 1"),
    (dict(packed=(PTR16, PTR16, ODD, PTR16)), r"packed_weights_d\[2\]"),
    (dict(packed=(PTR16, 0, PTR16, PTR16)), r"packed_weights_d\[1\]"),
    (dict(nnets=3), r"nnets = 3"),
    (dict(M=0), r"M = 0"),
])
def test_every_refused_argument_is_named_and_nothing_is_launched(libimx, kwargs, named):
    """The refusals run on the host before the first HIP call: they return non-zero on a machine without a GPU, where a launch (or a
    device query) would have failed with a HIP error instead of the message."""
    assert call(libimx, **kwargs) != 0
    msg = libimx.imx_last_error().decode()
    assert msg.startswith(NAME + ":") and re.search(named, msg), msg
    assert "hip" not in msg.lower(), msg


def test_the_shared_input_entry_points_keep_their_checks(libimx):
    """``imx_mlp_infer`` / ``imx_mlp_infer_act`` still refuse two networks of different input widths, in their own words."""
    w = arr(ctypes.c_void_p, *([PTR16] * 4))
    b = arr(ctypes.c_void_p, *([PTR] * 4))
    out = arr(ctypes.c_void_p, PTR, PTR)
    args = (2, arr(ctypes.c_int, 2, 2), arr(ctypes.c_int, 48, 64, 12, 235, 64, 1), w, arr(ctypes.c_int, 64, 64, 256, 64))
    assert libimx.imx_mlp_infer(64, PTR, 235, *args, b, arr(ctypes.c_float, 1.0, 1.0), out, None) != 0
    assert "imx_mlp_infer: the networks must share the input (width 48, pitch 235)" == libimx.imx_last_error().decode()
    assert libimx.imx_mlp_infer_act(64, PTR, 235, *args, None, b, arr(ctypes.c_float, 1.0, 1.0), out, None, None) != 0
    assert "imx_mlp_infer: the networks must share the input (width 48, pitch 235)" == libimx.imx_last_error().decode()
    assert libimx.imx_mlp_infer(64, None, 48, *args, b, arr(ctypes.c_float, 1.0, 1.0), out, None) != 0
    assert "imx_mlp_infer: bad arguments" == libimx.imx_last_error().decode()


def test_no_struct_moved(libimx):
    assert len(_abi.STRUCTS) == 8 and "imx_policy_act_t" in _abi.STRUCTS
    assert int(libimx.imx_struct_size(4)) == ctypes.sizeof(_lib.ImxPolicyAct) == 96
    assert [n for n, _ in _lib.ImxPolicyAct._fields_] == ["std_d", "seed", "step_counter_d", "actions_out_d", "logp_out_d", "mu_out_d", "sigma_out_d",
                                                          "obs_out_d", "plan", "state", "buf", "pre_clip"]
    # the sizes other tests pin
    assert int(libimx.imx_struct_size(0)) == ctypes.sizeof(_lib.ImxState) == 248 and int(libimx.imx_struct_size(1)) == 216
    assert int(libimx.imx_struct_size(5)) == 1944 and int(libimx.imx_struct_size(6)) == 176
    assert int(libimx.imx_struct_size(3)) == ctypes.sizeof(_lib.ImxRolloutSlot)
    assert all(int(libimx.imx_struct_size(k)) == 0 for k in (9, 14, 17, 19, 21))


def test_fused_inference_of_stacks_with_different_inputs_is_a_two_input_instance():
    """Built on the CPU up to the first library call that needs a device: the instance's shape logic and its refusals."""
    import torch

    from isaaclab_amd.rsl_rl.actor_critic import ActorCritic
    from isaaclab_amd.rsl_rl.ppo import FusedInference, _mlp_layers

    class Built(FusedInference):
        def refresh(self):  # (the padded / packed copies need a GPU)
            pass

    pol = ActorCritic(48, 235, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[96])
    two = Built(_mlp_layers(pol.actor), _mlp_layers(pol.critic))
    assert two.ok and two.two_inputs and (two.in_features, two.critic_in_features) == (48, 235)
    assert list(two._nl) == [4, 2] and list(two._dims) == [48, 128, 64, 32, 12, 235, 96, 1]
    assert list(two._pitch) == [64, 128, 64, 32, 256, 96]  # per layer, as before: in-features up to a multiple of 32
    same = ActorCritic(48, 48, 12, actor_hidden_dims=[64], critic_hidden_dims=[64])
    shared = Built(_mlp_layers(same.actor), _mlp_layers(same.critic))
    assert shared.ok and not shared.two_inputs
    assert Built(_mlp_layers(same.actor), _mlp_layers(same.critic), two_inputs=True).two_inputs  # a critic group as wide as the policy's
    assert not Built(_mlp_layers(same.critic), two_inputs=True).two_inputs                       # one network has one input
    x, cx = torch.zeros(4, 48), torch.zeros(4, 235)
    mu, v = torch.zeros(4, 12), torch.zeros(4, 1)
    with pytest.raises(_lib.ImxError, match="needs critic_x"):
        two(x, mu, v)
    with pytest.raises(_lib.ImxError, match="critic_x must be row-major"):
        two(x, mu, v, critic_x=torch.zeros(4, 234))
    with pytest.raises(_lib.ImxError, match="critic_obs_out must be contiguous"):
        two(x, mu, v, critic_x=cx, critic_obs_out=torch.zeros(4, 236)[:, :235])
    with pytest.raises(_lib.ImxError, match="shared-input"):
        shared(x, mu, v, critic_x=x)
    with pytest.raises(_lib.ImxError, match="shared-input"):
        shared(x, mu, v, critic_obs_out=x)
    wide = ActorCritic(48, 600, 12, actor_hidden_dims=[64], critic_hidden_dims=[64])
    assert not Built(_mlp_layers(wide.actor), _mlp_layers(wide.critic)).ok  # a critic input over 512 columns: the library path
