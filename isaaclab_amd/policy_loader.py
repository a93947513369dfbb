"""The low-level policy of a ``PreTrainedPolicyAction``: a TorchScript archive, an ``nn.Module`` or a list of ``(W, b)`` pairs -> the
Linear layers the fused kernel runs (``imx_pretrained_policy``).  Host side only; nothing is ever fetched.

The reference loads ``cfg.policy_path`` with ``torch.jit.load`` and calls the module (isaaclab_tasks .../navigation/mdp/
pre_trained_policy_action.py:41-45, 96).  Here the module is taken apart once: what comes out must be an MLP of at most four Linear
layers up to 512 wide with one ELU alpha between them (``imx_mlp_infer``'s limits); anything else is refused with the reason."""

from __future__ import annotations

import dataclasses
import os
from typing import Any

import torch

from . import _lib

MAX_LAYERS = _lib.PP_MAX_LAYERS
MAX_WIDTH = 512
CHECK_ROWS, CHECK_TOL = 8, 1.0e-6


class PolicyError(NotImplementedError):
    """A low-level policy the fused path cannot take."""


@dataclasses.dataclass
class PolicyLayers:
    layers: list  # [(W (out, in) fp32 cpu, b (out) fp32 cpu)]
    elu_alpha: float = 1.0
    source: str = ""

    @property
    def dims(self) -> list[int]:
        return [int(self.layers[0][0].shape[1])] + [int(w.shape[0]) for w, _ in self.layers]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The layers in torch, in ``x``'s dtype (the comparator of the load-time check and of the tests' restatement)."""
        for i, (w, b) in enumerate(self.layers):
            x = torch.nn.functional.linear(x, w.to(x.dtype), b.to(x.dtype))
            if i + 1 < len(self.layers):
                x = torch.nn.functional.elu(x, alpha=self.elu_alpha)
        return x


def resolve_policy_path(path: Any, term: str = "pre_trained_policy_action") -> str:
    """``check_file_path`` (isaaclab/utils/assets.py:37-56) for a local file; a path that is no local file raises the reference's
    ``FileNotFoundError`` (pre_trained_policy_action.py:42-43) -- a Nucleus URL is never fetched."""
    if not isinstance(path, (str, os.PathLike)) or not os.path.isfile(path):
        raise FileNotFoundError(f"Policy file '{path}' does not exist. (action term '{term}': only a local file is read, nothing is "
                                "fetched; pass the policy as low_level_policy= -- a path, an nn.Module or a list of (W, b) pairs)")
    return os.fspath(path)


def _kind(m) -> str:
    return getattr(m, "original_name", None) or type(m).__name__


def _sequential_layers(seq, where: str) -> tuple[list, float]:
    kinds = [(_kind(c), c) for _, c in seq.named_children()]
    layers, alphas = [], []
    expect_linear = True
    for kind, c in kinds:
        if kind not in ("Linear", "ELU"):
            raise PolicyError(f"low-level policy: {where} holds a {kind}; the fused path runs Linear layers with ELU between them")
        if (kind == "Linear") != expect_linear:
            raise PolicyError(f"low-level policy: {where} is not Linear (ELU Linear)*: {[k for k, _ in kinds]}")
        if kind == "Linear":
            w, b = c.weight.detach().to("cpu", torch.float32), getattr(c, "bias", None)
            if b is None:
                b = torch.zeros(w.shape[0])
            layers.append((w.contiguous(), b.detach().to("cpu", torch.float32).contiguous()))
        else:
            alphas.append(float(c.alpha))
        expect_linear = kind != "Linear"
    if not layers or expect_linear:
        raise PolicyError(f"low-level policy: {where} must end with a Linear layer: {[k for k, _ in kinds]}")
    if len(set(alphas)) > 1:
        raise PolicyError(f"low-level policy: {where} has ELU alphas {sorted(set(alphas))}; the fused path carries one")
    return layers, (alphas[0] if alphas else 1.0)


def _from_module(m, source: str) -> PolicyLayers:
    if _kind(m) == "Sequential":
        layers, alpha = _sequential_layers(m, "the Sequential")
        return PolicyLayers(layers, alpha, source)
    children = dict(m.named_children())
    if "actor" not in children or _kind(children["actor"]) != "Sequential":
        raise PolicyError(f"low-level policy: a {_kind(m)} with children {list(children)}; an `actor` Sequential with an Identity "
                          "`normalizer` (the exporter's structure, isaaclab_rl/rsl_rl/exporter.py) or a bare Sequential is taken")
    for name, c in children.items():
        if name == "actor":
            continue
        if name == "normalizer":
            if _kind(c) != "Identity":
                raise PolicyError(f"low-level policy: the normalizer is a {_kind(c)}; only the exporter's Identity is on the fused path")
            continue
        raise PolicyError(f"low-level policy: child module '{name}' ({_kind(c)}) beside the actor -- a recurrent policy is not on the "
                          "fused path")
    layers, alpha = _sequential_layers(children["actor"], "the actor")
    return PolicyLayers(layers, alpha, source)


def _check_limits(p: PolicyLayers) -> PolicyLayers:
    if len(p.layers) > MAX_LAYERS:
        raise PolicyError(f"low-level policy: {len(p.layers)} Linear layers; the fused path takes at most {MAX_LAYERS}")
    for i, (w, b) in enumerate(p.layers):
        if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise PolicyError(f"low-level policy: layer {i} has weight {tuple(w.shape)} and bias {tuple(b.shape)}")
        if i and w.shape[1] != p.layers[i - 1][0].shape[0]:
            raise PolicyError(f"low-level policy: layer {i} takes {w.shape[1]} inputs, layer {i - 1} gives {p.layers[i - 1][0].shape[0]}")
    wide = [d for d in p.dims if not 1 <= d <= MAX_WIDTH]
    if wide:
        raise PolicyError(f"low-level policy: layer width {wide[0]}; the fused path takes widths up to {MAX_WIDTH}")
    return p


def load_policy(source: Any, term: str = "pre_trained_policy_action") -> PolicyLayers:
    """``source``: the path of a TorchScript archive (loaded on the CPU), an ``nn.Module`` (scripted or not) or a list of ``(W, b)``.
    A module's extracted layers are run on ``CHECK_ROWS`` random rows against the module itself: a mismatch above ``CHECK_TOL`` raises
    (a misparsed archive must not run)."""
    if isinstance(source, (list, tuple)):
        layers = [(torch.as_tensor(w, dtype=torch.float32).detach().cpu().contiguous(), torch.as_tensor(b, dtype=torch.float32).detach().cpu().contiguous())
                  for w, b in source]
        if not layers:
            raise PolicyError("low-level policy: an empty list of layers")
        return _check_limits(PolicyLayers(layers, 1.0, "layers"))
    if isinstance(source, (str, os.PathLike)):
        path = resolve_policy_path(source, term)
        try:
            module = torch.jit.load(path, map_location="cpu").eval()
        except (RuntimeError, ValueError) as e:
            raise PolicyError(f"low-level policy: '{path}' is no TorchScript archive torch.jit.load reads ({str(e).splitlines()[0]})") from e
        name = path
    elif isinstance(source, torch.nn.Module):
        module, name = source, type(source).__name__
    else:
        raise TypeError(f"low_level_policy: a path, an nn.Module or a list of (W, b) pairs, not {type(source).__name__}")
    p = _check_limits(_from_module(module, name))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(CHECK_ROWS, p.dims[0], generator=g)
    with torch.no_grad():
        try:
            ref = module.to("cpu")(x) if not isinstance(source, (str, os.PathLike)) else module(x)
        except Exception as e:  # noqa: BLE001  (whatever the module raises on a (8, in) batch)
            raise PolicyError(f"low-level policy: the module does not take a ({CHECK_ROWS}, {p.dims[0]}) batch ({e})") from e
        err = float((p.forward(x) - ref).abs().max())
    if not err <= CHECK_TOL:
        raise PolicyError(f"low-level policy: the extracted layers differ from the module by {err:.3g} on {CHECK_ROWS} random rows "
                          f"(more than {CHECK_TOL}): the archive holds more than Linear + ELU")
    return p


class DevicePolicy:
    """The layers on the device as ``imx_mlp_infer`` / ``imx_pretrained_policy`` take them: rows zero-padded to a pitch that is a multiple
    of 32 floats, and the packed image of the 32-row kernel; uploaded once."""

    def __init__(self, p: PolicyLayers, device):
        import ctypes

        L = _lib.lib()
        self.layers, self.device = p, torch.device(device)
        self.dims, self.nlayers, self.elu_alpha = p.dims, len(p.layers), float(p.elu_alpha)
        self.weights, self.biases, self.packed, self.pitch = [], [], [], []
        stream = _lib.current_stream(self.device)
        for w, b in p.layers:
            n, k = w.shape
            pitch = (k + 31) // 32 * 32
            wp = torch.zeros(n, pitch, device=self.device)
            wp[:, :k] = w.to(self.device)
            pk = torch.zeros(int(L.imx_mlp_packed_floats(n, k)), device=self.device)
            _lib.check(L.imx_mlp_pack_weights(n, k, wp.data_ptr(), pitch, pk.data_ptr(), stream))
            self.weights.append(wp)
            self.biases.append(b.to(self.device).contiguous())
            self.packed.append(pk)
            self.pitch.append(pitch)
        n = self.nlayers
        c = _lib.ImxPretrainedPolicy(nlayers=n, elu_alpha=self.elu_alpha)
        for i, d in enumerate(self.dims):
            c.dims[i] = d
        for i in range(n):
            c.weight_pitch[i] = self.pitch[i]
            c.weights_d[i], c.packed_weights_d[i], c.biases_d[i] = self.weights[i].data_ptr(), self.packed[i].data_ptr(), self.biases[i].data_ptr()
        self.struct = c
        # imx_mlp_infer's argument arrays (the unfused chain)
        self._nl = (ctypes.c_int * 1)(n)
        self._dims = (ctypes.c_int * (n + 1))(*self.dims)
        self._w = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.weights])
        self._b = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.biases])
        self._pitch = (ctypes.c_int * n)(*self.pitch)
        self._alpha = (ctypes.c_float * 1)(self.elu_alpha)

    def infer(self, x: torch.Tensor, out: torch.Tensor):
        """``imx_mlp_infer`` on (N, dims[0]) rows -> ``out`` (N, dims[-1]): the second launch of the unfused chain."""
        import ctypes

        o = (ctypes.c_void_p * 1)(out.data_ptr())
        _lib.check(_lib.lib().imx_mlp_infer(x.shape[0], x.data_ptr(), x.stride(0), 1, self._nl, self._dims, self._w, self._pitch, self._b,
                                            self._alpha, o, _lib.current_stream(self.device)))
