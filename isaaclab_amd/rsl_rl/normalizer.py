"""``EmpiricalNormalization`` (upstream ``rsl_rl/modules/normalizer.py`` @ v2.3.1 -- third-party, absent from the reference
tree; PARITY UNPINNED, restated in oracle/rsl_rl_oracle.py).  Enabled by ``empirical_normalization=True``
(reference isaaclab_rl/rsl_rl/rl_cfg.py).  Running mean / variance update + normalisation are ``imx_empirical_normalization``; the
fused rollout takes the two halves apart: ``update_rows`` (``imx_empirical_normalization_update``) and ``apply``."""

from __future__ import annotations

import torch
import torch.nn as nn

from .. import _lib
from .._lib import check, lib


class EmpiricalNormalization(nn.Module):
    def __init__(self, shape, eps: float = 1e-2, until: int | None = None):
        super().__init__()
        self.eps, self.until = eps, until
        shape = list(shape) if isinstance(shape, (list, tuple)) else [shape]
        self.register_buffer("_mean", torch.zeros(shape).unsqueeze(0))
        self.register_buffer("_var", torch.ones(shape).unsqueeze(0))
        self.register_buffer("_std", torch.ones(shape).unsqueeze(0))
        # upstream's buffer: ``self.register_buffer("count", torch.tensor(0, dtype=torch.long))``.  Exact past 2^24 (the fp32 count it
        # replaces was not), advanced on the device: no host sync in forward.  ``_host_count`` mirrors it for the ``until`` test.
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))
        self._host_count = 0

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return self._std.squeeze(0).clone()

    def updating(self) -> bool:
        """Whether ``forward`` folds its batch into the statistics (upstream ``update``: ``if until is not None and count >= until``)."""
        return self.training and (self.until is None or self._host_count < self.until)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # checkpoints of the earlier layout hold a float (1,) "_count_f" in place of the long "count"
        old = state_dict.pop(prefix + "_count_f", None)
        if old is not None and prefix + "count" not in state_dict:
            state_dict[prefix + "count"] = old.reshape(()).round().long()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._host_count = int(self.count)  # the one sync: a resumed run stops updating at ``until`` like the one it continues

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        N, D = x.shape
        update = self.updating()
        if update:
            self._host_count += N
        out = torch.empty_like(x)
        check(lib().imx_empirical_normalization(N, D, x.data_ptr(), int(update), float(self.eps), self._mean.data_ptr(),
                                                self._var.data_ptr(), self._std.data_ptr(), self.count.data_ptr(),
                                                out.data_ptr(), _lib.current_stream(x.device)))
        return out

    # ---- the two halves of ``forward`` on their own (the fused rollout: statistics after the env step, rows normalised where the
    # inference launch loads them) -------------------------------------------------------------------------------------------------
    def advance_host_count(self, N: int) -> None:
        """``_host_count`` by the rule the statistics kernels apply to ``count`` on the device: a batch counts only while
        ``count < until`` (a graph replay runs the kernels without running ``update_rows``)."""
        if self.until is None or self._host_count < self.until:
            self._host_count += N

    def _group(self, x: torch.Tensor) -> "_lib.ImxNormGroup":
        if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != self._mean.shape[1]:
            raise _lib.ImxError(f"update_rows needs row-major (N, {self._mean.shape[1]}) rows, not {tuple(x.shape)} with strides {x.stride()}")
        N, D = x.shape
        need = int(lib().imx_empirical_normalization_partials_bytes(N, D)) // 4
        part = getattr(self, "_partials", None)
        if part is None or part.numel() < need or part.device != x.device:
            self._partials = part = torch.empty(need, device=x.device, dtype=torch.float32)
        return _lib.ImxNormGroup(N=N, D=D, x_d=x.data_ptr(), ldx=x.stride(0), mean_d=self._mean.data_ptr(), var_d=self._var.data_ptr(),
                                 std_d=self._std.data_ptr(), count_d=self.count.data_ptr(), until=-1 if self.until is None else int(self.until),
                                 partials_d=part.data_ptr())

    def update_rows(self, x: torch.Tensor, advance_host: bool = True) -> None:
        """Fold the batch into the statistics (``imx_empirical_normalization_update``: two launches); whether it counts is decided
        on the device (``count >= until``: nothing happens).  ``advance_host`` False: under graph capture, where nothing runs."""
        update_rows_together((self, x), advance_host=advance_host)

    def apply(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """``(x - mean) / (std + eps)`` with the statistics as they are (``imx_empirical_normalization`` with ``update = 0``)."""
        x = x.contiguous()
        N, D = x.shape
        if out is None:
            out = torch.empty_like(x)
        elif not out.is_contiguous() or out.shape != x.shape:
            raise _lib.ImxError(f"apply: out must be contiguous {tuple(x.shape)}")
        check(lib().imx_empirical_normalization(N, D, x.data_ptr(), 0, float(self.eps), self._mean.data_ptr(), self._var.data_ptr(),
                                                self._std.data_ptr(), self.count.data_ptr(), out.data_ptr(), _lib.current_stream(x.device)))
        return out

    def infer_norm(self) -> "_lib.ImxInferNorm":
        """The {mean, std, eps} triple ``imx_mlp_infer_act2n`` normalises a network's rows with."""
        return _lib.ImxInferNorm(mean_d=self._mean.data_ptr(), std_d=self._std.data_ptr(), eps=float(self.eps))

    @torch.jit.unused
    def inverse(self, y):
        return y * (self._std + self.eps) + self._mean


def update_rows_together(*pairs, advance_host: bool = True) -> None:
    """``update_rows`` of one or two ``(normaliser, rows)`` pairs in ONE ``imx_empirical_normalization_update`` call (the policy and
    the critic group of an env step share the two launches)."""
    groups = (_lib.ImxNormGroup * len(pairs))(*[n._group(x) for n, x in pairs])
    check(lib().imx_empirical_normalization_update(len(pairs), groups, _lib.current_stream(pairs[0][1].device)))
    if advance_host:
        for n, x in pairs:
            n.advance_host_count(x.shape[0])
