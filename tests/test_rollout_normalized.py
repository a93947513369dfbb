"""CPU: the two entry points behind the fused rollout of an agent with ``empirical_normalization`` --
``imx_empirical_normalization_update`` (batch statistics as two wide launches, one or two normalisers per call) and
``imx_mlp_infer_act2n`` (the rollout inference launch that normalises its rows where it loads them) -- are declared, exported and
bound; every argument they refuse is refused on the host, before any launch, and named in ``imx_last_error``; their structs live in
``include/imx_normalization_struct.h`` (``imx.h``'s own struct table does not grow) and their sizes agree with the library's; the
normaliser's host mirror of ``count`` follows the rule the kernels apply on the device."""

import ctypes
import re

import pytest

from isaaclab_amd import _abi, _lib

UPDATE, INFER = "imx_empirical_normalization_update", "imx_mlp_infer_act2n"
# addresses that are never read: every call below is refused by the host-side checks
PTR, PTR16 = 0x10000, 0x20000


def arr(t, *v):
    return (t * len(v))(*v)


def group(**kw):
    g = dict(N=64, D=48, x_d=PTR, ldx=48, mean_d=PTR, var_d=PTR, std_d=PTR, count_d=PTR, until=-1, partials_d=PTR)
    g.update(kw)
    return _lib.ImxNormGroup(**g)


def test_the_entry_points_are_declared_exported_and_bound(libimx):
    with open(_abi.HEADER) as f:
        header = f.read()
    assert '#include "imx_normalization_struct.h"' in header
    for name in (UPDATE, INFER, "imx_empirical_normalization_partials_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(libimx, name)
    res, args, names = _abi.FUNCTIONS[UPDATE]
    assert names == ["ngroups", "groups", "stream"] and args[1] == ("imx_norm_group_t", 1, 0)
    assert getattr(libimx, UPDATE).argtypes[1] == ctypes.POINTER(_lib.ImxNormGroup)
    res, args, names = _abi.FUNCTIONS[INFER]
    two = _abi.FUNCTIONS["imx_mlp_infer_act2"]
    assert names == two[2][:-1] + ["norm", "stream"] and args[:-2] == two[1][:-1] and args[-2] == ("imx_infer_norm_t", 1, 0)
    assert getattr(libimx, INFER).argtypes[-2] == ctypes.POINTER(_lib.ImxInferNorm)
    # the entry points beside them keep their signatures
    assert len(_abi.FUNCTIONS["imx_empirical_normalization"][1]) == 11 and len(two[1]) == 15


def test_struct_sizes_agree(libimx):
    assert list(_abi.NORMALIZATION_STRUCTS) == ["imx_norm_group_t", "imx_infer_norm_t"]
    assert not set(_abi.NORMALIZATION_STRUCTS) & set(_abi.STRUCTS)
    assert [f for f, _ in _lib.ImxNormGroup._fields_] == ["N", "D", "x_d", "ldx", "mean_d", "var_d", "std_d", "count_d", "until", "partials_d"]
    assert [f for f, _ in _lib.ImxInferNorm._fields_] == ["mean_d", "std_d", "eps"]
    assert int(libimx.imx_struct_size(22)) == ctypes.sizeof(_lib.ImxNormGroup) == 80
    assert int(libimx.imx_struct_size(23)) == ctypes.sizeof(_lib.ImxInferNorm) == 24
    assert int(libimx.imx_struct_size(21)) == 0 and int(libimx.imx_struct_size(24)) == 0


def test_partials_size(libimx):
    """At most 64 slabs of at least 16 rows; (mean, M2) per slab and column, columns up to a multiple of 64."""
    size = lambda N, D: int(libimx.imx_empirical_normalization_partials_bytes(N, D))  # noqa: E731
    assert size(1, 1) == 1 * 2 * 64 * 4 and size(16, 64) == 1 * 2 * 64 * 4 and size(17, 65) == 2 * 2 * 128 * 4
    assert size(4096, 235) == 64 * 2 * 256 * 4                       # 64 slabs of 64 rows
    assert size(4097, 235) == 64 * 2 * 256 * 4                       # 65-row slabs: 64 of them
    assert size(100003, 157) == 64 * 2 * 192 * 4                     # the slab cap
    assert size(0, 5) == 0 and size(5, 0) == 0 and size(-1, 5) == 0


@pytest.mark.parametrize("ngroups,groups,named", [
    (0, [group()], r"ngroups = 0"),
    (3, [group(), group(), group()], r"ngroups = 3"),
    (1, None, r"groups is null"),
    (1, [group(x_d=None)], r"groups\[0\]\.x_d"),
    (2, [group(), group(x_d=None)], r"groups\[1\]\.x_d"),
    (1, [group(ldx=47)], r"groups\[0\]\.ldx = 47 .* 48"),
    (1, [group(mean_d=None)], r"groups\[0\].*null statistics"),
    (1, [group(var_d=None)], r"groups\[0\].*null statistics"),
    (2, [group(), group(std_d=None)], r"groups\[1\].*null statistics"),
    (1, [group(count_d=None)], r"groups\[0\].*null statistics.*count_d"),
    (1, [group(partials_d=None)], r"groups\[0\]\.partials_d"),
    (1, [group(N=0)], r"groups\[0\]: N = 0"),
    (1, [group(D=0, ldx=0)], r"groups\[0\].* D = 0"),
])
def test_update_refusals_name_the_argument_and_launch_nothing(libimx, ngroups, groups, named):
    """The refusals run on the host before the first HIP call: they return non-zero on a machine without a GPU, where a launch would have
    failed with a HIP error instead of the message."""
    g = None if groups is None else arr(_lib.ImxNormGroup, *groups)
    assert getattr(libimx, UPDATE)(ngroups, g, None) != 0
    msg = libimx.imx_last_error().decode()
    assert msg.startswith(UPDATE + ":") and re.search(named, msg), msg
    assert "hip" not in msg.lower(), msg


def infer(L, *, M=64, X=(PTR, PTR), ldx=(48, 235), nnets=2, dims=(48, 64, 12, 235, 64, 1), norm="both"):
    nlayers = (2, 2)
    nw = 4
    w, b, out = arr(ctypes.c_void_p, *([PTR16] * nw)), arr(ctypes.c_void_p, *([PTR] * nw)), arr(ctypes.c_void_p, PTR, PTR)
    pitch = [(d + 31) // 32 * 32 for d in (dims[0], dims[1], dims[3], dims[4])]
    triples = {"both": [(PTR, PTR), (PTR, PTR)], "no mean": [(0, PTR), (PTR, PTR)], "no std": [(PTR, PTR), (PTR, 0)], None: None}[norm]
    n = None if triples is None else arr(_lib.ImxInferNorm, *[_lib.ImxInferNorm(mean_d=m or None, std_d=s or None, eps=0.01) for m, s in triples])
    return getattr(L, INFER)(M, arr(ctypes.c_void_p, *X), arr(ctypes.c_int64, *ldx), nnets, arr(ctypes.c_int, *nlayers), arr(ctypes.c_int, *dims), w,
                             arr(ctypes.c_int, *pitch), None, b, arr(ctypes.c_float, 1.0, 1.0), out, None, None, n, None)


@pytest.mark.parametrize("kwargs,named", [
    (dict(norm=None), r"act2n: norm is null"),
    (dict(norm="no mean"), r"act2n: norm\[0\]: null statistics \(mean_d"),
    (dict(norm="no std"), r"act2n: norm\[1\]: null statistics \(std_d"),
    (dict(nnets=3), r"act2n: nnets = 3"),
    (dict(nnets=0), r"act2n: nnets = 0"),
    (dict(ldx=(47, 235)), r"ldx\[0\] = 47 .* 48"),
    (dict(ldx=(48, 234)), r"ldx\[1\] = 234 .* 235"),
    (dict(dims=(48, 64, 12, 513, 64, 1), ldx=(48, 513)), r"dims.* 513 .*1\.\.512"),
    (dict(dims=(513, 64, 12, 235, 64, 1), ldx=(513, 235)), r"dims.* 513 .*1\.\.512"),
    (dict(X=(0, PTR)), r"X_d\[0\]"),
    (dict(M=0), r"M = 0"),
])
def test_infer_refusals_name_the_argument_and_launch_nothing(libimx, kwargs, named):
    """(The checks it shares with ``imx_mlp_infer_act2`` answer under the name of the entry point that was called.)"""
    assert infer(libimx, **kwargs) != 0
    msg = libimx.imx_last_error().decode()
    assert msg.startswith(INFER + ":") and re.search(named, msg), msg
    assert "hip" not in msg.lower(), msg


def test_host_count_follows_the_device_rule():
    """A batch counts only while ``count < until`` -- the whole batch then, as upstream's ``update`` (and the kernels) have it."""
    import torch

    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization, update_rows_together

    n = EmpiricalNormalization([3], until=5)
    seen = []
    for _ in range(3):
        n.advance_host_count(4)
        seen.append(n._host_count)
    assert seen == [4, 8, 8]
    exact = EmpiricalNormalization([3], until=8)
    for _ in range(3):
        exact.advance_host_count(4)
    assert exact._host_count == 8  # count == until stops it: `count >= until`
    free = EmpiricalNormalization([3])
    for _ in range(3):
        free.advance_host_count(1 << 40)
    assert free._host_count == 3 << 40 and free.until is None
    # nothing is counted for a call that was refused (no GPU here: the launch is never reached)
    with pytest.raises(_lib.ImxError):
        n.update_rows(torch.zeros(4, 3))
    with pytest.raises(_lib.ImxError, match=r"row-major \(N, 3\)"):
        free.update_rows(torch.zeros(4, 4))
    with pytest.raises(_lib.ImxError):
        update_rows_together((free, torch.zeros(4, 3)), (exact, torch.zeros(4, 3)))
    assert (n._host_count, free._host_count, exact._host_count) == (8, 3 << 40, 8)
    g = free._group(torch.zeros(7, 5)[:, :3])
    assert (g.N, g.D, g.ldx, g.until) == (7, 3, 5, -1) and exact._group(torch.zeros(7, 3)).until == 8
    t = free.infer_norm()
    assert t.mean_d == free._mean.data_ptr() and t.std_d == free._std.data_ptr() and abs(t.eps - 0.01) < 1e-9


def test_runner_switch_exists():
    from isaaclab_amd.rsl_rl import OnPolicyRunner

    assert OnPolicyRunner.fuse_normalization is True and callable(OnPolicyRunner._fusable_normalized)
