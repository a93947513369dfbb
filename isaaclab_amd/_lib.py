"""ctypes binding of libimx.so, derived from ``include/imx.h``: the struct layouts, the signature of every exported function and the
constants below are what ``_abi`` parsed out of the header, which is the only place the ABI is written (tests/test_abi.py has a C++
compiler check the derivation).  There is NO fallback: if the library cannot be loaded the product path raises -- a silent eager/CPU
path would void every parity and performance claim."""

from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int32

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libimx.so")

ORCH_MAX_TERMS = _abi.DEFINES["IMX_ORCH_MAX_TERMS"]
ORCH_MAX_WEIGHT_TERMS = _abi.DEFINES["IMX_ORCH_MAX_WEIGHT_TERMS"]
IK_MAX_JOINTS = _abi.DEFINES["IMX_IK_MAX_JOINTS"]
OSC_CMD_WIDTH = _abi.DEFINES["IMX_OSC_CMD_WIDTH"]
PP_MAX_LAYERS = _abi.DEFINES["IMX_PP_MAX_LAYERS"]
_STRUCTS = {}  # typedef name -> class


def _struct(cname: str, cls=None):
    """The ``ctypes.Structure`` of an ABI struct (``imx_head_loss_t`` -> ``ImxHeadLoss``); one that holds another by value comes after it."""
    cls = cls or type("".join(w.capitalize() for w in cname[:-2].split("_")), (ctypes.Structure,), {})
    cls._fields_ = [(field, _abi.ctype(t, _STRUCTS)) for field, t in _abi.STRUCTS[cname]]
    _STRUCTS[cname] = cls
    return cls


class ImxDiffIk(ctypes.Structure):  # imx_diff_ik_t
    @classmethod
    def from_term(cls, ik) -> "ImxDiffIk":
        """The C struct of a ``plan.IkTerm``."""
        n = len(ik.joint_ids)
        if not 1 <= n <= IK_MAX_JOINTS:
            raise ImxError(f"action term '{ik.name}': {n} controlled joints (1..{IK_MAX_JOINTS})")
        pos, rot = ik.offset_pos or (0.0, 0.0, 0.0), ik.offset_rot or (1.0, 0.0, 0.0, 0.0)
        return cls(command_type=_abi.ENUMS["imx_ik_command"]["IMX_IK_" + ik.command_type.upper()], use_relative_mode=int(ik.use_relative_mode),
                   ik_method=_abi.ENUMS["imx_ik_method"]["IMX_IK_" + ik.ik_method.upper()], has_offset=int(ik.offset_pos is not None), lambda_val=ik.lambda_val,
                   k_val=ik.k_val, offset_pos=(c_float * 3)(*pos), offset_rot=(c_float * 4)(*rot), body_idx=ik.body_idx,
                   jacobi_body_idx=ik.jacobi_body_idx, num_joints=n, joint_ids=(c_int32 * IK_MAX_JOINTS)(*ik.joint_ids),
                   jacobi_joint_ids=(c_int32 * IK_MAX_JOINTS)(*ik.jacobi_joint_ids), processed_col=ik.processed_col)


class ImxOsc(ctypes.Structure):  # imx_osc_t
    @classmethod
    def from_term(cls, t) -> "ImxOsc":
        """The C struct of a ``plan.OscTerm``."""
        import math

        n = len(t.joint_ids)
        if not 1 <= n <= IK_MAX_JOINTS:
            raise ImxError(f"action term '{t.name}': {n} controlled joints (1..{IK_MAX_JOINTS})")
        E = _abi.ENUMS
        pos, rot = t.offset_pos or (0.0, 0.0, 0.0), t.offset_rot or (1.0, 0.0, 0.0, 0.0)
        col = lambda i: -1 if i is None else t.processed_col + i  # noqa: E731
        f6 = lambda v: (c_float * 6)(*v)  # noqa: E731
        kp = c_float(t.nullspace_stiffness).value  # torch.tensor(nullspace_stiffness): fp32 before the square root (:135-140)
        kd = c_float(c_float(2.0 * c_float(math.sqrt(kp)).value).value * c_float(t.nullspace_damping_ratio).value).value
        return cls(pose_type=E["imx_osc_pose"]["IMX_OSC_" + t.pose_type.upper()], has_wrench=int(t.wrench_idx is not None),
                   impedance_mode=E["imx_osc_impedance"]["IMX_OSC_" + t.impedance_mode.upper()],
                   decoupling=E["imx_osc_decoupling"]["IMX_OSC_DECOUPLING_" + t.decoupling.upper()],
                   gravity_compensation=int(t.gravity_compensation), nullspace_position=int(t.nullspace_control == "position"),
                   has_offset=int(t.offset_pos is not None), pose_col=col(t.pose_idx), wrench_col=col(t.wrench_idx),
                   stiffness_col=col(t.stiffness_idx), damping_ratio_col=col(t.damping_ratio_idx), motion_axes=f6(t.motion_control_axes),
                   wrench_axes=f6(t.contact_wrench_control_axes), motion_stiffness=f6(t.motion_stiffness),
                   motion_damping_ratio=f6(t.motion_damping_ratio), stiffness_limits=(c_float * 2)(*t.motion_stiffness_limits),
                   damping_ratio_limits=(c_float * 2)(*t.motion_damping_ratio_limits), nullspace_kp=kp, nullspace_kd=kd,
                   offset_pos=(c_float * 3)(*pos), offset_rot=(c_float * 4)(*rot), body_idx=t.body_idx, jacobi_body_idx=t.jacobi_body_idx,
                   num_joints=n, joint_ids=(c_int32 * IK_MAX_JOINTS)(*t.joint_ids), jacobi_joint_ids=(c_int32 * IK_MAX_JOINTS)(*t.jacobi_joint_ids))


ImxState = _struct("imx_state_t")
ImxBuffers = _struct("imx_buffers_t")
ImxRolloutSlot = _struct("imx_rollout_slot_t")
ImxEventTerm = _struct("imx_event_term_t")
ImxOrch = _struct("imx_orch_t")
ImxPolicyAct = _struct("imx_policy_act_t")
ImxHeadLoss = _struct("imx_head_loss_t")
_struct("imx_diff_ik_t", ImxDiffIk)
ImxOsc._fields_ = [(field, _abi.ctype(t, _STRUCTS)) for field, t in _abi.OSC_STRUCTS["imx_osc_t"]]  # (imx_osc_struct.h: imx.h only declares the type)
# (imx_orch_manip.h, the same way; the holder after the struct it holds by value)
ImxWeightTerm = type("ImxWeightTerm", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS)) for field, t in _abi.MANIP_STRUCTS["imx_weight_term_t"]]})
ImxOrchManip = type("ImxOrchManip", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, {**_STRUCTS, "imx_weight_term_t": ImxWeightTerm}))
                                                                      for field, t in _abi.MANIP_STRUCTS["imx_orch_manip_t"]]})
# (imx_pretrained_policy_struct.h, the same way)
ImxPretrainedPolicy = type("ImxPretrainedPolicy", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                                    for field, t in _abi.POLICY_STRUCTS["imx_pretrained_policy_t"]]})
# (imx_pose2d_struct.h, the same way)
ImxPose2dCommand = type("ImxPose2dCommand", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                              for field, t in _abi.POSE2D_STRUCTS["imx_pose2d_command_t"]]})
# (imx_inhand_command_struct.h, the same way)
ImxInhandCommand = type("ImxInhandCommand", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                              for field, t in _abi.INHAND_STRUCTS["imx_inhand_command_t"]]})
# (imx_object_state.h, the same way)
ImxObjectState = type("ImxObjectState", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                          for field, t in _abi.OBJECT_STATE_STRUCTS["imx_object_state_t"]]})
OBJECT_STATE_FIELDS = tuple(field for field, _ in ImxObjectState._fields_)
# (imx_articulation_state.h, the same way)
ImxArticulationState = type("ImxArticulationState", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                                      for field, t in _abi.ARTICULATION_STATE_STRUCTS["imx_articulation_state_t"]]})
ARTICULATION_STATE_FIELDS = tuple(field for field, _ in ImxArticulationState._fields_)
# (imx_orch_articulation.h, the same way)
ImxOrchArticulation = type("ImxOrchArticulation", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                                    for field, t in _abi.ORCH_ARTICULATION_STRUCTS["imx_orch_articulation_t"]]})
# (imx_normalization_struct.h, the same way)
ImxNormGroup = type("ImxNormGroup", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                      for field, t in _abi.NORMALIZATION_STRUCTS["imx_norm_group_t"]]})
ImxInferNorm = type("ImxInferNorm", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                      for field, t in _abi.NORMALIZATION_STRUCTS["imx_infer_norm_t"]]})
# (imx_ray_caster_struct.h, the same way)
ImxRayCaster = type("ImxRayCaster", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS))
                                                                      for field, t in _abi.RAY_CASTER_STRUCTS["imx_ray_caster_t"]]})
# (imx_imu_struct.h, the same way)
ImxImu = type("ImxImu", (ctypes.Structure,), {"_fields_": [(field, _abi.ctype(t, _STRUCTS)) for field, t in _abi.IMU_STRUCTS["imx_imu_t"]]})
MAX_IMU = _abi.DEFINES["IMX_MAX_IMU"]
FRAME_WORDS = _abi.DEFINES["IMX_FRAME_WORDS"]
FT_HEADER_WORDS = _abi.DEFINES["IMX_FT_HEADER_WORDS"]
if set(_STRUCTS) != set(_abi.STRUCTS):
    raise _abi.AbiError(f"{_abi.HEADER}: no class for {sorted(set(_abi.STRUCTS) - set(_STRUCTS))}")
STATE_FIELDS = tuple(field for field, _ in ImxState._fields_)
BUFFER_FIELDS = tuple(field for field, _ in ImxBuffers._fields_)


class ImxError(RuntimeError):
    pass


_lib = None

_BY_POINTER = {**_STRUCTS, "imx_pretrained_policy_t": ImxPretrainedPolicy, "imx_pose2d_command_t": ImxPose2dCommand,
               "imx_inhand_command_t": ImxInhandCommand, "imx_object_state_t": ImxObjectState,
               "imx_articulation_state_t": ImxArticulationState,
               "imx_orch_articulation_t": ImxOrchArticulation, "imx_norm_group_t": ImxNormGroup,
               "imx_infer_norm_t": ImxInferNorm, "imx_ray_caster_t": ImxRayCaster, "imx_imu_t": ImxImu}  # (a struct of an included header travels as POINTER(class) too)
_SIGNATURES = {name: (_abi.ctype(res, _BY_POINTER, ret=True), [_abi.ctype(t, _BY_POINTER) for t in args])
               for name, (res, args, _) in _abi.FUNCTIONS.items()}
EXPORTS = tuple(_SIGNATURES)


def lib():
    """Load libimx.so (building it when hipcc is available and the library is stale or missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from . import build as _build

        _build.build()
    # torch first: libimx.so must bind to the HIP runtime torch ships and has (or will have) initialised -- loaded on its own it pulls
    # /opt/rocm's libamdhip64 in, and a process with two HIP runtimes sees no GPU from the second one ("no GPU visible")
    import torch  # noqa: F401

    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # fail loudly: never substitute another implementation
        raise ImxError(f"cannot load {LIB_PATH}: {e}. Run `python -m isaaclab_amd.build` (hipcc, gfx950).") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    for which, cls in (*enumerate((ImxState, ImxBuffers, ImxHeadLoss, ImxRolloutSlot, ImxPolicyAct, ImxOrch, ImxEventTerm, ImxDiffIk, ImxOsc)),
                       (10, ImxOrchManip), (11, ImxWeightTerm), (12, ImxPretrainedPolicy), (13, ImxPose2dCommand), (15, ImxInhandCommand), (16, ImxObjectState),
                       (18, ImxArticulationState), (20, ImxOrchArticulation), (22, ImxNormGroup),
                       (23, ImxInferNorm), (25, ImxRayCaster), (27, ImxImu)):  # the binding's struct layouts against the library's (indices 9, 14, 17, 19, 21, 24 and 26 are unknown)
        if int(L.imx_struct_size(which)) != ctypes.sizeof(cls):
            raise ImxError(f"{LIB_PATH}: sizeof({cls.__name__}) is {int(L.imx_struct_size(which))} in the library, {ctypes.sizeof(cls)} in the "
                           "binding -- rebuild with `python -m isaaclab_amd.build`")
    _lib = L
    return L


def check(status: int):
    if status != 0:
        raise ImxError(lib().imx_last_error().decode())


def ptr(t) -> int | None:
    """Device/host pointer of a contiguous torch tensor (None stays NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ImxError("libimx needs contiguous tensors")
    return t.data_ptr()


def current_stream(device) -> int:
    import torch

    if device.type != "cuda":
        raise ImxError("libimx kernels only run on a GPU (device=%s)" % device)
    return torch.cuda.current_stream(device).cuda_stream
