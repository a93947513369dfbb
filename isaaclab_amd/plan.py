"""Term compiler: a reference env cfg (live ``@configclass`` object or its ``to_dict()``/JSON form) -> libimx plan blob.

Replaces the init-time work of the reference managers -- ``ManagerBase._resolve_common_term_cfg`` /
``_process_term_cfg_at_play`` (isaaclab/managers/manager_base.py:278-395), ``SceneEntityCfg.resolve``
(managers/scene_entity_cfg.py:112-250), ``ObservationManager._prepare_terms`` (observation_manager.py:337-470),
``RewardManager._prepare_terms`` (reward_manager.py:211-250), ``TerminationManager._prepare_terms``
(termination_manager.py:198-230), ``ActionManager._prepare_terms`` (action_manager.py:365-393) -- and keys the fused
ops on the *qualified function name* of each term (``"module:function"``, the form ``configclass.to_dict`` emits,
isaaclab/utils/dict.py:23-72).  Terms whose function is unknown are routed to ``IMX_*_EXTERNAL`` and evaluated by
calling the Python term (correct, slow) -- see ``env.py``.
"""

from __future__ import annotations

import dataclasses
import functools
import math
import struct
from typing import Any, Callable, NamedTuple

import numpy as np

from . import _abi
from ._lib import IK_MAX_JOINTS
from .robots import RobotSpec, SceneEntityResolver, resolve_matching_names, resolve_matching_names_values

# ---- the constants of include/imx.h under their names without the IMX_ prefix (_abi parses the header; nothing is copied here) ------
def _strip(table: dict, prefix: str) -> dict:
    return {k[len(prefix):]: v for k, v in table.items() if k.startswith(prefix)}


MAGIC, PLAN_VERSION, HEADER_WORDS, MAX_OBS_GROUPS, REC_WORDS = (
    _abi.DEFINES["IMX_" + n] for n in ("MAGIC", "PLAN_VERSION", "HEADER_WORDS", "MAX_OBS_GROUPS", "REC_WORDS"))
H = _strip(_abi.ENUMS["imx_header_word"], "IMX_H_")
R = _strip(_abi.ENUMS["imx_rec_word"], "IMX_R_")
M_OPS = _strip(_abi.ENUMS["imx_mod_op"], "IMX_M_")
T_OPS = _strip(_abi.ENUMS["imx_term_op"], "IMX_T_")
W_OPS = _strip(_abi.ENUMS["imx_rew_op"], "IMX_W_")
O_OPS = _strip(_abi.ENUMS["imx_obs_op"], "IMX_O_")
globals().update(_strip(_abi.ENUMS["imx_act_op"], "IMX_"))  # A_JOINT_AFFINE, A_BINARY_JOINT
globals().update({k: v for k, v in _strip(_abi.DEFINES, "IMX_").items() if k.startswith("F_")})  # F_NOISE_ADD ... F_ACT_TO_LIMITS: every flag

_MDP = "isaaclab.envs.mdp"
_VEL = "isaaclab_tasks.manager_based.locomotion.velocity.mdp"
_CART = "isaaclab_tasks.manager_based.classic.cartpole.mdp"
_SPOT = "isaaclab_tasks.manager_based.locomotion.velocity.config.spot.mdp.rewards"
_CLASSIC = "isaaclab_tasks.manager_based.classic.humanoid.mdp"  # its own modules; what it re-exports from isaaclab.envs.mdp keeps _MDP names
_REACH = "isaaclab_tasks.manager_based.manipulation.reach.mdp.rewards"
_LIFT = "isaaclab_tasks.manager_based.manipulation.lift.mdp"  # .observations, .rewards, .terminations (Isaac-Lift-Cube-Franka-v0)
_POSE_COMMAND = "isaaclab.envs.mdp.commands.pose_command:UniformPoseCommand"  # command = (N, 7): position + quaternion, base frame
_NAV = "isaaclab_tasks.manager_based.navigation.mdp"  # .rewards, .pre_trained_policy_action (Isaac-Navigation-Flat-Anymal-C-v0)
# command = (N, 4): pos_command_b 3 + heading_command_b 1 (pose_2d_command.py: UniformPose2dCommand.command and its terrain-based subclass)
_INHAND = "isaaclab_tasks.manager_based.manipulation.inhand.mdp"  # .observations, .rewards, .terminations (Isaac-Repose-Cube-Allegro-v0)
# command = (N, 7): pos_command_e 3 (the ENV frame) + quat_command_w 4 (orientation_command.py:75-78)
_INHAND_COMMAND = f"{_INHAND}.commands.orientation_command:InHandReOrientationCommand"
_CABINET = "isaaclab_tasks.manager_based.manipulation.cabinet.mdp"  # .observations, .rewards (Isaac-Open-Drawer-Franka-v0)
_POSE_2D_COMMANDS = tuple(f"isaaclab.envs.mdp.commands.pose_2d_command:{c}" for c in ("UniformPose2dCommand", "TerrainBasedPose2dCommand"))


def command_width(command_cfg: dict | None) -> int:
    """Width of a command term's ``command``: 7 for a ``UniformPoseCommand`` (pose_command.py:71-72) and an ``InHandReOrientationCommand``
    (inhand/mdp/commands/orientation_command.py:75-78), 4 for a ``UniformPose2dCommand`` /
    ``TerrainBasedPose2dCommand`` (pose_2d_command.py), 3 for any other (the base velocity command every other task uses)."""
    cls = func_name(command_cfg.get("class_type")) if command_cfg is not None else None
    return 7 if cls in (_POSE_COMMAND, _INHAND_COMMAND) else 4 if cls in _POSE_2D_COMMANDS else 3


def f32(x: float) -> float:
    """Python scalar -> the float32 value torch uses when it meets a float32 tensor."""
    return float(np.float32(x))


def _f2w(x: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def func_name(func: Any) -> str:
    """``module:function`` of a term function given as string or callable (isaaclab/utils/string.py:108-135)."""
    if isinstance(func, str):
        return func
    mod = getattr(func, "__module__", None)
    name = getattr(func, "__qualname__", getattr(func, "__name__", None))
    return f"{mod}:{name}"


def _short(name: str) -> tuple[str, str]:
    mod, _, fn = name.partition(":")
    return mod, fn


def _to_dict(cfg: Any) -> Any:
    if isinstance(cfg, dict):
        return cfg
    if hasattr(cfg, "to_dict"):
        return cfg.to_dict()
    raise TypeError(f"expected a configclass instance or its dict form, got {type(cfg)}")


@dataclasses.dataclass
class Term:
    name: str
    func: str
    op: int
    params: dict
    external: Callable | None = None  # python fallback
    dim: int = 1
    weight: float = 0.0
    time_out: bool = False
    py_modifiers: list = dataclasses.field(default_factory=list)  # (func, params) of a foreign modifier chain applied in Python
    processed_col: int = 0  # action terms: first column and width of the term in the processed action (dim = its raw columns)
    processed_dim: int = 0


_IK_WIDTH = {("position", False): 3, ("position", True): 3, ("pose", True): 6, ("pose", False): 7}  # DifferentialIKController.action_dim


@dataclasses.dataclass
class TaskSpaceTerm:
    """What the task-space action terms share: the controlled frame, its Jacobian block and the term's columns."""

    name: str
    offset_pos: tuple | None  # cfg.body_offset, or None
    offset_rot: tuple | None
    body_name: str
    body_idx: int
    jacobi_body_idx: int
    joint_ids: list  # columns of joint_pos / joint_vel (OSC: also rows and columns of the mass matrix, task_space_actions.py:571-574)
    jacobi_joint_ids: list
    action_col: int  # first raw column
    processed_col: int  # first processed column
    width: int  # action_dim: raw = processed columns
    scale: list  # per column
    clip: list | None  # per column (lo, hi); IK: None without a cfg.clip; OSC: +-inf on the columns the reference does not clamp


def _match_frame(tcfg: dict, robot: RobotSpec, joint_names, body_label: str):
    """The joint and body matching of both ``__init__``: ``(joint_ids, joint names, body_idx, body name)``."""
    joint_ids, jn = resolve_matching_names(tcfg["joint_names"], list(joint_names if joint_names is not None else robot.joint_names))
    body_ids, body_names = resolve_matching_names(tcfg["body_name"], list(robot.body_names))
    if len(body_ids) != 1:
        raise ValueError(f"Expected one match for the {body_label}: {tcfg['body_name']}. Found {len(body_ids)}: {body_names}.")
    return joint_ids, jn, body_ids[0], body_names[0]


def _frame_fields(name: str, robot: RobotSpec, kernel: str, joint_ids, body_idx, body_name) -> dict:
    """The joint-count limit and the Jacobian's row and columns (task_space_actions.py:72-77, 266-274): the index fields of a
    ``TaskSpaceTerm``."""
    n = len(joint_ids)
    if n > IK_MAX_JOINTS:
        raise NotImplementedError(f"action term '{name}': {n} controlled joints; the {kernel} kernel takes at most {IK_MAX_JOINTS}")
    if robot.fixed_base:  # the Jacobian of a fixed base has no row for the root body and no root columns
        jb, jcols = body_idx - 1, list(joint_ids)
        if jb < 0:
            raise ValueError(f"action term '{name}': body '{body_name}' is the root of a fixed-base articulation: it has no Jacobian row")
    else:
        jb, jcols = body_idx, [i + 6 for i in joint_ids]
    return dict(body_name=body_name, body_idx=int(body_idx), jacobi_body_idx=int(jb), joint_ids=[int(i) for i in joint_ids],
                jacobi_joint_ids=[int(i) for i in jcols])


def _body_offset(tcfg: dict) -> dict:
    off = tcfg.get("body_offset")
    return dict(offset_pos=None if off is None else tuple(float(v) for v in off.get("pos", (0.0, 0.0, 0.0))),
                offset_rot=None if off is None else tuple(float(v) for v in off.get("rot", (1.0, 0.0, 0.0, 0.0))))


@dataclasses.dataclass
class IkTerm(TaskSpaceTerm):
    """One ``DifferentialInverseKinematicsAction`` as resolved by its ``__init__`` (task_space_actions.py:53-121): the parameters of
    ``imx_diff_ik_t``.  They travel beside the plan, not in its blob."""

    command_type: str  # "position" | "pose"
    use_relative_mode: bool
    ik_method: str  # "dls" | "trans"
    lambda_val: float
    k_val: float


def resolve_ik_term(name: str, tcfg: dict, robot: RobotSpec, action_col: int = 0, processed_col: int = 0, joint_names=None) -> IkTerm:
    """``DifferentialInverseKinematicsAction.__init__`` (task_space_actions.py:53-121) and the controller cfg's defaults
    (differential_ik_cfg.py:60-70) over a robot's name tables."""
    ctrl = tcfg.get("controller")
    missing = [k for k in ("joint_names", "body_name", "controller") if tcfg.get(k) is None]
    missing += [f"controller.{k}" for k in ("command_type", "ik_method") if isinstance(ctrl, dict) and ctrl.get(k) is None]
    if missing or not isinstance(ctrl, dict):  # (MISSING fields of the configclass: the reference stops at cfg validation)
        raise NotImplementedError(f"action term '{name}': a DifferentialInverseKinematicsAction cfg without {missing or ['a controller dict']} "
                                  "is not on the fused path")
    command_type, method = ctrl["command_type"], ctrl["ik_method"]
    relative = bool(ctrl.get("use_relative_mode", False))
    if command_type not in ("position", "pose"):
        raise ValueError(f"Unsupported inverse-kinematics command: {command_type}.")
    if method not in ("pinv", "svd", "trans", "dls"):
        raise ValueError(f"Unsupported inverse-kinematics method: {method}.")
    if method in ("pinv", "svd"):
        raise NotImplementedError(f"action term '{name}': ik_method '{method}' is not on the fused path (it needs an SVD inside the kernel); "
                                  "'dls' and 'trans' are")
    params = {"trans": {"k_val": 1.0}, "dls": {"lambda_val": 0.01}}[method]
    params.update(ctrl.get("ik_params") or {})
    joint_ids, jn, body_idx, body_name = _match_frame(tcfg, robot, joint_names, "body name")
    frame = _frame_fields(name, robot, "differential-IK", joint_ids, body_idx, body_name)
    width = _IK_WIDTH[(command_type, relative)]
    scale = tcfg.get("scale", 1.0)
    if isinstance(scale, (int, float)):
        scale = [float(scale)] * width
    else:
        scale = [float(v) for v in scale]
        if len(scale) != width:  # torch.tensor(cfg.scale) broadcast into (N, action_dim)
            raise ValueError(f"action term '{name}': scale has {len(scale)} entries for {width} action columns")
    clip = None
    if tcfg.get("clip") is not None:
        if not isinstance(tcfg["clip"], dict):
            raise ValueError(f"Unsupported clip type: {type(tcfg['clip'])}. Supported types are dict.")
        clip = [(-math.inf, math.inf)] * width
        # the reference resolves the keys against the term's JOINT names and indexes the action columns with the result (:117-118)
        i_, _, v_ = resolve_matching_names_values(tcfg["clip"], jn)
        for i, v in zip(i_, v_):
            if i >= width:
                raise IndexError(f"action term '{name}': clip key matches joint {i} of the term, past its {width} action columns")
            clip[i] = (float(v[0]), float(v[1]))
    return IkTerm(name=name, command_type=command_type, use_relative_mode=relative, ik_method=method,
                  lambda_val=float(params.get("lambda_val", 0.01)), k_val=float(params.get("k_val", 1.0)), **frame, **_body_offset(tcfg),
                  action_col=action_col, processed_col=processed_col, width=width, scale=scale, clip=clip)


_OSC_TARGET_WIDTH = {"pose_abs": 7, "pose_rel": 6, "wrench_abs": 6}  # OperationalSpaceController.__init__ (operational_space.py:50-61)


@dataclasses.dataclass
class OscTerm(TaskSpaceTerm):
    """One ``OperationalSpaceControllerAction`` as resolved by its ``__init__`` (task_space_actions.py:248-378) and its controller's
    (operational_space.py:34-140): the parameters of ``imx_osc_t``.  They travel beside the plan, not in its blob."""

    name: str
    target_types: list  # "pose_abs" | "pose_rel", then optionally "wrench_abs" (in cfg order)
    impedance_mode: str  # "fixed" | "variable_kp" | "variable"
    decoupling: str  # "none" | "full" | "partial"
    gravity_compensation: bool
    nullspace_control: str  # "none" | "position"
    nullspace_joint_pos_target: str  # "none" | "zero" | "center" | "default"
    nullspace_stiffness: float
    nullspace_damping_ratio: float
    motion_control_axes: list  # 6
    contact_wrench_control_axes: list  # 6
    motion_stiffness: list  # 6
    motion_damping_ratio: list  # 6
    motion_stiffness_limits: tuple
    motion_damping_ratio_limits: tuple
    pose_idx: int  # first column of each part inside the term (_resolve_command_indexes :504-537); None = absent
    wrench_idx: int | None
    stiffness_idx: int | None
    damping_ratio_idx: int | None

    @property
    def pose_type(self) -> str:
        return "pose_rel" if "pose_rel" in self.target_types else "pose_abs"


def _six(name: str, key: str, v, scalar_ok: bool = True) -> list:
    if isinstance(v, (int, float)) and scalar_ok:
        return [float(v)] * 6
    v = [float(x) for x in v]
    if len(v) != 6:
        raise ValueError(f"action term '{name}': {key} has {len(v)} entries, not 6")
    return v


def resolve_osc_term(name: str, tcfg: dict, robot: RobotSpec, action_col: int = 0, processed_col: int = 0, joint_names=None) -> OscTerm:
    """``OperationalSpaceControllerAction.__init__`` (task_space_actions.py:248-378), ``_resolve_command_indexes`` (:504-537),
    ``_resolve_nullspace_joint_pos_targets`` (:539-566) and ``OperationalSpaceController.__init__`` / ``action_dim``
    (operational_space.py:34-160) with the defaults of operational_space_cfg.py, over a robot's name tables."""
    ctrl = tcfg.get("controller_cfg")
    missing = [k for k in ("joint_names", "body_name", "controller_cfg") if tcfg.get(k) is None]
    missing += [f"controller_cfg.{k}" for k in ("target_types",) if isinstance(ctrl, dict) and ctrl.get(k) is None]
    if missing or not isinstance(ctrl, dict):  # (MISSING fields of the configclass: the reference stops at cfg validation)
        raise NotImplementedError(f"action term '{name}': an OperationalSpaceControllerAction cfg without {missing or ['a controller_cfg dict']} "
                                  "is not on the fused path")
    targets = list(ctrl["target_types"])
    for t in targets:
        if t not in _OSC_TARGET_WIDTH:
            raise ValueError(f"Invalid control command: {t}.")
    mode = ctrl.get("impedance_mode", "fixed")
    if mode not in ("fixed", "variable_kp", "variable"):
        raise ValueError(f"Invalid impedance mode: {mode}.")
    null_ctrl, null_target = ctrl.get("nullspace_control", "none"), tcfg.get("nullspace_joint_pos_target", "none")
    if null_target != "none" and null_ctrl != "position":
        raise ValueError("Nullspace joint targets can only be set when null space control is set to 'position'.")
    if null_target == "none" and null_ctrl == "position":
        raise ValueError("Nullspace joint targets must be set when null space control is set to 'position'.")
    if null_target not in ("none", "zero", "center", "default"):
        raise ValueError("Invalid value for nullspace joint pos targets.")
    if null_ctrl not in ("none", "position"):
        raise ValueError(f"Invalid null-space control method: {null_ctrl}.")
    joint_ids, _, body_idx, body_name = _match_frame(tcfg, robot, joint_names, "ee body name")
    n = len(joint_ids)
    if null_ctrl != "none" and n <= 6:  # (operational_space.py:491-493, raised by the first compute())
        raise ValueError("Null-space control is only applicable for redundant manipulators.")
    # ---- what the fused path does not build
    if tcfg.get("task_frame_rel_path") is not None:
        raise NotImplementedError(f"action term '{name}': task_frame_rel_path '{tcfg['task_frame_rel_path']}' needs a FrameTransformer on a "
                                  "rigid body of the scene; only the identity task frame (the root frame) is on the fused path")
    if "wrench_abs" in targets and ctrl.get("contact_wrench_stiffness_task") is not None:
        raise NotImplementedError(f"action term '{name}': closed-loop wrench control (contact_wrench_stiffness_task set) needs a contact sensor "
                                  "on the end effector; only the open-loop wrench is on the fused path")
    if sum(t.startswith("pose") for t in targets) > 1 or targets.count("wrench_abs") > 1:
        raise NotImplementedError(f"action term '{name}': target_types {targets} holds two motion targets or two wrench targets; the fused "
                                  "path takes one of each")
    if not any(t.startswith("pose") for t in targets):
        raise NotImplementedError(f"action term '{name}': target_types {targets} holds no motion target; the fused path takes 'pose_abs' or "
                                  "'pose_rel', alone or with 'wrench_abs'")
    decoupled, partial = bool(ctrl.get("inertial_dynamics_decoupling", False)), bool(ctrl.get("partial_inertial_dynamics_decoupling", False))
    decoupling = "none" if not decoupled else ("partial" if partial else "full")
    if null_ctrl == "position" and decoupling != "full":
        raise NotImplementedError(f"action term '{name}': nullspace_control 'position' without full inertial decoupling takes torch.pinverse of "
                                  "the Jacobian, an SVD inside the kernel (as ik_method 'pinv'); it is on the fused path with "
                                  "inertial_dynamics_decoupling=True, partial_inertial_dynamics_decoupling=False only")
    frame = _frame_fields(name, robot, "operational-space", joint_ids, body_idx, body_name)
    # ---- _resolve_command_indexes and _preprocess_actions: per-column scale and clamp
    idx = {"pose": None, "wrench_abs": None, "stiffness": None, "damping_ratio": None}
    scale, clip, col = [], [], 0
    inf = (-math.inf, math.inf)
    ps, os_, ws = float(tcfg.get("position_scale", 1.0)), float(tcfg.get("orientation_scale", 1.0)), float(tcfg.get("wrench_scale", 1.0))
    for t in targets:
        w = _OSC_TARGET_WIDTH[t]
        idx["pose" if t.startswith("pose") else t] = col
        scale += [ws] * 6 if t == "wrench_abs" else [ps] * 3 + [os_] * (w - 3)
        clip += [inf] * w
        col += w
    k_lim = tuple(float(v) for v in ctrl.get("motion_stiffness_limits_task", (0, 1000)))
    d_lim = tuple(float(v) for v in ctrl.get("motion_damping_ratio_limits_task", (0, 100)))
    if mode in ("variable_kp", "variable"):
        idx["stiffness"] = col
        scale += [float(tcfg.get("stiffness_scale", 1.0))] * 6
        clip += [k_lim] * 6
        col += 6
        if mode == "variable":
            idx["damping_ratio"] = col
            scale += [float(tcfg.get("damping_ratio_scale", 1.0))] * 6
            clip += [d_lim] * 6
            col += 6
    return OscTerm(name=name, target_types=targets, impedance_mode=mode, decoupling=decoupling,
                   gravity_compensation=bool(ctrl.get("gravity_compensation", False)), nullspace_control=null_ctrl,
                   nullspace_joint_pos_target=null_target, nullspace_stiffness=float(ctrl.get("nullspace_stiffness", 10.0)),
                   nullspace_damping_ratio=float(ctrl.get("nullspace_damping_ratio", 1.0)),
                   motion_control_axes=_six(name, "motion_control_axes_task", ctrl.get("motion_control_axes_task", (1,) * 6), False),
                   contact_wrench_control_axes=_six(name, "contact_wrench_control_axes_task", ctrl.get("contact_wrench_control_axes_task", (0,) * 6), False),
                   motion_stiffness=_six(name, "motion_stiffness_task", ctrl.get("motion_stiffness_task", 100.0)),
                   motion_damping_ratio=_six(name, "motion_damping_ratio_task", ctrl.get("motion_damping_ratio_task", 1.0)),
                   motion_stiffness_limits=k_lim, motion_damping_ratio_limits=d_lim, **frame, **_body_offset(tcfg),
                   action_col=action_col, processed_col=processed_col, width=col,
                   pose_idx=idx["pose"], wrench_idx=idx["wrench_abs"], stiffness_idx=idx["stiffness"], damping_ratio_idx=idx["damping_ratio"],
                   scale=scale, clip=clip)


@dataclasses.dataclass
class PolicyTerm:
    """One ``PreTrainedPolicyAction`` (isaaclab_tasks .../navigation/mdp/pre_trained_policy_action.py:24-100): its low-level observation
    group and its low-level action term compiled as a plan of their own (``imx_pretrained_policy`` and the unfused chain run on it), the
    launch period and where the policy comes from.  It travels beside the plan, not in its blob."""

    name: str
    action_col: int  # first raw (= processed) column; the term's raw action is its processed action (process_actions copies)
    width: int  # action_dim: 3
    low_level_decimation: int
    policy_path: Any  # cfg.policy_path (a local file), or None: the env is given low_level_policy=
    low_level_plan: "Plan"  # D = the policy's inputs, A = its outputs; generated_commands reads the raw action, last_action low_level_actions
    low_level_action_name: str


@dataclasses.dataclass
class Plan:
    blob: np.ndarray  # int32 words
    robot: RobotSpec
    num_joints: int
    num_bodies: int
    history: int
    action_dim: int
    obs_dim: int
    num_rays: int
    cmd_dim: int
    step_dt: float
    max_episode_length: int
    max_episode_length_s: float
    is_finite_horizon: bool
    reward_terms: list[Term]  # ALL reward terms incl. zero weight (active_terms order)
    termination_terms: list[Term]
    obs_terms: list[Term]
    obs_term_dims: list[tuple[int, ...]]
    action_terms: list[Term]
    enable_corruption: bool
    ray_starts_local: np.ndarray | None
    ray_direction: tuple[float, float, float]
    ray_max_distance: float
    scanner_cfg: dict | None
    n_ext_rew: int = 0
    n_ext_term: int = 0
    n_ext_obs: int = 0
    mod_state_dim: int = 0  # floats of observation-modifier state per env (DigitalFilter / Integrator)
    gravity_dir: tuple[float, float, float] = (0.0, 0.0, -1.0)
    obs_groups: list = dataclasses.field(default_factory=list)  # every observation group (ObsGroup), cfg order; [0] = obs_terms/obs_dim
    obs_dim_total: int = 0  # sum of the group widths (= width of the parity-mode noise feed)
    scan_stateful: bool = False  # the height scanner keeps per-env timestamps / drift (update_period > 0 or a drift range)
    scan_drift_range: tuple[float, float] = (0.0, 0.0)
    term_slots: int = 0  # rows of per-env reward-term state (imx_buffers.term_state): one per progress_reward term
    processed_action_dim: int = 0  # width of the processed action (= action_dim unless a term writes more joints than it takes columns)
    ik_terms: list = dataclasses.field(default_factory=list)  # IkTerm of the env's DifferentialInverseKinematicsAction (at most one)
    osc_terms: list = dataclasses.field(default_factory=list)  # OscTerm of the env's OperationalSpaceControllerAction (at most one, and no IkTerm beside it)
    policy_terms: list = dataclasses.field(default_factory=list)  # PolicyTerm of the env's PreTrainedPolicyAction (at most one, no IK / OSC term beside it)
    # which of the rigid object's further state tensors and of the in-hand command's metrics the terms read (state_feed.OBJECT_STATE
    # names, sorted): the env asks the feed for them (StateFeed.ensure_object_state); a plan that reads none allocates none
    state_reads: tuple = ()
    # ... and which tensors of the scene's second articulation (state_feed.ARTICULATION_STATE names: "articulation_joint_pos", ...): the
    # env asks the feed for those with StateFeed.ensure_articulation_state.  frame_tables: the FrameTransformer sensors the fused terms
    # read, resolved (robots.FrameTable by entity name; None for a sensor the scene lacks), as written to the blob at frame_table_off
    frame_tables: dict = dataclasses.field(default_factory=dict)
    frame_table_off: int = 0
    imu_sensors: tuple = ()  # the scene's Imu sensors the imu_* observation terms read; a term's sensor index (AUX0) indexes this


@dataclasses.dataclass
class ObsGroup:
    name: str
    enable_corruption: bool = False
    first_record: int = 0
    num_records: int = 0
    dim: int = 0
    terms: list = dataclasses.field(default_factory=list)
    term_dims: list = dataclasses.field(default_factory=list)    # the reference's group_obs_term_dim: (d,), (H*d,) or (H, d) per term
    term_widths: list = dataclasses.field(default_factory=list)  # columns of each term in the fused row (history windows flattened, oldest first)
    concatenate: bool = True                                     # ObservationGroupCfg.concatenate_terms

    @property
    def is_flat(self) -> bool:
        """The group IS its fused row: concatenated, every term one-dimensional."""
        return self.concatenate and all(len(d) == 1 for d in self.term_dims)


class _Blob:
    def __init__(self):
        self.w: list[int] = [0] * HEADER_WORDS

    def ints(self, xs) -> int:
        off = len(self.w)
        self.w.extend(int(x) for x in xs)
        return off

    def floats(self, xs) -> int:
        off = len(self.w)
        self.w.extend(_f2w(x) for x in xs)
        return off

    def table(self, recs: list[list[int]]) -> int:
        off = len(self.w)
        for r in recs:
            assert len(r) == REC_WORDS
            self.w.extend(r)
        return off


def compile_modifiers(mods) -> tuple[list[int], int]:
    """``ObservationTermCfg.modifiers`` (isaaclab/utils/modifiers/modifier_cfg.py; applied at observation_manager.py:310-312)
    -> (program words, state slots per element) in the format of include/imx.h ``IMX_F_MODIFIERS``.  Raises
    NotImplementedError for a modifier that is not one of modifier.py's five."""
    prog: list[int] = []
    slots = 0
    for m in mods:
        m = m if isinstance(m, dict) else m.to_dict()
        mod, fn = _short(func_name(m["func"]))
        if not mod.startswith("isaaclab.utils.modifiers"):
            raise NotImplementedError(f"modifier {mod}:{fn}")
        p = m.get("params") or {}
        if fn == "scale":
            prog += [M_OPS["SCALE"], _f2w(f32(p["multiplier"])), 0, 0]
        elif fn == "bias":
            prog += [M_OPS["BIAS"], _f2w(f32(p["value"])), 0, 0]
        elif fn == "clip":
            lo, hi = p["bounds"]
            prog += [M_OPS["CLIP"], _f2w(-math.inf if lo is None else f32(lo)), _f2w(math.inf if hi is None else f32(hi)), 0]
        elif fn == "Integrator":
            prog += [M_OPS["INTEGRATOR"], _f2w(f32(m["dt"])), 0, slots]
            slots += 2
        elif fn == "DigitalFilter":
            A_, B_ = m.get("A"), m.get("B")
            if A_ is None or B_ is None:  # modifier.py:131-132
                raise ValueError("Digital filter coefficients A and B must not be None. Please provide valid coefficients.")
            prog += [M_OPS["DIGITAL_FILTER"], len(A_), len(B_), slots] + [_f2w(f32(x)) for x in list(A_) + list(B_)]
            slots += len(A_) + len(B_)
        else:
            raise NotImplementedError(f"modifier {mod}:{fn}")
    return prog, slots


def _rec(**kw) -> list[int]:
    r = [0] * REC_WORDS
    for k, v in kw.items():
        key = k.upper()
        r[R[key]] = _f2w(v) if isinstance(v, float) else int(v)
    return r


def grid_pattern(resolution: float, size, direction=(0.0, 0.0, -1.0), ordering: str = "xy"):
    """``grid_pattern`` (isaaclab/sensors/ray_caster/patterns/patterns.py:16-58).  ``torch.arange`` on float32
    evaluates ``start + i*step`` in double and rounds to float32; ``meshgrid`` 'xy' puts x fastest."""
    if ordering not in ("xy", "yx"):
        raise ValueError(f"Ordering must be 'xy' or 'yx'. Received: '{ordering}'.")
    if resolution <= 0:
        raise ValueError(f"Resolution must be greater than 0. Received: '{resolution}'.")

    def arange(start, end, step):
        n = int(math.ceil((end - start) / step))
        return (start + step * np.arange(n, dtype=np.float64)).astype(np.float32)

    x = arange(-size[0] / 2, size[0] / 2 + 1.0e-9, resolution)
    y = arange(-size[1] / 2, size[1] / 2 + 1.0e-9, resolution)
    if ordering == "xy":  # torch.meshgrid(indexing="xy"): output shape (len(y), len(x))
        gx, gy = np.meshgrid(x, y, indexing="xy")
    else:  # "ij"
        gx, gy = np.meshgrid(x, y, indexing="ij")
    starts = np.zeros((gx.size, 3), np.float32)
    starts[:, 0] = gx.reshape(-1)
    starts[:, 1] = gy.reshape(-1)
    dirs = np.tile(np.asarray(direction, np.float32), (gx.size, 1))
    return starts, dirs


def _pattern_field(cfg, name, default=None):
    v = cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)
    if v is None or (isinstance(v, str) and v == "MISSING") or type(v).__name__ == "_MISSING_TYPE":
        raise ValueError(f"ray pattern cfg: '{name}' is missing")
    return v


_BPEARL_VERTICAL_RAY_ANGLES = (  # BpearlPatternCfg.vertical_ray_angles (patterns_cfg.py:188-192): the sensor's 32 unevenly spaced rings
    89.5, 86.6875, 83.875, 81.0625, 78.25, 75.4375, 72.625, 69.8125, 67.0, 64.1875, 61.375, 58.5625, 55.75, 52.9375, 50.125, 47.3125, 44.5,
    41.6875, 38.875, 36.0625, 33.25, 30.4375, 27.625, 24.8125, 22, 19.1875, 16.375, 13.5625, 10.75, 7.9375, 5.125, 2.3125)


def bpearl_pattern(cfg):
    """``bpearl_pattern`` (isaaclab/sensors/ray_caster/patterns/patterns.py:106-133) of a ``BpearlPatternCfg`` or its dict form, the same
    torch ops in the same order on the CPU: (starts, directions), (R, 3) float32 arrays; the vertical angle runs fastest."""
    import torch

    fov, res = _pattern_field(cfg, "horizontal_fov", 360.0), _pattern_field(cfg, "horizontal_res", 10.0)
    h = torch.arange(-fov / 2, fov / 2, res)
    v = torch.tensor(list(_pattern_field(cfg, "vertical_ray_angles", _BPEARL_VERTICAL_RAY_ANGLES)))
    pitch, yaw = torch.meshgrid(v, h, indexing="xy")
    pitch, yaw = torch.deg2rad(pitch.reshape(-1)), torch.deg2rad(yaw.reshape(-1))
    pitch += torch.pi / 2
    x = torch.sin(pitch) * torch.cos(yaw)
    y = torch.sin(pitch) * torch.sin(yaw)
    z = torch.cos(pitch)
    dirs = -torch.stack([x, y, z], dim=1)
    return torch.zeros_like(dirs).numpy(), dirs.numpy()


def lidar_pattern(cfg):
    """``lidar_pattern`` (patterns.py:136-179) of a ``LidarPatternCfg`` or its dict form: a full 360 degree range drops its last azimuth,
    the azimuth count is ``math.ceil(span / horizontal_res)``; the azimuth runs fastest."""
    import torch

    vr, hr = _pattern_field(cfg, "vertical_fov_range"), _pattern_field(cfg, "horizontal_fov_range")
    vertical_angles = torch.linspace(vr[0], vr[1], int(_pattern_field(cfg, "channels")))
    up_to = -1 if abs(abs(hr[0] - hr[1]) - 360.0) < 1e-6 else None
    n = math.ceil((hr[1] - hr[0]) / _pattern_field(cfg, "horizontal_res"))
    horizontal_angles = torch.linspace(hr[0], hr[1], n)[:up_to]
    v_angles, h_angles = torch.meshgrid(torch.deg2rad(vertical_angles), torch.deg2rad(horizontal_angles), indexing="ij")
    x = torch.cos(v_angles) * torch.cos(h_angles)
    y = torch.cos(v_angles) * torch.sin(h_angles)
    z = torch.sin(v_angles)
    dirs = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
    return torch.zeros_like(dirs).numpy(), dirs.numpy()


def ray_pattern(pattern_cfg):
    """(starts, directions) of a ray-caster ``pattern_cfg`` (object or ``to_dict()`` form, ``func`` a callable or its
    ``module:function`` name): ``grid_pattern``, ``bpearl_pattern`` or ``lidar_pattern``.  ``pinhole_camera_pattern`` is refused by name."""
    func = pattern_cfg.get("func") if isinstance(pattern_cfg, dict) else getattr(pattern_cfg, "func", None)
    if func is None:
        raise ValueError("ray pattern cfg: 'func' is missing")
    name = _short(func_name(func))[1].rsplit(".", 1)[-1]
    if name == "pinhole_camera_pattern":
        raise NotImplementedError("pinhole_camera_pattern belongs to the camera sensors (RayCasterCamera), which are out of scope: "
                                  "the RayCaster takes grid_pattern, bpearl_pattern and lidar_pattern")
    if name == "bpearl_pattern":
        return bpearl_pattern(pattern_cfg)
    if name == "lidar_pattern":
        return lidar_pattern(pattern_cfg)
    if name == "grid_pattern":
        return grid_pattern(_pattern_field(pattern_cfg, "resolution"), _pattern_field(pattern_cfg, "size"),
                            tuple(_pattern_field(pattern_cfg, "direction", (0.0, 0.0, -1.0))), _pattern_field(pattern_cfg, "ordering", "xy"))
    raise NotImplementedError(f"ray pattern '{name}' is not known (grid_pattern, bpearl_pattern, lidar_pattern)")


def _quat_apply_np(q, v):
    w, xyz = np.float32(q[0]), np.asarray(q[1:], np.float32)
    t = np.cross(xyz, v).astype(np.float32) * np.float32(2)
    return (v + w * t + np.cross(xyz, t)).astype(np.float32)


# ---- the fused term functions: one table per manager, keyed on the qualified function name.  Porting a term function is one entry,
#      plus a hook where its record is not just id lists and float params ------------------------------------------------------------
class _Ids(NamedTuple):
    """Where an id list comes from: the ``SceneEntityCfg`` under ``params[key]`` (``required``: a ``KeyError`` without it), resolved to
    joint or body ids; without a cfg, every joint / body of ``entity`` (the term function's default argument)."""
    key: str
    kind: str
    entity: str = "robot"
    required: bool = False


_JOINTS, _BODIES, _CONTACTS = _Ids("asset_cfg", "joint"), _Ids("asset_cfg", "body"), _Ids("sensor_cfg", "body", "contact_forces")


@dataclasses.dataclass(frozen=True)
class _Fused:
    """How one term function's cfg becomes its op record: ``PlanCompiler._fuse`` fills the id lists, calls the hook, then reads the params."""
    op: str                        # name in T_OPS / W_OPS / O_OPS
    ids: _Ids | None = None        # first id list
    ids2: _Ids | None = None       # second id list
    params: tuple = ()             # -> P0, P1, P2 through f32: "name" (required) or ("name", default)
    width: int = 0                 # observations: columns of the term; 0 = one per id, or set by the hook (rec["dim"])
    hook: Callable | None = None   # the irregular rest: hook(c, name, p, rec), c the PlanCompiler
    applies: Callable | None = None  # applies(p) false: the entry is not for these params (the term is Python-evaluated)
    articulation: bool = False     # an id list may name the scene's second articulation (the hook then says how the record tells)


# Closed modules -- Spot's rewards, the classic tasks' observations and rewards, the reach rewards -- have no Python fallback: a function
# of theirs without a table entry is refused in the managers named here.  Any other unknown function is Python-evaluated (``EXTERNAL``).
_CLOSED = {_SPOT: ("reward",), _REACH: ("reward",), **{f"{_CLASSIC}.{m}": ("termination", "reward", "observation") for m in ("observations", "rewards")},
           **{f"{_LIFT}.{m}": ("termination", "reward", "observation") for m in ("observations", "rewards", "terminations")},
           f"{_NAV}.rewards": ("reward",),
           **{f"{_INHAND}.{m}": ("termination", "reward", "observation") for m in ("observations", "rewards", "terminations")},
           **{f"{_CABINET}.{m}": ("termination", "reward", "observation") for m in ("observations", "rewards")}}


def _target_pos(kind: str, name: str, p: dict) -> list[float]:
    t = p["target_pos"]
    if len(t) != 3:
        raise ValueError(f"{kind} term '{name}': target_pos must have 3 components, got {t}")
    return [f32(t[0]), f32(t[1]), f32(t[2])]


def _all_joints(c, name, p, rec):
    """The record lists ALL joints whatever ``asset_cfg`` names: the function never indexes with ``asset_cfg.joint_ids``."""
    c.entities.ids(p.get("asset_cfg"), "joint")  # the cfg must still resolve (SceneEntityCfg.resolve) though it selects nothing
    rec.update(ids_off=c.blob.ints(range(c.robot.num_joints)), nids=c.robot.num_joints)


# -- terminations (isaaclab/envs/mdp/terminations.py, .../locomotion/velocity/mdp/terminations.py)
def _manual_limit_bounds(c, name, p, rec):
    rec.update(p0=f32(p["bounds"][0]), p1=f32(p["bounds"][1]))


def _command_resample(c, name, p, rec):
    # time_left (f32) <= step_dt and command_counter == num_resamples (terminations.py:35-42)
    rec.update(p0=f32(c.step_dt), nids=int(p.get("num_resamples", 1)))


def _terrain_out_of_bounds(c, name, p, rec):
    terr = c.scene.get("terrain") or {}
    if terr.get("terrain_type") == "plane" or not terr.get("terrain_generator"):
        rec.update(p0=math.inf, p1=math.inf)
    else:
        tg = terr["terrain_generator"]
        buf = float(p.get("distance_buffer", 3.0))
        mw = tg["num_rows"] * tg["size"][0] + 2 * tg["border_width"]
        mh = tg["num_cols"] * tg["size"][1] + 2 * tg["border_width"]
        rec.update(p0=f32(0.5 * mw - buf), p1=f32(0.5 * mh - buf))


# -- the lift task's own terms (isaaclab_tasks .../manipulation/lift/mdp: Isaac-Lift-Cube-Franka-v0) and what they share
def _entity_name(ent, default: str) -> str:
    if ent is None:
        return default
    return ent.get("name") if isinstance(ent, dict) else getattr(ent, "name", None)


def _object(c, kind, name, p, key="object_cfg", default="object"):
    """The ``RigidObject`` a term reads (``object.data.root_pos_w``): the scene's one rigid object, served as ``object_root_pos_w``."""
    ent = _entity_name(p.get(key), default)
    if ent not in c.entities.rigid_objects:
        raise ValueError(f"{kind} term '{name}': '{key}' names the scene entity '{ent}', which is not a RigidObject of the scene "
                         f"(it has {list(c.entities.rigid_objects)})")
    if len(c.entities.rigid_objects) > 1:
        raise NotImplementedError(f"{kind} term '{name}': the scene has {len(c.entities.rigid_objects)} rigid objects "
                                  f"{list(c.entities.rigid_objects)}; the fused path carries one object root position")
    c.entities.ids(p.get(key), "body", ent)  # the cfg must still resolve (SceneEntityCfg.resolve)


def _robot(c, kind, name, p, key="robot_cfg"):
    ent = _entity_name(p.get(key), "robot")
    if ent != "robot":
        raise NotImplementedError(f"{kind} term '{name}': '{key}' names the scene entity '{ent}'; the fused op reads the robot's root state")


def _pose_command(c, kind, name, p, default=None):
    """``command_name`` must name a command term of the cfg whose command is (N, 7) (``command[:, :3]`` = the goal in the base frame)."""
    cname = p.get("command_name", default)
    ccfg = (c.cfg.get("commands") or {}).get(cname)
    if ccfg is None:
        raise ValueError(f"{kind} term '{name}': command_name '{cname}' is not a command term of the cfg (it has {list(c.cfg.get('commands') or {})})")
    if command_width(ccfg) != 7 or c.cmd_dim != 7:
        raise ValueError(f"{kind} term '{name}': command '{cname}' must be a UniformPoseCommand (N, 7); it is {command_width(ccfg)} wide")


def _root_height_asset(c, name, p, rec):
    """``asset_cfg`` selects whose root: the robot (AUX0 = 0, the word every older blob has) or the scene's rigid object (AUX0 = 1)."""
    ent = _entity_name(p.get("asset_cfg"), "robot")
    if ent in c.entities.rigid_objects:
        _object(c, "termination", name, p, key="asset_cfg")
        rec["aux0"] = 1
    elif ent != "robot":
        c.entities.names(ent, "body")  # raises: the entity does not exist


def _object_reached_goal(c, name, p, rec):
    _robot(c, "termination", name, p)
    _object(c, "termination", name, p)
    _pose_command(c, "termination", name, p, default="object_pose")


def _object_is_lifted(c, name, p, rec):
    _object(c, "reward", name, p)


def _object_goal_distance(c, name, p, rec):
    _robot(c, "reward", name, p)
    _object(c, "reward", name, p)
    _pose_command(c, "reward", name, p)


def _object_ee_distance(c, name, p, rec):
    """``ee_frame.data.target_pos_w[:, 0]``: the record carries the robot body of the frame's first target and its offset position."""
    _object(c, "reward", name, p)
    body, pos, rot = c.entities.frame(_entity_name(p.get("ee_frame_cfg"), "ee_frame"))
    if tuple(rot) != (1.0, 0.0, 0.0, 0.0):
        raise NotImplementedError(f"reward term '{name}': the target frame's offset rotation {rot} is not the identity; the fused op "
                                  "adds the rotated offset position only")
    if body not in c.entities.body_names:
        raise ValueError(f"reward term '{name}': the target frame sits on '{body}', which is not a body of the robot ({c.entities.body_names})")
    rec.update(ids_off=c.blob.ints([c.entities.body_names.index(body)]), nids=1, p1=f32(pos[0]), p2=f32(pos[1]), p3=f32(pos[2]))


def _object_position(c, name, p, rec):
    _robot(c, "observation", name, p)
    _object(c, "observation", name, p)


# -- the in-hand task's own terms (isaaclab_tasks .../manipulation/inhand/mdp: Isaac-Repose-Cube-Allegro-v0)
def _inhand_command(c, kind, name, p, threshold=False) -> dict:
    """``command_name`` must name a command term of the cfg whose command is (N, 7); with ``threshold`` its cfg must carry
    ``orientation_success_threshold`` (an ``InHandReOrientationCommandCfg``: the term reads that field or the term's
    ``consecutive_success`` metric, which a ``UniformPoseCommand`` does not have).  Returns the command cfg."""
    cname = p.get("command_name")
    ccfg = (c.cfg.get("commands") or {}).get(cname)
    if ccfg is None:
        raise ValueError(f"{kind} term '{name}': command_name '{cname}' is not a command term of the cfg (it has {list(c.cfg.get('commands') or {})})")
    if command_width(ccfg) != 7 or c.cmd_dim != 7:
        raise ValueError(f"{kind} term '{name}': command '{cname}' must be an InHandReOrientationCommand (N, 7); it is {command_width(ccfg)} wide")
    if threshold and not isinstance(ccfg.get("orientation_success_threshold"), (int, float)):
        raise NotImplementedError(f"{kind} term '{name}': command '{cname}' ({func_name(ccfg.get('class_type'))}) has no "
                                  "orientation_success_threshold: the term reads the success threshold / the consecutive_success metric of an "
                                  "InHandReOrientationCommand, which a UniformPoseCommand does not have")
    return ccfg


def _reads(c, *names):
    c.state_reads.update(names)


def _max_consecutive_success(c, name, p, rec):
    _inhand_command(c, "termination", name, p, threshold=True)
    _reads(c, "command_consecutive_success")
    rec["p0"] = f32(p["num_success"])  # (the metric is a float tensor: `>= num_success` compares in fp32)


def _object_away_from_goal(c, name, p, rec):
    _inhand_command(c, "termination", name, p)
    _object(c, "termination", name, p)


def _object_away_from_robot(c, name, p, rec):
    _robot(c, "termination", name, p, key="asset_cfg")
    _object(c, "termination", name, p)


def _track_orientation(c, name, p, rec):
    _inhand_command(c, "reward", name, p)
    _object(c, "reward", name, p)
    _reads(c, "object_root_quat_w")


def _success_bonus(c, name, p, rec):
    ccfg = _inhand_command(c, "reward", name, p, threshold=True)
    _object(c, "reward", name, p)
    _reads(c, "object_root_quat_w")
    rec["p0"] = f32(ccfg["orientation_success_threshold"])


def _track_pos(c, name, p, rec):
    _inhand_command(c, "reward", name, p)
    _object(c, "reward", name, p)


def _goal_quat_diff(c, name, p, rec):
    _inhand_command(c, "observation", name, p)
    if p.get("asset_cfg") is None:
        raise KeyError(f"observation term '{name}': goal_quat_diff needs 'asset_cfg'")
    _object(c, "observation", name, p, key="asset_cfg")
    _reads(c, "object_root_quat_w")
    _quat_unique(c, name, p, rec)


# -- the Open-Drawer task's own terms (isaaclab_tasks .../manipulation/cabinet/mdp: Isaac-Open-Drawer-Franka-v0).  They read two
#    FrameTransformer sensors by name -- env.scene["ee_frame"]: target 0 = the tool centre point, targets 1, 2 = the left / right
#    fingertip; env.scene["cabinet_frame"]: target 0 = the drawer handle -- and the scene's second articulation (the cabinet)
_EE_FRAME, _CABINET_FRAME = "ee_frame", "cabinet_frame"
_NO_FRAME = [0, 0, _f2w(0.0), _f2w(0.0), _f2w(0.0), _f2w(1.0), _f2w(0.0), _f2w(0.0), _f2w(0.0)]  # the source slot of a sensor the scene does not have


def _frame_table(c, kind, name, sensors=()) -> int:
    """The plan's frame table (include/imx.h ``IMX_FT_*``), written into the blob by the first term that needs it: the row widths J2, B2
    of the second articulation's tensors, the target counts of the two sensors, then source and targets of each as nine words.  Returns
    its offset.  ``sensors``: the sensors this term reads -- they must exist in the scene."""
    if c.ft_off is None:
        tabs = {s: c.entities.frame_table(s) if s in c.entities.frames else None for s in (_EE_FRAME, _CABINET_FRAME)}
        second = c.entities.second
        w = [second.num_joints if second else 0, second.num_bodies if second else 0] + [len(t.targets) if t else 0 for t in tabs.values()]
        for t in tabs.values():
            for f in ([t.source] + list(t.targets)) if t else [None]:
                w += _NO_FRAME if f is None else [f.body_id, f.asset] + [_f2w(f32(x)) for x in (*f.pos, *f.rot)]
        c.ft_off, c.frame_tables = c.blob.ints(w), tabs
    for s in sensors:
        if c.frame_tables[s] is None:
            raise ValueError(f"{kind} term '{name}': the scene entity '{s}' is not a FrameTransformer of the scene (it has {list(c.entities.frames)})")
    return c.ft_off


def _reads_frames(c, *frames):
    """The body poses a frame reads: the robot's arrive with every state struct; the second articulation's are asked for by name."""
    if any(f.asset == 1 for f in frames):
        _reads(c, "articulation_body_pos_w", "articulation_body_quat_w")


def _cabinet_reward(fingers, c, name, p, rec):
    rec["aux0"] = _frame_table(c, "reward", name, (_EE_FRAME, _CABINET_FRAME))
    ee, cab = c.frame_tables[_EE_FRAME], c.frame_tables[_CABINET_FRAME]
    if fingers and len(ee.targets) < 3:
        raise ValueError(f"reward term '{name}': the function reads the fingertip frames, targets 1 and 2 of '{_EE_FRAME}'; the sensor has "
                         f"{len(ee.targets)} target frame(s) {ee.target_frame_names}")
    _reads_frames(c, ee.targets[0], cab.targets[0], *(ee.targets[1:3] if fingers else ()))


def _drawer_joint(c, name, p, rec):
    """``asset_cfg.joint_ids[0]`` of ``env.scene[asset_cfg.name]``: the robot (AUX1 = 0) or the second articulation (AUX1 = 1)."""
    _cabinet_reward(True, c, name, p, rec)
    if rec["nids"] < 1:
        raise ValueError(f"reward term '{name}': asset_cfg selects no joint")
    if _entity_name(p.get("asset_cfg"), "robot") in c.entities.articulations:
        rec["aux1"] = 1
        _reads(c, "articulation_joint_pos")


def _cabinet_obs(fn, c, name, p, rec):
    sensors = (_EE_FRAME, _CABINET_FRAME) if fn == "rel_ee_drawer_distance" else (_EE_FRAME,)
    rec["aux0"] = _frame_table(c, "observation", name, sensors)
    ee = c.frame_tables[_EE_FRAME]
    if fn == "rel_ee_drawer_distance":
        _reads_frames(c, ee.targets[0], c.frame_tables[_CABINET_FRAME].targets[0])
    elif fn == "fingertips_pos":  # (N, targets - 1, 3) flattened
        if len(ee.targets) < 2:
            raise ValueError(f"observation term '{name}': fingertips_pos reads the target frames after the first; '{_EE_FRAME}' has {len(ee.targets)}")
        rec["dim"] = 3 * (len(ee.targets) - 1)
        _reads_frames(c, *ee.targets[1:])
    else:
        _reads_frames(c, ee.targets[0])
        if fn == "ee_quat" and p.get("make_quat_unique", True):  # (the function's default is True, observations.py:51)
            rec["flags"] |= F_QUAT_UNIQUE


def _joint_rel_asset(fn, c, name, p, rec):
    """``joint_pos_rel`` / ``joint_vel_rel`` with an ``asset_cfg`` that names the second articulation: the op that reads its tensors, the
    defaults of the selected joints beside the record (P2 = their offset).  On the robot the record stays word for word what it was."""
    ent = _entity_name(p.get("asset_cfg"), "robot")
    if ent not in c.entities.articulations:
        return
    art = c.entities.articulations[ent]
    ids = c.entities.ids(p.get("asset_cfg"), "joint")
    defaults = art.default_joint_pos if fn == "joint_pos_rel" else art.default_joint_vel
    rec.update(op=O_OPS["ARTICULATION_" + fn.upper()], p2=int(c.blob.floats([f32(defaults[i]) for i in ids])),
               aux0=_frame_table(c, "observation", name))
    _reads(c, "articulation_joint_pos" if fn == "joint_pos_rel" else "articulation_joint_vel")


_ROOT_OBJECT_READS = {"ROOT_QUAT_W": "object_root_quat_w", "ROOT_LIN_VEL_W": "object_root_lin_vel_w", "ROOT_ANG_VEL_W": "object_root_ang_vel_w"}


def _root_asset(op, c, name, p, rec):
    """``asset_cfg`` of the four root observations selects whose root: the robot (AUX0 = 0, the word every older blob has) or the scene's
    rigid object (AUX0 = 1), as for ``root_height_below_minimum``.  Anything else is refused."""
    ent = _entity_name(p.get("asset_cfg"), "robot")
    if ent in c.entities.rigid_objects:
        _object(c, "observation", name, p, key="asset_cfg")
        rec["aux0"] = 1
        if op in _ROOT_OBJECT_READS:
            _reads(c, _ROOT_OBJECT_READS[op])
    elif ent != "robot":
        c.entities.names(ent, "body")  # raises: the entity does not exist
        raise NotImplementedError(f"observation term '{name}': asset_cfg names the scene entity '{ent}'; the fused op reads the root state of "
                                  "the robot or of the scene's rigid object")
    if op == "ROOT_QUAT_W":
        _quat_unique(c, name, p, rec)


_IMU_READS = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")
MAX_IMU = _abi.DEFINES["IMX_MAX_IMU"]


def _imu_obs(c, name, p, rec):
    """``imu_orientation`` / ``imu_ang_vel`` / ``imu_lin_acc`` (observations.py:188-231): only ``asset_cfg.name`` is read.  AUX0 = the
    sensor's index among the Imu sensors this plan reads (``Plan.imu_sensors``, first use first); the sensor is fed the four body
    tensors of the robot."""
    ent = _entity_name(p.get("asset_cfg"), "imu")
    if ent not in c.entities.imus:
        raise ValueError(f"observation term '{name}': asset_cfg names the scene entity '{ent}', which is not an Imu of the scene "
                         f"(it has {list(c.entities.imus)})")
    c.entities.imu(ent)  # refuses debug_vis and a prim_path that ends in no robot body, with the reason
    if ent not in c.imu_sensors:
        if len(c.imu_sensors) >= MAX_IMU:
            raise NotImplementedError(f"observation term '{name}': the plan already reads {MAX_IMU} Imu sensors {c.imu_sensors}; one refresh "
                                      f"launch carries at most {MAX_IMU}")
        c.imu_sensors.append(ent)
    rec["aux0"] = c.imu_sensors.index(ent)
    _reads(c, *_IMU_READS)


_T = f"{_MDP}.terminations:"
TERMINATION_TERMS = {
    _T + "time_out": _Fused("TIME_OUT"),
    _T + "illegal_contact": _Fused("ILLEGAL_CONTACT", _Ids("sensor_cfg", "body", required=True), params=("threshold",)),
    _T + "joint_pos_out_of_manual_limit": _Fused("JOINT_POS_MANUAL_LIMIT", _JOINTS, hook=_manual_limit_bounds),
    _T + "bad_orientation": _Fused("BAD_ORIENTATION", params=("limit_angle",)),
    _T + "root_height_below_minimum": _Fused("ROOT_HEIGHT_BELOW_MIN", params=("minimum_height",), hook=_root_height_asset),
    _T + "joint_vel_out_of_limit": _Fused("JOINT_VEL_LIMIT", _JOINTS),
    _T + "joint_vel_out_of_manual_limit": _Fused("JOINT_VEL_MANUAL_LIMIT", _JOINTS, params=("max_velocity",)),
    _T + "joint_effort_out_of_limit": _Fused("JOINT_EFFORT_LIMIT", _JOINTS),
    _T + "command_resample": _Fused("COMMAND_RESAMPLE", hook=_command_resample),
    f"{_VEL}.terminations:terrain_out_of_bounds": _Fused("TERRAIN_OUT_OF_BOUNDS", hook=_terrain_out_of_bounds),
    f"{_LIFT}.terminations:object_reached_goal": _Fused("OBJECT_REACHED_GOAL", params=(("threshold", 0.02),), hook=_object_reached_goal),  # :25-53
    f"{_INHAND}.terminations:max_consecutive_success": _Fused("MAX_CONSECUTIVE_SUCCESS", hook=_max_consecutive_success),  # :18-28
    f"{_INHAND}.terminations:object_away_from_goal": _Fused("OBJECT_AWAY_FROM_GOAL", params=("threshold",), hook=_object_away_from_goal),  # :31-56
    f"{_INHAND}.terminations:object_away_from_robot": _Fused("OBJECT_AWAY_FROM_ROBOT", params=("threshold",), hook=_object_away_from_robot),  # :59-83
}


# -- rewards (isaaclab/envs/mdp/rewards.py, .../locomotion/velocity/mdp/rewards.py, .../classic/cartpole/mdp/rewards.py)
def _is_terminated_term(c, name, p, rec):
    ids, _ = resolve_matching_names(p.get("term_keys", ".*"), [t.name for t in c.termination_terms])
    rec.update(ids_off=c.blob.ints(ids), nids=len(ids))


def _std_squared(c, name, p, rec):
    rec["p0"] = f32(float(p["std"]) ** 2)  # python: std**2 in double, then fp32


def _feet_air_time(c, name, p, rec):
    rec["p1"] = f32(c.step_dt + 1.0e-8)


# -- Spot's own reward terms (isaaclab_tasks .../velocity/config/spot/mdp/rewards.py), 14 functions
def _four_feet(c, name, p, rec):  # `.expand(-1, 4)` fixes the foot count
    if rec["nids"] != 4:
        raise ValueError(f"reward term '{name}': air_time_reward expands its command mask to 4 feet; the sensor cfg selects {rec['nids']} bodies")


def _gait_reward(c, name, p, rec):  # ManagerTermBase; the pairs are resolved once against the contact sensor's bodies
    pairs = p["synced_feet_pair_names"]
    if len(pairs) != 2 or len(pairs[0]) != 2 or len(pairs[1]) != 2:
        raise ValueError("This reward only supports gaits with two pairs of synchronized feet, like trotting.")
    names = c.entities.names("contact_forces", "body")
    ids = []
    for pair in pairs:  # ContactSensor.find_bodies(pair)[0]: target order (preserve_order=False)
        r_ids, _ = resolve_matching_names(list(pair), names)
        if len(r_ids) < 2:
            raise ValueError(f"reward term '{name}': synced feet pair {list(pair)} resolves to {len(r_ids)} body")
        ids += [int(r_ids[0]), int(r_ids[1])]
    rec.update(ids_off=c.blob.ints(ids), nids=4, p0=f32(p["std"]), p1=f32(float(p["max_err"]) ** 2), p2=f32(p["velocity_threshold"]))


def _paired_feet(c, name, p, rec):  # sensor ids and asset ids are separate lists
    if rec["nids"] != rec["nids2"]:
        raise ValueError(f"reward term '{name}': foot_slip_penalty pairs {rec['nids']} sensor bodies with {rec['nids2']} asset bodies")


# -- the classic tasks' own terms (isaaclab_tasks .../classic/humanoid/mdp: Isaac-Ant-v0, Isaac-Humanoid-v0)
def _move_to_target(c, name, p, rec):  # (base_heading_proj ignores the target's z)
    t = _target_pos("reward", name, p)
    rec.update(p1=t[0], p2=t[1])


def _progress_reward(c, name, p, rec):  # ManagerTermBase with per-env potentials -> one term_state slot
    t = _target_pos("reward", name, p)
    rec.update(p0=t[0], p1=t[1], p2=t[2], aux0=len(c.term_slots))
    c.term_slots.append(name)


def _gear_ratio(c, name, p, rec):
    """The two gear-ratio terms read every joint whatever ``asset_cfg`` selects (``asset.data.joint_pos`` unindexed, rewards.py:108-111,
    140): their id list is all joints, their gear table one float per joint.  ``gear_ratio_scaled`` as their ``__init__`` builds it
    (rewards.py:87-97): ones, the matched joints set from ``{regex: ratio}`` (fp32 values), divided by the fp32 maximum."""
    _all_joints(c, name, p, rec)
    g = np.ones(rec["nids"], np.float32)
    idx, _, vals = resolve_matching_names_values(p["gear_ratio"], c.entities.joint_names)
    g[idx] = np.asarray(vals, np.float32)
    rec.update(ids2_off=c.blob.floats((g / g.max()).astype(np.float32).tolist()), nids2=len(g))


def _limits_penalty_ratio(c, name, p, rec):
    _gear_ratio(c, name, p, rec)
    th = float(p["threshold"])
    rec.update(p0=f32(th), p1=f32(1.0 - th))  # (1 - threshold): a Python double


def _power_consumption(c, name, p, rec):
    _gear_ratio(c, name, p, rec)
    if c.action_dim != rec["nids"]:  # (N, A) actions times (N, J) joint velocities
        raise ValueError(f"reward term '{name}': power_consumption multiplies the {c.action_dim} actions with the {rec['nids']} joint velocities")


# -- the reach tasks' own terms (isaaclab_tasks .../manipulation/reach/mdp/rewards.py: Isaac-Reach-Franka-v0, -UR10-v0)
def _reach_body(fn, c, name, p, rec):
    """Each reads ``asset_cfg.body_ids[0]`` (one body id in the record) and the (N, 7) pose command."""
    if c.cmd_dim != 7:
        raise ValueError(f"reward term '{name}': {fn} reads a UniformPoseCommand (N, 7); the cfg's command is {c.cmd_dim} wide")
    ids = c.entities.ids(p.get("asset_cfg"), "body")
    if not ids:
        raise ValueError(f"reward term '{name}': asset_cfg selects no body")
    rec.update(ids_off=c.blob.ints(ids[:1]), nids=1)


# -- the navigation task's own terms (isaaclab_tasks .../navigation/mdp/rewards.py: Isaac-Navigation-Flat-Anymal-C-v0)
def _pose_2d_command(fn, c, name, p, rec):
    """Each reads the (N, 4) pose-2d command: ``command_name`` must name a command term of the cfg that is 4 wide."""
    cname = p.get("command_name")
    ccfg = (c.cfg.get("commands") or {}).get(cname)
    if ccfg is None:
        raise ValueError(f"reward term '{name}': command_name '{cname}' is not a command term of the cfg (it has {list(c.cfg.get('commands') or {})})")
    if command_width(ccfg) != 4 or c.cmd_dim != 4:
        raise ValueError(f"reward term '{name}': {fn} reads a UniformPose2dCommand (N, 4); command '{cname}' is {command_width(ccfg)} wide")


_W, _WV, _WS, _WC = f"{_MDP}.rewards:", f"{_VEL}.rewards:", f"{_SPOT}:", f"{_CLASSIC}.rewards:"
REWARD_TERMS = {
    **{_W + f: _Fused(f.upper()) for f in ("is_alive", "is_terminated", "lin_vel_z_l2", "ang_vel_xy_l2", "flat_orientation_l2",
                                           "action_rate_l2", "action_l2")},
    **{_W + f: _Fused(f.upper(), _JOINTS) for f in ("joint_torques_l2", "joint_vel_l1", "joint_vel_l2", "joint_acc_l2", "joint_deviation_l1",
                                                    "joint_pos_limits", "applied_torque_limits")},
    _W + "is_terminated_term": _Fused("IS_TERMINATED_TERM", hook=_is_terminated_term),
    _W + "base_height_l2": _Fused("BASE_HEIGHT_L2", params=("target_height",), applies=lambda p: p.get("sensor_cfg") is None),
    _W + "joint_vel_limits": _Fused("JOINT_VEL_LIMITS", _JOINTS, params=("soft_ratio",)),
    _W + "undesired_contacts": _Fused("UNDESIRED_CONTACTS", _CONTACTS, params=("threshold",)),
    _W + "contact_forces": _Fused("CONTACT_FORCES", _CONTACTS, params=("threshold",)),
    _W + "track_lin_vel_xy_exp": _Fused("TRACK_LIN_VEL_XY_EXP", hook=_std_squared),
    _W + "track_ang_vel_z_exp": _Fused("TRACK_ANG_VEL_Z_EXP", hook=_std_squared),
    _W + "body_lin_acc_l2": _Fused("BODY_LIN_ACC_L2", _BODIES),
    _WV + "track_lin_vel_xy_yaw_frame_exp": _Fused("TRACK_LIN_VEL_XY_YAW_FRAME_EXP", hook=_std_squared),
    _WV + "track_ang_vel_z_world_exp": _Fused("TRACK_ANG_VEL_Z_WORLD_EXP", hook=_std_squared),
    _WV + "feet_air_time": _Fused("FEET_AIR_TIME", _CONTACTS, params=("threshold",), hook=_feet_air_time),
    _WV + "feet_air_time_positive_biped": _Fused("FEET_AIR_TIME_POSITIVE_BIPED", _CONTACTS, params=("threshold",)),
    _WV + "feet_slide": _Fused("FEET_SLIDE", _CONTACTS, _BODIES),
    f"{_CART}.rewards:joint_pos_target_l2": _Fused("JOINT_POS_TARGET_L2", _JOINTS, params=("target",)),
    _WS + "air_time_reward": _Fused("AIR_TIME_REWARD", _CONTACTS, params=("mode_time", "velocity_threshold"), hook=_four_feet),  # :31-58
    _WS + "base_angular_velocity_reward": _Fused("BASE_ANGULAR_VELOCITY_REWARD", params=("std",)),  # :61-68
    _WS + "base_linear_velocity_reward": _Fused("BASE_LINEAR_VELOCITY_REWARD", params=("std", ("ramp_rate", 0.5), ("ramp_at_vel", 1.0))),  # :71-83
    _WS + "GaitReward": _Fused("GAIT_REWARD", hook=_gait_reward),  # :86-177
    _WS + "foot_clearance_reward": _Fused("FOOT_CLEARANCE_REWARD", _BODIES, params=("target_height", "std", "tanh_mult")),  # :180-188
    _WS + "action_smoothness_penalty": _Fused("ACTION_SMOOTHNESS_PENALTY"),  # :196-198
    _WS + "air_time_variance_penalty": _Fused("AIR_TIME_VARIANCE_PENALTY", _CONTACTS),  # :201-212
    _WS + "base_motion_penalty": _Fused("BASE_MOTION_PENALTY"),  # :216-222
    _WS + "base_orientation_penalty": _Fused("BASE_ORIENTATION_PENALTY"),  # :225-232
    _WS + "foot_slip_penalty": _Fused("FOOT_SLIP_PENALTY", _CONTACTS, _BODIES, params=("threshold",), hook=_paired_feet),  # :235-249
    # the four joint penalties take the norm over ALL joints (rewards.py:252-282)
    _WS + "joint_acceleration_penalty": _Fused("JOINT_ACCELERATION_PENALTY", hook=_all_joints),  # :252-256
    _WS + "joint_position_penalty": _Fused("JOINT_POSITION_PENALTY", params=("stand_still_scale", "velocity_threshold"), hook=_all_joints),  # :259-268
    _WS + "joint_torques_penalty": _Fused("JOINT_TORQUES_PENALTY", hook=_all_joints),  # :271-275
    _WS + "joint_velocity_penalty": _Fused("JOINT_VELOCITY_PENALTY", hook=_all_joints),  # :278-282
    _WC + "upright_posture_bonus": _Fused("UPRIGHT_POSTURE_BONUS", params=("threshold",)),  # :21-27
    _WC + "move_to_target_bonus": _Fused("MOVE_TO_TARGET_BONUS", params=("threshold",), hook=_move_to_target),  # :30-40
    _WC + "progress_reward": _Fused("PROGRESS_REWARD", hook=_progress_reward),  # :43-78
    _WC + "joint_pos_limits_penalty_ratio": _Fused("JOINT_POS_LIMITS_PENALTY_RATIO", hook=_limits_penalty_ratio),  # :81-111
    _WC + "power_consumption": _Fused("POWER_CONSUMPTION", hook=_power_consumption),  # :114-140
    **{f"{_REACH}:{f}": _Fused(f.upper(), params=par, hook=functools.partial(_reach_body, f))
       for f, par in (("position_command_error", ()), ("position_command_error_tanh", ("std",)), ("orientation_command_error", ()))},
    f"{_NAV}.rewards:position_command_error_tanh": _Fused("NAV_POSITION_COMMAND_ERROR_TANH", params=("std",),
                                                          hook=functools.partial(_pose_2d_command, "position_command_error_tanh")),  # :17-22
    f"{_NAV}.rewards:heading_command_error_abs": _Fused("NAV_HEADING_COMMAND_ERROR_ABS",
                                                        hook=functools.partial(_pose_2d_command, "heading_command_error_abs")),  # :25-29
    f"{_LIFT}.rewards:object_is_lifted": _Fused("OBJECT_IS_LIFTED", params=("minimal_height",), hook=_object_is_lifted),  # :20-25
    f"{_LIFT}.rewards:object_ee_distance": _Fused("OBJECT_EE_DISTANCE", params=("std",), hook=_object_ee_distance),  # :28-45
    f"{_LIFT}.rewards:object_goal_distance": _Fused("OBJECT_GOAL_DISTANCE", params=("std", "minimal_height"), hook=_object_goal_distance),  # :48-67
    f"{_INHAND}.rewards:track_orientation_inv_l2": _Fused("TRACK_ORIENTATION_INV_L2", params=(("rot_eps", 1.0e-3),), hook=_track_orientation),  # :71-96
    f"{_INHAND}.rewards:success_bonus": _Fused("SUCCESS_BONUS", hook=_success_bonus),  # :20-44
    f"{_INHAND}.rewards:track_pos_l2": _Fused("TRACK_POS_L2", hook=_track_pos),  # :47-68
    f"{_CABINET}.rewards:approach_ee_handle": _Fused("APPROACH_EE_HANDLE", params=("threshold",), hook=functools.partial(_cabinet_reward, False)),  # :18-40
    f"{_CABINET}.rewards:align_ee_handle": _Fused("ALIGN_EE_HANDLE", hook=functools.partial(_cabinet_reward, False)),  # :43-72
    f"{_CABINET}.rewards:align_grasp_around_handle": _Fused("ALIGN_GRASP_AROUND_HANDLE", hook=functools.partial(_cabinet_reward, True)),  # :75-91
    f"{_CABINET}.rewards:approach_gripper_handle": _Fused("APPROACH_GRIPPER_HANDLE", params=(("offset", 0.04),),
                                                          hook=functools.partial(_cabinet_reward, True)),  # :94-114
    f"{_CABINET}.rewards:grasp_handle": _Fused("GRASP_HANDLE", _Ids("asset_cfg", "joint", required=True), params=("threshold", "open_joint_pos"),
                                               hook=functools.partial(_cabinet_reward, False)),  # :117-135
    f"{_CABINET}.rewards:open_drawer_bonus": _Fused("OPEN_DRAWER_BONUS", _Ids("asset_cfg", "joint", required=True), hook=_drawer_joint,
                                                    articulation=True),  # :138-146
    f"{_CABINET}.rewards:multi_stage_open_drawer": _Fused("MULTI_STAGE_OPEN_DRAWER", _Ids("asset_cfg", "joint", required=True), hook=_drawer_joint,
                                                          articulation=True),  # :149-162
}


# -- observations (isaaclab/envs/mdp/observations.py, .../classic/humanoid/mdp/observations.py); a hook may set rec["dim"] and rec["flags"]
def _quat_unique(c, name, p, rec):
    if p.get("make_quat_unique"):
        rec["flags"] |= F_QUAT_UNIQUE


def _last_action(c, name, p, rec):
    rec["dim"] = c.action_dim


def _generated_commands(c, name, p, rec):
    rec["dim"] = command_width((c.cfg.get("commands") or {}).get(p.get("command_name")))
    if rec["dim"] != c.cmd_dim:
        raise ValueError(f"observation term '{name}': command '{p.get('command_name')}' is {rec['dim']} wide, the env's command {c.cmd_dim}")


def _incoming_wrench(c, name, p, rec):  # observations.py:176-185: 6 columns per body, body_ids order
    rec["dim"] = 6 * rec["nids"]


def _target_obs(c, name, p, rec):
    t = _target_pos("observation", name, p)
    rec.update(p0=t[0], p1=t[1], p2=t[2])


def _height_scan(c, name, p, rec):
    """The scanner's ray table is built by the first height_scan term; later ones without history reuse its ray hits."""
    scanner = c.scene.get("height_scanner")
    if scanner is None:
        raise ValueError(f"Error while parsing '{name}:sensor_cfg'. The scene entity 'height_scanner' does not exist.")
    if c.ray_local is None:
        pc = scanner["pattern_cfg"]
        if _short(func_name(pc["func"]))[1] != "grid_pattern":
            raise NotImplementedError("only grid_pattern ray patterns are on the fused path")
        starts, dirs = grid_pattern(pc["resolution"], pc["size"], tuple(pc.get("direction", (0.0, 0.0, -1.0))),
                                    pc.get("ordering", "xy"))
        off = scanner.get("offset") or {}
        starts = starts + np.asarray(off.get("pos", (0.0, 0.0, 0.0)), np.float32)
        d0 = _quat_apply_np(off.get("rot", (1.0, 0.0, 0.0, 0.0)), dirs[0])
        c.ray_local, c.ray_dir = starts, tuple(float(x) for x in d0)
        c.ray_max = float(scanner.get("max_distance", 1.0e6))
    rec.update(p0=f32(p.get("offset", 0.5)), dim=len(c.ray_local))
    if c.scan_primary < 0:
        c.scan_primary = len(c.obs_recs)
    elif rec["aux1"] == 0:  # no history
        rec["flags"] |= F_SCAN_TWIN  # shares the rays of record `scan_primary` (AUX0)
        rec["aux0"] = c.scan_primary


_O, _OC = f"{_MDP}.observations:", f"{_CLASSIC}.observations:"
OBSERVATION_TERMS = {
    **{_O + f: _Fused(f.upper(), width=w) for f, w in (("base_pos_z", 1), ("base_lin_vel", 3), ("base_ang_vel", 3), ("projected_gravity", 3))},
    **{_O + f: _Fused(f.upper(), width=w, hook=functools.partial(_root_asset, f.upper()))
       for f, w in (("root_pos_w", 3), ("root_quat_w", 4), ("root_lin_vel_w", 3), ("root_ang_vel_w", 3))},
    **{_O + f: _Fused(f.upper(), _JOINTS) for f in ("joint_pos", "joint_pos_rel", "joint_pos_limit_normalized", "joint_vel", "joint_vel_rel")},
    _O + "height_scan": _Fused("HEIGHT_SCAN", hook=_height_scan),
    _O + "last_action": _Fused("LAST_ACTION", hook=_last_action, applies=lambda p: p.get("action_name") is None),
    _O + "generated_commands": _Fused("GENERATED_COMMANDS", hook=_generated_commands),
    _O + "body_incoming_wrench": _Fused("BODY_INCOMING_WRENCH", _BODIES, hook=_incoming_wrench),
    **{_O + f: _Fused(f.upper(), width=w, hook=_imu_obs) for f, w in (("imu_orientation", 4), ("imu_ang_vel", 3), ("imu_lin_acc", 3))},  # :188-231
    _OC + "base_yaw_roll": _Fused("BASE_YAW_ROLL", width=2),  # :19-30
    _OC + "base_up_proj": _Fused("BASE_UP_PROJ", width=1),  # :33-40
    _OC + "base_heading_proj": _Fused("BASE_HEADING_PROJ", width=1, hook=_target_obs),  # :43-58
    _OC + "base_angle_to_target": _Fused("BASE_ANGLE_TO_TARGET", width=1, hook=_target_obs),  # :61-77
    f"{_LIFT}.observations:object_position_in_robot_root_frame": _Fused("OBJECT_POSITION_IN_ROBOT_ROOT_FRAME", width=3, hook=_object_position),  # :19-31
    f"{_INHAND}.observations:goal_quat_diff": _Fused("GOAL_QUAT_DIFF", width=4, hook=_goal_quat_diff),  # :20-38
    # manipulation/cabinet/mdp/observations.py (rel_ee_object_distance :19-24 reads a scene entity "object" the task does not have: no entry)
    **{f"{_CABINET}.observations:{f}": _Fused(f.upper(), width=w, hook=functools.partial(_cabinet_obs, f))
       for f, w in (("rel_ee_drawer_distance", 3), ("ee_pos", 3), ("ee_quat", 4), ("fingertips_pos", 0))},
}
# joint_pos_rel / joint_vel_rel also run on the scene's second articulation (the cabinet's drawer joint)
OBSERVATION_TERMS.update({_O + f: _Fused(f.upper(), _JOINTS, hook=functools.partial(_joint_rel_asset, f), articulation=True)
                          for f in ("joint_pos_rel", "joint_vel_rel")})

_JOINT_ACTIONS = ("JointPositionAction", "JointVelocityAction", "JointEffortAction", "RelativeJointPositionAction",
                  "JointPositionToLimitsAction", "EMAJointPositionToLimitsAction")
_BINARY_ACTIONS = ("BinaryJointPositionAction", "BinaryJointVelocityAction")
_IK_ACTION = "isaaclab.envs.mdp.actions.task_space_actions:DifferentialInverseKinematicsAction"
_OSC_ACTION = "isaaclab.envs.mdp.actions.task_space_actions:OperationalSpaceControllerAction"
_POLICY_ACTION = f"{_NAV}.pre_trained_policy_action:PreTrainedPolicyAction"
_NOISE_OPS = {"add": F_NOISE_ADD, "scale": F_NOISE_SCALE, "abs": F_NOISE_ABS}
# noise function -> the scalar parameters in NOISE_LO / NOISE_HI, flag.  constant_noise: u * (b - b) + b == b for every u: the uniform
# path, bit-identical
_NOISE_FUNCS = {"uniform_noise": ("n_min", "n_max", 0), "constant_noise": ("bias", "bias", 0), "gaussian_noise": ("mean", "std", F_NOISE_GAUSS)}


class PlanCompiler:
    """Compile one env cfg: ``compile()`` runs the managers in a fixed order -- actions, terminations, rewards, observations; each appends
    its id / float lists to the blob as it goes and leaves its records and ``Term`` mirrors on the compiler -- then assembles the plan."""

    def __init__(self, env_cfg: Any, robot: RobotSpec):
        self.cfg = _to_dict(env_cfg)
        self.robot = robot
        self.entities = SceneEntityResolver(robot, self.cfg.get("scene"))
        self.blob = _Blob()
        self.state_reads: set[str] = set()
        self.ft_off: int | None = None  # the frame table (_frame_table): written by the first term that reads a FrameTransformer frame
        self.frame_tables: dict = {}
        self.imu_sensors: list[str] = []  # the Imu sensors the imu_* observation terms read, in index order (_imu_obs)

    def compile(self) -> Plan:
        self._scalars()
        self._actions()
        self._terminations()
        self._rewards()  # reads the termination names, action_dim and cmd_dim
        self._observations()  # reads action_dim and cmd_dim
        return self._assemble()

    def _scalars(self) -> None:
        cfg = self.cfg
        # the env's one command tensor: as wide as its command terms' command (CommandManager.get_command)
        widths = {command_width(c) for c in (cfg.get("commands") or {}).values() if isinstance(c, dict)}
        if len(widths) > 1:
            raise NotImplementedError(f"command terms of widths {sorted(widths)}: the fused path carries one command tensor")
        self.cmd_dim = widths.pop() if widths else 3
        self.scene = cfg.get("scene", {})
        contact = self.scene.get("contact_forces")
        self.history = max(int(contact.get("history_length", 0)), 1) if contact else 1
        self.step_dt = cfg["sim"]["dt"] * cfg["decimation"]
        self.max_len_s = float(cfg["episode_length_s"])
        self.max_len = math.ceil(self.max_len_s / self.step_dt)  # manager_based_rl_env.py:100-103
        g = np.asarray(cfg["sim"].get("gravity", (0.0, 0.0, -9.81)), np.float32)
        self.gravity_dir = g / max(float(np.linalg.norm(g)), 1e-9)  # articulation_data.py:54-60

    def _fuse(self, table: dict, ops: dict, kind: str, name: str, fn: str, p: dict, rec: dict) -> _Fused | None:
        """Fill ``rec`` from the table entry of term function ``fn``.  None (``rec`` untouched): the term is Python-evaluated."""
        e = table.get(fn)
        if e is None or (e.applies is not None and not e.applies(p)):
            if kind in _CLOSED.get(_short(fn)[0], ()):
                raise NotImplementedError(f"{kind} term '{name}': {fn} has no fused op")
            return None
        rec["op"] = ops[e.op]
        for slot, src in (("ids", e.ids), ("ids2", e.ids2)):
            if src is not None:
                ent = _entity_name(p.get(src.key), src.entity)
                if ent in self.entities.articulations and not e.articulation:
                    raise NotImplementedError(f"{kind} term '{name}': '{src.key}' names the scene's second articulation '{ent}'; the fused op "
                                              f"{e.op} reads the robot's tensors only")
                ids = self.entities.ids(p[src.key] if src.required else p.get(src.key), src.kind, src.entity)
                rec.update({f"{slot}_off": self.blob.ints(ids), f"n{slot}": len(ids)})
        if e.hook is not None:
            e.hook(self, name, p, rec)
        for i, key in enumerate(e.params):
            rec[f"p{i}"] = f32(p[key] if isinstance(key, str) else p.get(*key))
        return e

    # -- actions (ActionManager._prepare_terms; JointAction.__init__ joint_actions.py:55-112)
    def _actions(self) -> None:
        blob = self.blob
        self.action_terms: list[Term] = []
        self.act_recs: list[list[int]] = []
        self.action_dim = 0
        self.processed_dim = 0  # columns of the processed action so far (a binary term writes more joints than it takes columns)
        self.ik_terms: list[IkTerm] = []
        self.osc_terms: list[OscTerm] = []
        self.policy_terms: list[PolicyTerm] = []
        for name, tcfg in (self.cfg.get("actions") or {}).items():
            if tcfg is None or not isinstance(tcfg, dict) or "class_type" not in tcfg:
                continue
            cls = func_name(tcfg["class_type"])
            _, cname = _short(cls)
            if cname in _BINARY_ACTIONS:
                self._binary_action(name, cls, tcfg)
                continue
            if cls in (_IK_ACTION, _OSC_ACTION):
                if self.policy_terms:
                    raise NotImplementedError(f"action term '{name}': a {cname} beside the PreTrainedPolicyAction '{self.policy_terms[0].name}' is "
                                              "not on the fused path")
                self._task_space_action(name, cls, tcfg)
                continue
            if cls == _POLICY_ACTION:
                self._policy_action(name, tcfg)
                continue
            if cname not in _JOINT_ACTIONS:
                raise NotImplementedError(f"action term '{name}': class {cls} is not on the fused path")
            ids, jn = resolve_matching_names(tcfg["joint_names"], self.entities.joint_names, bool(tcfg.get("preserve_order")))
            dim = len(ids)
            rec = dict(op=A_JOINT_AFFINE, ids_off=blob.ints(ids), nids=dim, out=self.action_dim, dim=dim)
            if self.processed_dim != self.action_dim:  # P2 = the first processed column; 0 = the raw column (every plan without a binary term)
                rec["p2"] = int(self.processed_dim)
            flags = 0
            scale, offset = tcfg.get("scale", 1.0), tcfg.get("offset", 0.0)
            if cname.endswith("JointPositionToLimitsAction") or (cname == "RelativeJointPositionAction" and tcfg.get("use_zero_offset", True)):
                offset = 0.0  # joint_actions_to_limits.py:111 (no offset at all), joint_actions.py:180-182
            if cname == "EMAJointPositionToLimitsAction":  # the offset slots carry the moving-average weight (:174-193)
                offset = tcfg.get("alpha", 1.0)
                if isinstance(offset, dict):
                    for jname_, v_ in zip(*resolve_matching_names_values(offset, jn)[1:]):
                        if not 0.0 <= v_ <= 1.0:
                            raise ValueError(f"Moving average weight must be in the range [0, 1]. Got {v_} for joint {jname_}.")
                elif isinstance(offset, float):
                    if not 0.0 <= offset <= 1.0:
                        raise ValueError(f"Moving average weight must be in the range [0, 1]. Got {offset}.")
                else:
                    raise ValueError(f"Unsupported moving average weight type: {type(offset)}. Supported types are float and dict.")
            if not isinstance(scale, (int, float, dict)):
                raise ValueError(f"Unsupported scale type: {type(scale)}. Supported types are float and dict.")
            if not isinstance(offset, (int, float, dict)):
                raise ValueError(f"Unsupported offset type: {type(offset)}. Supported types are float and dict.")
            if isinstance(scale, dict):
                tab = [1.0] * dim
                i_, _, v_ = resolve_matching_names_values(scale, jn)
                for i, v in zip(i_, v_):
                    tab[i] = float(v)
                rec["aux0"] = blob.floats(tab)
            else:
                rec["p0"] = float(scale)
            if isinstance(offset, dict):
                tab = [1.0 if cname == "EMAJointPositionToLimitsAction" else 0.0] * dim
                i_, _, v_ = resolve_matching_names_values(offset, jn)
                for i, v in zip(i_, v_):
                    tab[i] = float(v)
                rec["aux1"] = blob.floats(tab)
            else:
                rec["p1"] = float(offset)
            if cname == "JointPositionAction" and tcfg.get("use_default_offset", True):
                flags |= F_ACT_DEFAULT_POS_OFFSET
            if cname == "JointVelocityAction" and tcfg.get("use_default_offset", True):
                flags |= F_ACT_DEFAULT_VEL_OFFSET
            if cname.endswith("JointPositionToLimitsAction") and tcfg.get("rescale_to_limits", True):
                flags |= F_ACT_TO_LIMITS
            if cname == "EMAJointPositionToLimitsAction":
                flags |= F_ACT_EMA
            if tcfg.get("clip") is not None:
                if not isinstance(tcfg["clip"], dict):
                    raise ValueError(f"Unsupported clip type: {type(tcfg['clip'])}. Supported types are dict.")
                tab = [-math.inf, math.inf] * dim
                i_, _, v_ = resolve_matching_names_values(tcfg["clip"], jn)
                for i, v in zip(i_, v_):
                    tab[2 * i], tab[2 * i + 1] = float(v[0]), float(v[1])
                rec["ids2_off"] = blob.floats(tab)
                rec["nids2"] = 2 * dim
                flags |= F_ACT_CLIP
            rec["flags"] = flags
            self.act_recs.append(_rec(**rec))
            self.action_terms.append(Term(name, cls, A_JOINT_AFFINE, dict(tcfg), dim=dim, processed_col=self.processed_dim, processed_dim=dim))
            self.action_dim += dim
            self.processed_dim += dim

    def _task_space_action(self, name: str, cls: str, tcfg: dict) -> None:
        """``DifferentialInverseKinematicsAction`` (task_space_actions.py:53-166) and ``OperationalSpaceControllerAction`` (:248-378,
        664-700): raw -> processed is a per-column scale and an optional clip (IK: cfg.clip; OSC: the clamp of the stiffness and
        damping-ratio columns, +-inf on the others), which the A_JOINT_AFFINE record already does (offset 0, no flag but the clip's);
        the controller's parameters go to ``ik_terms`` / ``osc_terms``.  The record's id list only has to pass the blob validation:
        without the default-offset, to-limits or EMA flag ``action_process_element`` loads the id and never indexes a joint array
        with it, so it is joint 0 for every column."""
        ik = cls == _IK_ACTION
        a, mine, other = ("a", "DifferentialInverseKinematicsAction", "OperationalSpaceControllerAction") if ik else \
            ("an", "OperationalSpaceControllerAction", "DifferentialInverseKinematicsAction")
        terms, others = (self.ik_terms, self.osc_terms) if ik else (self.osc_terms, self.ik_terms)
        if others:
            raise NotImplementedError(f"action term '{name}': {a} {mine} beside the {other} '{others[0].name}'; the fused path runs one "
                                      "task-space term per env")
        if terms:
            raise NotImplementedError(f"action term '{name}': a second {mine} (after '{terms[0].name}'); the fused path runs one per env")
        blob = self.blob
        term = (resolve_ik_term if ik else resolve_osc_term)(name, tcfg, self.robot, action_col=self.action_dim, processed_col=self.processed_dim,
                                                             joint_names=self.entities.joint_names)
        dim = term.width
        rec = dict(op=A_JOINT_AFFINE, ids_off=blob.ints([0] * dim), nids=dim, out=self.action_dim, dim=dim, p1=0.0)
        if self.processed_dim != self.action_dim:
            rec["p2"] = int(self.processed_dim)
        if len(set(term.scale)) == 1:
            rec["p0"] = term.scale[0]
        else:
            rec["aux0"] = blob.floats(term.scale)
        flags = 0
        if term.clip is not None and (ik or any(lo_hi != (-math.inf, math.inf) for lo_hi in term.clip)):
            rec["ids2_off"] = blob.floats([x for lo_hi in term.clip for x in lo_hi])
            rec["nids2"] = 2 * dim
            flags |= F_ACT_CLIP
        rec["flags"] = flags
        self.act_recs.append(_rec(**rec))
        self.action_terms.append(Term(name, cls, A_JOINT_AFFINE, dict(tcfg), dim=dim, processed_col=self.processed_dim, processed_dim=dim))
        terms.append(term)
        self.action_dim += dim
        self.processed_dim += dim

    def _policy_action(self, name: str, tcfg: dict) -> None:
        """``PreTrainedPolicyAction`` (isaaclab_tasks .../navigation/mdp/pre_trained_policy_action.py:34-100).  raw -> processed is a copy
        (``process_actions`` :90-91, ``action_dim`` 3 :73-74): the A_JOINT_AFFINE record with scale 1 and offset 0, as for the task-space
        terms.  The low-level observation group and the low-level action term are compiled as a plan of their own: the term named
        ``velocity_commands`` becomes a generated_commands op over a 3-wide command (the env points the state's command at this term's
        raw action, :64), the term named ``actions`` a last_action op (the env points the buffers' action at low_level_actions, :53-62)."""
        import copy

        if self.policy_terms:
            raise NotImplementedError(f"action term '{name}': a second PreTrainedPolicyAction (after '{self.policy_terms[0].name}'); the fused "
                                      "path runs one per env")
        task_space = self.ik_terms + self.osc_terms
        if task_space:
            raise NotImplementedError(f"action term '{name}': a PreTrainedPolicyAction beside the task-space term '{task_space[0].name}' is not "
                                      "on the fused path")
        lla, group = tcfg.get("low_level_actions"), tcfg.get("low_level_observations")
        if not isinstance(lla, dict) or not isinstance(group, dict) or "class_type" not in lla:
            raise NotImplementedError(f"action term '{name}': a PreTrainedPolicyAction cfg without low_level_actions / low_level_observations "
                                      "is not on the fused path")
        lld = int(tcfg.get("low_level_decimation", 4))
        if lld < 1:
            raise ValueError(f"action term '{name}': low_level_decimation {lld}")
        ll_cls = func_name(lla["class_type"])
        if _short(ll_cls)[1] not in _JOINT_ACTIONS:
            raise NotImplementedError(f"action term '{name}': low-level action class {ll_cls} is not on the fused path (the joint classes "
                                      f"{', '.join(_JOINT_ACTIONS)} are)")
        for key in ("actions", "velocity_commands"):  # (the reference assigns cfg.low_level_observations.<key>.func, :63-66)
            if not isinstance(group.get(key), dict):
                raise ValueError(f"action term '{name}': the low-level observation group has no term '{key}' "
                                 "(PreTrainedPolicyAction remaps the terms of these two names)")
        if group.get("history_length"):
            raise NotImplementedError(f"action term '{name}': a low-level observation group with history (history_length "
                                      f"{group['history_length']}) is not on the fused path")
        if not group.get("concatenate_terms", True):
            raise NotImplementedError(f"action term '{name}': a low-level observation group with concatenate_terms=False feeds no policy")
        group = copy.deepcopy(group)
        for tname, ocfg in group.items():
            if not isinstance(ocfg, dict) or "func" not in ocfg:
                continue
            if ocfg.get("history_length"):
                raise NotImplementedError(f"action term '{name}': low-level observation term '{tname}' has history (history_length "
                                          f"{ocfg['history_length']}); not on the fused path")
            if ocfg.get("modifiers"):
                raise NotImplementedError(f"action term '{name}': low-level observation term '{tname}' has modifiers; not on the fused path")
        group["actions"].update(func=f"{_MDP}.observations:last_action", params={})
        group["velocity_commands"].update(func=f"{_MDP}.observations:generated_commands", params={"command_name": None})
        sub = {"sim": self.cfg["sim"], "decimation": self.cfg["decimation"], "episode_length_s": self.cfg["episode_length_s"],
               "scene": self.cfg.get("scene") or {}, "actions": {"low_level": lla}, "observations": {"ll_policy": group}, "commands": {}}
        try:
            ll = PlanCompiler(sub, self.robot).compile()
        except NotImplementedError as e:
            raise NotImplementedError(f"action term '{name}': low-level {e}") from e
        for t in ll.obs_terms:
            if t.external is not None:
                raise NotImplementedError(f"action term '{name}': low-level observation term '{t.name}' ({t.func}) would be evaluated in "
                                          "Python; not on the fused path")
            if t.op == O_OPS["HEIGHT_SCAN"]:
                raise NotImplementedError(f"action term '{name}': low-level observation term '{t.name}' is a height scan (a rough-terrain "
                                          "low-level policy); not on the fused path")
            if t.op in (O_OPS["IMU_ORIENTATION"], O_OPS["IMU_ANG_VEL"], O_OPS["IMU_LIN_ACC"]):
                raise NotImplementedError(f"action term '{name}': low-level observation term '{t.name}' ({t.func}) reads an Imu sensor: the "
                                          "sensor is refreshed once per env step, before the policy observations, not between the low-level "
                                          "steps; not on the fused path")
        blob = self.blob
        dim = 3
        rec = dict(op=A_JOINT_AFFINE, ids_off=blob.ints([0] * dim), nids=dim, out=self.action_dim, dim=dim, p0=1.0, p1=0.0, flags=0)
        if self.processed_dim != self.action_dim:
            rec["p2"] = int(self.processed_dim)
        self.act_recs.append(_rec(**rec))
        self.action_terms.append(Term(name, _POLICY_ACTION, A_JOINT_AFFINE, dict(tcfg), dim=dim, processed_col=self.processed_dim, processed_dim=dim))
        self.policy_terms.append(PolicyTerm(name=name, action_col=self.action_dim, width=dim, low_level_decimation=lld,
                                            policy_path=tcfg.get("policy_path"), low_level_plan=ll, low_level_action_name="low_level"))
        self.action_dim += dim
        self.processed_dim += dim

    def _binary_action(self, name: str, cls: str, tcfg: dict) -> None:
        """``BinaryJointAction.__init__`` (binary_joint_actions.py:47-96): one raw column; every joint of the term gets its entry of the
        open or the close table (``process_actions`` :118-133).  The position and the velocity class differ in ``apply_actions`` only."""
        blob = self.blob
        ids, jn = resolve_matching_names(tcfg["joint_names"], self.entities.joint_names)
        n = len(ids)
        tabs = []
        for key in ("open_command_expr", "close_command_expr"):
            tab = [0.0] * n
            i_, n_, v_ = resolve_matching_names_values(tcfg[key], jn)
            if len(i_) != n:
                raise ValueError(f"Could not resolve all joints for the action term. Missing: {set(jn) - set(n_)}")
            for i, v in zip(i_, v_):
                tab[i] = f32(v)
            tabs.append(tab)
        if tcfg.get("clip") is not None:
            if not isinstance(tcfg["clip"], dict):
                raise ValueError(f"Unsupported clip type: {type(tcfg['clip'])}. Supported types are dict.")
            if n != 1:  # the reference's clip tensor is (N, action_dim = 1, 2): indexing it with the ids of several joints fails there
                raise NotImplementedError(f"action term '{name}': clip on a binary action term over {n} joints")
            for _, _, (lo, hi) in zip(*resolve_matching_names_values(tcfg["clip"], jn)):
                tabs = [[min(max(x, f32(lo)), f32(hi)) for x in tab] for tab in tabs]  # clamp(where(m, c, o)) == where(m, clamp(c), clamp(o))
        rec = dict(op=A_BINARY_JOINT, ids_off=blob.ints(ids), nids=n, out=self.action_dim, dim=1, aux0=blob.floats(tabs[0]), aux1=blob.floats(tabs[1]))
        if self.processed_dim != self.action_dim:
            rec["p2"] = int(self.processed_dim)
        self.act_recs.append(_rec(**rec))
        self.action_terms.append(Term(name, cls, A_BINARY_JOINT, dict(tcfg), dim=1, processed_col=self.processed_dim, processed_dim=n))
        self.action_dim += 1
        self.processed_dim += n

    # -- terminations (TerminationManager._prepare_terms)
    def _terminations(self) -> None:
        self.termination_terms: list[Term] = []
        self.term_recs: list[list[int]] = []
        self.n_ext_term = 0
        for name, tcfg in (self.cfg.get("terminations") or {}).items():
            if tcfg is None:
                continue
            fn = func_name(tcfg["func"])
            p = dict(tcfg.get("params") or {})
            rec = dict(out=len(self.termination_terms), weight=1 if tcfg.get("time_out") else 0)
            known = self._fuse(TERMINATION_TERMS, T_OPS, "termination", name, fn, p, rec) is not None
            if not known:
                rec.update(op=T_OPS["EXTERNAL"], aux0=self.n_ext_term)
                self.n_ext_term += 1
            self.term_recs.append(_rec(**rec))
            self.termination_terms.append(Term(name, fn, rec["op"], p, external=None if known else tcfg["func"],
                                               time_out=bool(tcfg.get("time_out"))))

    # -- rewards (zero-weight terms keep their slot and record but are skipped at run time: reward_manager.py:145)
    def _rewards(self) -> None:
        self.reward_terms: list[Term] = []
        self.rew_recs: list[list[int]] = []
        self.n_ext_rew = 0
        self.term_slots: list[str] = []  # stateful reward terms, one term_state row each
        for name, tcfg in (self.cfg.get("rewards") or {}).items():
            if tcfg is None:
                continue
            fn = func_name(tcfg["func"])
            p = dict(tcfg.get("params") or {})
            weight = tcfg["weight"]
            if not isinstance(weight, (float, int)):
                raise TypeError(f"Weight for the term '{name}' is not of type float or int. Received: '{type(weight)}'.")
            rec: dict[str, Any] = dict(out=len(self.reward_terms), weight=f32(weight))
            known = self._fuse(REWARD_TERMS, W_OPS, "reward", name, fn, p, rec) is not None
            if not known:
                rec.update(op=W_OPS["EXTERNAL"], aux0=self.n_ext_rew)
                self.n_ext_rew += 1
            self.reward_terms.append(Term(name, fn, rec["op"], p, external=None if known else tcfg["func"], weight=float(weight)))
            self.rew_recs.append(_rec(**rec))  # zero-weight terms keep their record: the kernel skips them at run time, set_term_cfg can wake them

    # -- observations (ObservationManager._prepare_terms, observation_manager.py:337-470): every group of the cfg, in cfg order;
    #    group g fills its own (N, D_g) tensor.  Record OUT = column inside the group, WEIGHT word = group index.
    def _observations(self) -> None:
        obs_groups_cfg = self.cfg.get("observations") or {}
        group_names = [g_ for g_, v in obs_groups_cfg.items() if isinstance(v, dict)]
        if not group_names:
            raise ValueError("env cfg has no observation groups")
        if len(group_names) > MAX_OBS_GROUPS:
            raise NotImplementedError(f"{len(group_names)} observation groups; the fused path carries at most {MAX_OBS_GROUPS}")
        self.obs_recs: list[list[int]] = []
        self.groups: list[ObsGroup] = []
        self.n_ext_obs = 0
        self.mod_state = 0  # floats of modifier state per env
        self.ray_local, self.ray_dir, self.ray_max = None, (0.0, 0.0, -1.0), 1.0e6
        self.scan_primary = -1  # obs record index of the first height_scan term: later ones reuse its ray hits (one cast per ray and step)
        group_keys = ("concatenate_terms", "enable_corruption", "history_length", "flatten_history_dim")
        for gi, gname in enumerate(group_names):
            gcfg = obs_groups_cfg[gname]
            # concatenate_terms=False / flatten_history_dim=False change the SHAPE the manager hands out, not what is computed: the
            # kernel fills the same fused row, ObservationManager returns views of it (env.py)
            grp = ObsGroup(name=gname, enable_corruption=bool(gcfg.get("enable_corruption", False)), first_record=len(self.obs_recs),
                           concatenate=bool(gcfg.get("concatenate_terms", True)))
            for name, tcfg in gcfg.items():
                if name in group_keys or tcfg is None or not isinstance(tcfg, dict) or "func" not in tcfg:
                    continue
                self._observation_term(grp, gi, gcfg, name, tcfg)
            if grp.concatenate and len({len(d) for d in grp.term_dims}) > 1:  # observation_manager.py:89-99
                raise RuntimeError(f"Unable to concatenate observation terms in group '{gname}'. The shapes of the terms are: {grp.term_dims}."
                                   " Please ensure that the shapes are compatible for concatenation. Otherwise, set 'concatenate_terms' to False"
                                   " in the group configuration.")
            grp.num_records = len(self.obs_recs) - grp.first_record
            self.groups.append(grp)

    def _observation_term(self, grp: ObsGroup, gi: int, gcfg: dict, name: str, tcfg: dict) -> None:
        """One observation term: its record (column ``grp.dim`` onwards of group ``gi``) and its ``Term`` mirror."""
        fn = func_name(tcfg["func"])
        p = dict(tcfg.get("params") or {})
        # history (observation_manager.py:412-431): a group-level history_length overrides the terms'; the (N,H,d) window
        # is flattened oldest-first into H*d columns (flatten_history_dim); kept in the obs buffer itself by the kernel
        gh = gcfg.get("history_length")
        hist = int(gh if gh is not None else (tcfg.get("history_length") or 0))
        flat = gcfg.get("flatten_history_dim", True) if gh is not None else tcfg.get("flatten_history_dim", True)
        rec = dict(out=grp.dim, weight=int(gi), flags=0, aux1=hist)
        known = True  # the term FUNCTION is one of the fused ops (else: evaluated by calling the Python term, IMX_O_EXTERNAL)
        # modifiers (observation_manager.py:310-312): modifier.py's five compile to a per-term program run by the kernel on the raw
        # value, whatever produced it.  A chain with a modifier from elsewhere is applied in Python, right after the (then
        # Python-evaluated) term function -- possible for function-style modifiers only (stateful classes need the manager)
        mod_prog, mod_slots, py_mods = [], 0, []
        if tcfg.get("modifiers"):
            try:
                mod_prog, mod_slots = compile_modifiers(tcfg["modifiers"])
            except NotImplementedError:
                for m in tcfg["modifiers"]:
                    m = m if isinstance(m, dict) else m.to_dict()
                    if _short(func_name(m["func"]))[1][:1].isupper():
                        raise NotImplementedError(
                            f"observation term '{name}': class-based modifier {func_name(m['func'])} next to a modifier that is not one of "
                            "isaaclab.utils.modifiers' five cannot run on the fused path")
                    py_mods.append((m["func"], dict(m.get("params") or {})))
                known = False
            last = _short(func_name(tcfg["modifiers"][-1]["func"] if isinstance(tcfg["modifiers"][-1], dict) else tcfg["modifiers"][-1].func))[1]
            # the reference's Integrator returns its state tensor itself; a following in-place clip_/mul_ (no noise in
            # between) writes into that state -- a reference quirk the fused path does not reproduce: refuse instead of differing
            if last == "Integrator" and not (tcfg.get("noise") and grp.enable_corruption) and (tcfg.get("clip") is not None or tcfg.get("scale") is not None):
                raise NotImplementedError(
                    f"observation term '{name}': an Integrator as last modifier followed by clip/scale without noise aliases the "
                    "integrator state in the reference (modifier.py:247-259, observation_manager.py:314-317); not supported")
        entry = self._fuse(OBSERVATION_TERMS, O_OPS, "observation", name, fn, p, rec) if known else None
        if entry is not None:
            dim = rec.setdefault("dim", entry.width or rec.get("nids", 0))
        else:
            # the term function (and a foreign modifier chain) is evaluated in Python; the kernel still applies modifier.py's
            # modifiers, uniform noise, clip and scale to the value.  Its width comes with the cfg.
            known = False
            dim = int(tcfg.get("_dim", 0))
            rec.update(op=O_OPS["EXTERNAL"], aux0=self.n_ext_obs, dim=dim)
            if dim <= 0:
                raise NotImplementedError(
                    f"observation term '{name}' ({fn}) is not on the fused path; give its width as cfg['_dim']")
            self.n_ext_obs += dim
            if hist > 0:
                raise NotImplementedError(f"observation term '{name}': history on a term evaluated in Python is not supported")
        noise = tcfg.get("noise")
        if noise:  # the reference's three noise functions with scalar parameters run in the kernel; anything else must not be dropped silently
            nfn = _short(func_name(noise["func"]))[1]
            opbit = _NOISE_OPS.get(noise.get("operation", "add"))
            if opbit is None:
                raise ValueError(f"Unknown operation in noise: {noise.get('operation')}")  # noise_model.py:38,68,94
            lo, hi, bit = _NOISE_FUNCS.get(nfn, (None, None, 0))
            if lo is not None and all(isinstance(noise.get(k_), (int, float)) for k_ in (lo, hi)):
                rec["flags"] |= opbit | bit
                rec.update(noise_lo=f32(noise[lo]), noise_hi=f32(noise[hi]))
            elif grp.enable_corruption:
                raise NotImplementedError(f"observation term '{name}': noise model {func_name(noise['func'])} is not on the fused path "
                                          "(uniform_noise, constant_noise and gaussian_noise with scalar parameters are)")
        if tcfg.get("clip") is not None:
            rec["flags"] |= F_CLIP
            rec.update(clip_lo=f32(tcfg["clip"][0]), clip_hi=f32(tcfg["clip"][1]))
        if tcfg.get("scale") is not None:
            if not isinstance(tcfg["scale"], (int, float)):
                raise NotImplementedError(f"observation term '{name}': only a scalar `scale` is on the fused path")
            rec["flags"] |= F_SCALE
            rec["scale"] = f32(tcfg["scale"])
        if mod_prog:
            rec["flags"] |= F_MODIFIERS
            rec.update(ids2_off=self.blob.ints(mod_prog), nids2=len(mod_prog), p1=int(self.mod_state))
            self.mod_state += mod_slots * dim
        width = max(hist, 1) * dim
        self.obs_recs.append(_rec(**rec))
        grp.terms.append(Term(name, fn, rec["op"], p, external=None if known else tcfg["func"], dim=width, py_modifiers=py_mods))
        grp.term_dims.append((hist, dim) if hist > 0 and not flat else (width,))
        grp.term_widths.append(width)
        grp.dim += width

    # -- header and tables
    def _assemble(self) -> Plan:
        cfg, robot, blob, groups, scene = self.cfg, self.robot, self.blob, self.groups, self.scene
        if self.policy_terms and len(self.action_terms) > 1:
            raise NotImplementedError(f"action term '{self.policy_terms[0].name}': a PreTrainedPolicyAction beside other action terms "
                                      f"({[t.name for t in self.action_terms if t.name != self.policy_terms[0].name]}) is not on the fused "
                                      "path: the low-level policy reads the term's raw action as the env's whole processed action")
        J, B = robot.num_joints, robot.num_bodies
        Hh, max_len, max_len_s, gdir = self.history, self.max_len, self.max_len_s, self.gravity_dir
        D = sum(g_.dim for g_ in groups)
        ray_local, ray_dir = self.ray_local, self.ray_dir
        R_n = len(ray_local) if ray_local is not None else 0

        # ---- height scanner as a SensorBase: update_period gating and drift (sensor_base.py:196-205,287-297; ray_caster.py:107-114)
        scanner = scene.get("height_scanner")
        scan_period = float((scanner or {}).get("update_period", 0.0) or 0.0)
        drift = tuple((scanner or {}).get("drift_range", (0.0, 0.0)) or (0.0, 0.0))
        scan_stateful = bool(R_n > 0 and (scan_period > 0.0 or drift[0] != 0.0 or drift[1] != 0.0))

        # the step kernel stages words [HEADER_WORDS, end of the reward table) in LDS (id lists + termination and reward records):
        # keep that range small -- the ray table and the observation / action records come after it
        group_off = blob.ints([x for g_ in groups for x in (g_.dim, int(g_.enable_corruption), g_.first_record, g_.num_records)])
        term_off = blob.table(self.term_recs)
        rew_off = blob.table(self.rew_recs)
        ray_off = blob.floats(ray_local.reshape(-1)) if ray_local is not None else 0
        obs_off = blob.table(self.obs_recs)
        act_off = blob.table(self.act_recs)
        w = blob.w
        hdr = {
            "MAGIC": MAGIC, "VERSION": PLAN_VERSION, "J": J, "B": B, "H": Hh, "A": self.action_dim, "D": D, "R": R_n,
            "NTERM": len(self.term_recs), "NREW": len(self.rew_recs), "NOBS": len(self.obs_recs), "NACT": len(self.act_recs),
            "MAX_EP_LEN": max_len, "TERM_OFF": term_off, "REW_OFF": rew_off, "OBS_OFF": obs_off, "ACT_OFF": act_off,
            "TOTAL_WORDS": len(w), "NB": B, "NREW_ALL": len(self.reward_terms), "RAY_OFF": ray_off,
            "NEXT_REW": self.n_ext_rew, "NEXT_TERM": self.n_ext_term, "NEXT_OBS": self.n_ext_obs,
            "RAY_YAW_ONLY": 1 if (scanner and scanner.get("attach_yaw_only")) else 0, "CMD_DIM": self.cmd_dim,
            "MOD_STATE": self.mod_state, "NGROUPS": len(groups), "GROUP_OFF": group_off, "SCAN_SUBSTEPS": int(cfg["decimation"]),
            "SCAN_STATEFUL": int(scan_stateful), "TERM_SLOTS": len(self.term_slots),
            "PA": self.processed_dim if self.processed_dim != self.action_dim else 0,  # 0 = A: the word of every plan without a binary term
        }
        for k, v in hdr.items():
            w[H[k]] = int(v)
        for k, v in {"STEP_DT": f32(self.step_dt), "GRAV_X": gdir[0], "GRAV_Y": gdir[1], "GRAV_Z": gdir[2],
                     "RAYDIR_X": ray_dir[0], "RAYDIR_Y": ray_dir[1], "RAYDIR_Z": ray_dir[2], "RAY_MAXDIST": self.ray_max,
                     "MAX_EP_LEN_S": f32(max_len_s), "SCAN_PERIOD": f32(scan_period), "SCAN_DT": f32(cfg["sim"]["dt"]),
                     "SCAN_DRIFT_LO": f32(drift[0]), "SCAN_DRIFT_HI": f32(drift[1])}.items():
            w[H[k]] = _f2w(float(v))
        arr = np.asarray(w, dtype=np.int64)
        arr = np.where(arr >= 2 ** 31, arr - 2 ** 32, arr).astype(np.int32)
        return Plan(blob=arr, robot=robot, num_joints=J, num_bodies=B, history=Hh, action_dim=self.action_dim, obs_dim=groups[0].dim,
                    num_rays=R_n, obs_groups=groups, obs_dim_total=D, scan_stateful=scan_stateful,
                    scan_drift_range=(float(drift[0]), float(drift[1])), cmd_dim=self.cmd_dim, step_dt=self.step_dt,
                    max_episode_length=max_len, max_episode_length_s=max_len_s, is_finite_horizon=bool(cfg.get("is_finite_horizon", False)),
                    reward_terms=self.reward_terms, termination_terms=self.termination_terms, obs_terms=groups[0].terms,
                    obs_term_dims=groups[0].term_dims, action_terms=self.action_terms,
                    enable_corruption=any(g_.enable_corruption for g_ in groups), ray_starts_local=ray_local, ray_direction=ray_dir,
                    ray_max_distance=self.ray_max, scanner_cfg=scanner, n_ext_rew=self.n_ext_rew, n_ext_term=self.n_ext_term,
                    n_ext_obs=self.n_ext_obs, gravity_dir=tuple(float(x) for x in gdir), mod_state_dim=self.mod_state,
                    term_slots=len(self.term_slots), processed_action_dim=self.processed_dim, ik_terms=self.ik_terms, osc_terms=self.osc_terms,
                    policy_terms=self.policy_terms, state_reads=tuple(sorted(self.state_reads)), frame_tables=dict(self.frame_tables),
                    frame_table_off=int(self.ft_off or 0), imu_sensors=tuple(self.imu_sensors))


def compile_plan(env_cfg: Any, robot: RobotSpec) -> Plan:
    return PlanCompiler(env_cfg, robot).compile()
