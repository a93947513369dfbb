"""Articulation name tables and defaults for the configs in BASELINE.json.

The reference obtains joint/body names and default joint positions from PhysX after loading the robot USD
(``Articulation._initialize_impl``); neither PhysX nor the USD files exist here, so the *names* ship as data.
Defaults follow the asset cfgs (reference ``source/isaaclab_assets/isaaclab_assets/robots/anymal.py:112-121``,
``unitree.py:290-307`` (G1), ``spot.py:151-160``, ``cartpole.py``, ``ant.py:33-42``, the humanoid task's init state, ``franka.py:39-47``,
``universal_robots.py:35-41``, ``allegro.py:50-58``).  The G1, Spot, Ant, Humanoid, Franka and UR10 joint / body orders are synthetic
breadth-first orders of the names the task cfgs' regexes refer to (the true PhysX order is not recoverable offline); term
semantics do not depend on them because every index list is resolved by name through :func:`resolve_matching_names`.
"""

from __future__ import annotations

import dataclasses
import math
import re
from collections.abc import Sequence
from typing import NamedTuple


def resolve_matching_names(keys, list_of_strings: Sequence[str], preserve_order: bool = False):
    """Regex name resolution with the reference's semantics (``isaaclab/utils/string.py:178-271``).

    Each target string may match at most one key (else ``ValueError``); every key must match something (else
    ``ValueError``).  Result order follows ``list_of_strings`` unless ``preserve_order`` (then key order).
    """
    if isinstance(keys, str):
        keys = [keys]
    hits: list[tuple[int, int]] = []  # (key index, target index)
    matched_by: list[str | None] = [None] * len(list_of_strings)
    key_hits = [0] * len(keys)
    for ti, s in enumerate(list_of_strings):
        for ki, k in enumerate(keys):
            if re.fullmatch(k, s):
                if matched_by[ti]:
                    raise ValueError(f"Multiple matches for '{s}': '{matched_by[ti]}' and '{k}'!")
                matched_by[ti] = k
                hits.append((ki, ti))
                key_hits[ki] += 1
    if not all(key_hits):
        missing = [k for k, c in zip(keys, key_hits) if not c]
        raise ValueError(
            f"Not all regular expressions are matched! Unmatched: {missing}. Available strings: {list(list_of_strings)}"
        )
    if preserve_order:
        hits.sort(key=lambda kt: kt[0])  # stable: target order inside one key
    idx = [ti for _, ti in hits]
    return idx, [list_of_strings[i] for i in idx]


def resolve_matching_names_values(data: dict, list_of_strings: Sequence[str]):
    """``{regex: value}`` -> (indices, names, values) in target order (``isaaclab/utils/string.py:274-360``)."""
    idx, names, vals = [], [], []
    matched_by: list[str | None] = [None] * len(list_of_strings)
    key_hits = {k: 0 for k in data}
    for ti, s in enumerate(list_of_strings):
        for k, v in data.items():
            if re.fullmatch(k, s):
                if matched_by[ti]:
                    raise ValueError(f"Multiple matches for '{s}': '{matched_by[ti]}' and '{k}'!")
                matched_by[ti] = k
                idx.append(ti)
                names.append(s)
                vals.append(v)
                key_hits[k] += 1
    if not all(key_hits.values()):
        raise ValueError(f"Not all regular expressions are matched! {key_hits}")
    return idx, names, vals


@dataclasses.dataclass
class RobotSpec:
    name: str
    joint_names: list[str]
    body_names: list[str]
    default_joint_pos: dict  # regex -> value (InitialStateCfg.joint_pos)
    default_root_height: float
    soft_joint_pos_limit_factor: float = 1.0
    joint_pos_limits: tuple[float, float] = (-2.0 * math.pi, 2.0 * math.pi)
    joint_vel_limit: float = 100.0
    command_dim: int = 3  # width of the command the state feed serves: 3 = base velocity (vx, vy, wz), 7 = end-effector pose
    fixed_base: bool = False  # Articulation.is_fixed_base: PhysX then computes no Jacobian row for the root body and no root columns
    object_offset: tuple | None = None  # where the scene's rigid object lies relative to the root in the state feed; None = the Lift task's place

    @property
    def num_joints(self) -> int:
        return len(self.joint_names)

    @property
    def num_bodies(self) -> int:
        return len(self.body_names)

    def default_joint_pos_list(self) -> list[float]:
        out = [0.0] * self.num_joints
        idx, _, vals = resolve_matching_names_values(self.default_joint_pos, self.joint_names)
        for i, v in zip(idx, vals):
            out[i] = float(v)
        return out

    def soft_joint_pos_limits(self) -> list[tuple[float, float]]:
        # Articulation._process_cfg: mean +- 0.5 * range * factor  (reference articulation.py soft limits)
        lo, hi = self.joint_pos_limits
        mean, rng = 0.5 * (lo + hi), hi - lo
        f = self.soft_joint_pos_limit_factor
        return [(mean - 0.5 * rng * f, mean + 0.5 * rng * f)] * self.num_joints


def _is_slice_all(x) -> bool:
    return x is None or x == slice(None) or (isinstance(x, str) and x.replace(" ", "") == "slice(None,None,None)")


class Frame(NamedTuple):
    """One FrameTransformer frame: its name, the asset its body belongs to (0 the robot, 1 the second articulation), the body and its
    index in that asset, the offset position and rotation (w, x, y, z)."""

    name: str
    asset: int
    body: str
    body_id: int
    pos: tuple
    rot: tuple

    def words(self) -> list:
        """The frame as ``IMX_FRAME_WORDS`` blob entries (include/imx.h): two ints, then seven floats."""
        return [int(self.body_id), int(self.asset), *(float(x) for x in self.pos), *(float(x) for x in self.rot)]


class FrameTable(NamedTuple):
    """A resolved FrameTransformer: the asset all its frames sit on, the source frame, the target frames in cfg order."""

    entity: str
    asset: int
    source: Frame
    targets: list

    @property
    def target_frame_names(self) -> list:
        return [f.name for f in self.targets]


@dataclasses.dataclass
class SecondArticulation:
    """The scene's articulation beside the robot (the Open-Drawer task's cabinet): what ``Articulation._initialize_impl`` learns from
    PhysX -- the joint and body names, in the order its tensors are laid out -- and the defaults its cfg's ``init_state`` gives."""

    name: str
    joint_names: list
    body_names: list
    default_joint_pos: list  # one float per joint
    default_joint_vel: list
    root_pos: tuple
    root_rot: tuple  # w, x, y, z
    prim_path: str | None = None
    # what PhysX reports in the reference (ArticulationData.joint_pos_limits / joint_vel_limits) and the cfg's soft_joint_pos_limit_factor:
    # read from the scene entry when it carries them; only a joint reset event on this asset needs them
    joint_pos_limits: list | None = None  # one (lower, upper) per joint
    joint_vel_limits: list | None = None  # one float per joint
    soft_joint_pos_limit_factor: float = 1.0
    root_lin_vel: tuple = (0.0, 0.0, 0.0)
    root_ang_vel: tuple = (0.0, 0.0, 0.0)

    @property
    def num_joints(self) -> int:
        return len(self.joint_names)

    @property
    def default_root_state(self) -> list:
        """``ArticulationData.default_root_state`` of one env: position, w-x-y-z rotation, linear and angular velocity."""
        return [*self.root_pos, *self.root_rot, *self.root_lin_vel, *self.root_ang_vel]

    @property
    def soft_joint_pos_limits(self) -> list | None:
        """Articulation._process_cfg: mean +- 0.5 * range * factor per joint (None without ``joint_pos_limits``)."""
        if self.joint_pos_limits is None:
            return None
        f = self.soft_joint_pos_limit_factor
        return [(0.5 * (lo + hi) - 0.5 * (hi - lo) * f, 0.5 * (lo + hi) + 0.5 * (hi - lo) * f) for lo, hi in self.joint_pos_limits]

    @property
    def num_bodies(self) -> int:
        return len(self.body_names)

    @classmethod
    def from_scene_entry(cls, name: str, ent: dict) -> "SecondArticulation":
        jn, bn = ent.get("joint_names"), ent.get("body_names")
        if not jn or not bn:
            raise ValueError(f"scene entity '{name}' is an Articulation without 'joint_names' / 'body_names' tables: the reference learns them "
                             "from PhysX; here they come with the scene entry (a cfg fixture's side file)")
        init = ent.get("init_state") or {}

        def table(key):  # InitialStateCfg.joint_pos / joint_vel: {regex: value} (articulation.py _process_cfg)
            out = [0.0] * len(jn)
            spec = init.get(key) or {}
            if spec:
                idx, _, vals = resolve_matching_names_values(spec, list(jn))
                for i, v in zip(idx, vals):
                    out[i] = float(v)
            return out

        def limits(key, width):  # a per-joint table of the scene entry: one row for every joint, or one row for all of them
            v = ent.get(key)
            if v is None:
                return None
            rows = list(v)
            if width == 2 and len(rows) == 2 and not isinstance(rows[0], (list, tuple)):
                rows = [rows] * len(jn)
            elif width == 1 and len(rows) == 1:
                rows = rows * len(jn)
            if len(rows) != len(jn):
                raise ValueError(f"scene entity '{name}': '{key}' has {len(rows)} rows, the articulation has {len(jn)} joints")
            return [tuple(float(x) for x in r) for r in rows] if width == 2 else [float(r) for r in rows]

        return cls(name=name, joint_names=list(jn), body_names=list(bn), default_joint_pos=table("joint_pos"), default_joint_vel=table("joint_vel"),
                   root_pos=tuple(float(x) for x in init.get("pos", (0.0, 0.0, 0.0))), root_rot=tuple(float(x) for x in init.get("rot", (1.0, 0.0, 0.0, 0.0))),
                   prim_path=ent.get("prim_path"), joint_pos_limits=limits("joint_pos_limits", 2), joint_vel_limits=limits("joint_vel_limits", 1),
                   soft_joint_pos_limit_factor=float(ent.get("soft_joint_pos_limit_factor", 1.0)),
                   root_lin_vel=tuple(float(x) for x in init.get("lin_vel", (0.0, 0.0, 0.0))),
                   root_ang_vel=tuple(float(x) for x in init.get("ang_vel", (0.0, 0.0, 0.0))))


class SceneEntityResolver:
    """``SceneEntityCfg.resolve`` (isaaclab/managers/scene_entity_cfg.py:112-250) over a robot's name tables: the joint / body ids a
    ``SceneEntityCfg`` selects.  The term compiler resolves the fused terms' entities with it, the env those of Python-evaluated terms.

    ``scene``: the cfg's ``scene`` dict.  Its entries beyond the robot and the two sensors are learnt by ``class_type``: a ``RigidObject`` has
    one body, named after the last component of its ``prim_path``, and no joints (``self.rigid_objects``); a ``FrameTransformer`` is
    resolved to its first target frame by :meth:`frame` and to its source and all its targets by :meth:`frame_table` (``self.frames``
    holds the cfg entries); an ``Articulation`` other than ``robot`` is the scene's second articulation (``self.articulations``,
    :class:`SecondArticulation`): its name tables come with the scene entry (``joint_names`` / ``body_names``: PhysX provides them in
    the reference, a cfg fixture's side file here), its defaults from the entry's ``init_state``.  More than one is refused.  An
    ``Imu`` (``self.imus`` holds the cfg entries) is resolved by :meth:`imu` to the robot body its ``prim_path`` ends in; the entry may
    carry ``body_com_pos_b``, the centre of mass of that body in its link frame ((3,), or (B, 3) for every body of the robot: PhysX
    provides it in the reference), default zeros."""

    def __init__(self, robot: RobotSpec, scene: dict | None = None):
        self.joint_names = list(robot.joint_names)
        self.body_names = list(robot.body_names)
        self.rigid_objects: dict[str, str] = {}  # entity -> its one body's name
        self.frames: dict[str, dict] = {}
        self.ray_casters: dict[str, dict] = {}  # RayCaster entries (the env serves those no height_scan term reads through producers.RayCaster)
        self.imus: dict[str, dict] = {}  # Imu entries (producers.Imu; the imu_* observation terms read them inside the fused step)
        self.articulations: dict[str, SecondArticulation] = {}
        for name, ent in (scene or {}).items():
            cls = ent.get("class_type") if isinstance(ent, dict) else None
            cls = cls if isinstance(cls, str) or cls is None else f"{cls.__module__}:{cls.__qualname__}"
            if cls and cls.endswith(":RigidObject"):
                self.rigid_objects[name] = str(ent.get("prim_path", name)).rstrip("/").rsplit("/", 1)[-1]
            elif cls and cls.endswith(":FrameTransformer"):
                self.frames[name] = ent
            elif cls and cls.endswith(":RayCaster"):
                self.ray_casters[name] = ent
            elif cls and cls.endswith(":Imu"):
                self.imus[name] = ent
            elif cls and cls.endswith(":Articulation") and name != "robot":
                self.articulations[name] = SecondArticulation.from_scene_entry(name, ent)
        if len(self.articulations) > 1:
            raise NotImplementedError(f"the scene has {len(self.articulations)} articulations beside the robot {list(self.articulations)}; the "
                                      "fused path carries the state of one second articulation")
        for name in self.imus:  # an Imu the resolver cannot serve is refused here, with the reason, whether a term reads it or not
            self.imu(name)

    @property
    def second(self) -> "SecondArticulation | None":
        """The scene's second articulation, or None."""
        return next(iter(self.articulations.values()), None)

    def names(self, entity: str, kind: str) -> list[str]:
        if entity in ("robot", "contact_forces"):
            return self.joint_names if kind == "joint" else self.body_names
        if entity in self.rigid_objects:
            return [] if kind == "joint" else [self.rigid_objects[entity]]
        if entity in self.articulations:
            return self.articulations[entity].joint_names if kind == "joint" else self.articulations[entity].body_names
        raise ValueError(f"The scene entity '{entity}' does not exist. Available entities: "
                         f"{['robot', 'contact_forces', 'height_scanner'] + list(self.rigid_objects) + list(self.frames) + list(self.articulations) + list(self.imus)}.")

    def imu(self, entity: str) -> tuple[int, list | None]:
        """Imu ``entity`` resolved: (index of the robot body its ``prim_path`` ends in -- 0 for the articulation root --, the body's
        ``com_pos_b`` from the entry's ``body_com_pos_b`` table or None).  Refused with the reason: ``debug_vis=True``, a body of the
        second articulation or the rigid object, a last segment that is no body at all."""
        if entity not in self.imus:
            raise ValueError(f"The scene entity '{entity}' is not an Imu of the scene (it has {list(self.imus)}).")
        cfg = self.imus[entity]
        if cfg.get("debug_vis"):
            raise NotImplementedError(f"Imu '{entity}': debug_vis=True: the acceleration markers are not drawn (no visualisation here)")
        body = str(cfg.get("prim_path", "")).rstrip("/").rsplit("/", 1)[-1]
        names = self.body_names
        if body in ("Robot", "robot") or (names and body == names[0]):
            idx = 0  # the articulation root
        elif body in names:
            idx = names.index(body)
        elif any(body in a.body_names for a in self.articulations.values()) or body in self.rigid_objects.values():
            raise NotImplementedError(f"Imu '{entity}': its prim_path ends in '{body}', a body of a second articulation or of the rigid object; "
                                      "the sensor is fed the body states of the robot only")
        else:
            raise ValueError(f"Imu '{entity}': its prim_path ends in '{body}', which is neither a body of the robot ({names}) nor its root")
        com = cfg.get("body_com_pos_b")
        if com is not None:
            com = [list(map(float, r)) for r in com] if isinstance(com[0], (list, tuple)) else [float(x) for x in com]
            if isinstance(com[0], list):
                if len(com) != len(names) or any(len(r) != 3 for r in com):
                    raise ValueError(f"Imu '{entity}': body_com_pos_b must be (3,) or ({len(names)}, 3)")
                com = com[idx]
            elif len(com) != 3:
                raise ValueError(f"Imu '{entity}': body_com_pos_b must be (3,) or ({len(names)}, 3)")
        return idx, com

    def frame_table(self, entity: str) -> "FrameTable":
        """FrameTransformer ``entity`` resolved: its source frame and every target frame in cfg order, each on the body its ``prim_path``
        ends in (frame_transformer.py:96-254), of the robot (asset word 0) or of the second articulation (asset word 1).  A frame whose
        body belongs to neither is a ``ValueError`` naming it; a sensor whose frames span both assets is refused: one launch of the
        sensor's kernel reads the body poses of one articulation."""
        if entity not in self.frames:
            raise ValueError(f"The scene entity '{entity}' is not a FrameTransformer of the scene (it has {list(self.frames)}).")
        cfg = self.frames[entity]
        second = self.second

        def resolve(label: str, path: str, offset: dict | None) -> Frame:
            body = str(path).rstrip("/").rsplit("/", 1)[-1]
            prim = str(second.prim_path).rstrip("/") + "/" if second is not None and second.prim_path else None
            if second is not None and body in second.body_names and (body not in self.body_names or (prim and str(path).startswith(prim))):
                asset, bid = 1, second.body_names.index(body)
            elif body in self.body_names:
                asset, bid = 0, self.body_names.index(body)
            else:
                raise ValueError(f"FrameTransformer '{entity}': frame '{label}' sits on '{body}', which is a body neither of the robot "
                                 f"({self.body_names}) nor of a second articulation ({second.body_names if second is not None else 'the scene has none'})")
            off = offset or {}
            return Frame(label, asset, body, bid, tuple(float(x) for x in off.get("pos", (0.0, 0.0, 0.0))),
                         tuple(float(x) for x in off.get("rot", (1.0, 0.0, 0.0, 0.0))))

        source = resolve("source", cfg["prim_path"], cfg.get("source_frame_offset"))
        targets = [resolve(t.get("name") or str(t["prim_path"]).rstrip("/").rsplit("/", 1)[-1], t["prim_path"], t.get("offset"))
                   for t in (cfg.get("target_frames") or [])]
        if not targets:
            raise ValueError(f"FrameTransformer '{entity}' has no target frames")
        assets = {f.asset for f in [source] + targets}
        if len(assets) > 1:
            raise NotImplementedError(f"FrameTransformer '{entity}': its frames sit on bodies of the robot and of '{second.name}' "
                                      f"({[(f.name, f.body) for f in [source] + targets]}); the sensor's kernel reads the body poses of one articulation")
        return FrameTable(entity, assets.pop(), source, targets)

    def frame(self, entity: str) -> tuple[str, tuple, tuple]:
        """``target_frames[0]`` of FrameTransformer ``entity`` -> (robot body name, offset position, offset rotation w, x, y, z): the
        frame sits on the body its ``prim_path`` ends in (frame_transformer.py:189-254)."""
        if entity not in self.frames:
            raise ValueError(f"The scene entity '{entity}' is not a FrameTransformer of the scene (it has {list(self.frames)}).")
        targets = self.frames[entity].get("target_frames") or []
        if not targets:
            raise ValueError(f"FrameTransformer '{entity}' has no target frames")
        t = targets[0]
        off = t.get("offset") or {}
        body = str(t["prim_path"]).rstrip("/").rsplit("/", 1)[-1]
        return body, tuple(float(x) for x in off.get("pos", (0.0, 0.0, 0.0))), tuple(float(x) for x in off.get("rot", (1.0, 0.0, 0.0, 0.0)))

    def ids(self, ent, kind: str, default_entity: str = "robot") -> list[int]:
        """joint_ids / body_ids of a SceneEntityCfg (dict form, live object, or None = function default)."""
        if ent is None:
            return list(range(len(self.names(default_entity, kind))))
        get = (lambda k: ent.get(k)) if isinstance(ent, dict) else (lambda k: getattr(ent, k, None))
        name = get("name")
        names = self.names(name, kind)
        keys, ids = get(f"{kind}_names"), get(f"{kind}_ids")
        preserve = bool(get("preserve_order"))
        if keys is not None:
            keys = [keys] if isinstance(keys, str) else keys
            r_ids, _ = resolve_matching_names(keys, names, preserve)
            if _is_slice_all(ids):
                return list(r_ids)
            ids = [ids] if isinstance(ids, int) else ids
            if list(r_ids) != list(ids) or [names[i] for i in ids] != list(keys):
                raise ValueError(f"Both '{kind}_names' and '{kind}_ids' are specified, and are not consistent.")
            return list(ids)
        if not _is_slice_all(ids):
            return [ids] if isinstance(ids, int) else [int(i) for i in ids]
        return list(range(len(names)))


_LEGS = ("LF", "LH", "RF", "RH")

ANYMAL_C = RobotSpec(
    name="anymal_c",
    # PhysX breadth-first order of anymal_c.usd
    joint_names=[f"{leg}_{j}" for j in ("HAA", "HFE", "KFE") for leg in _LEGS],
    body_names=["base"] + [f"{leg}_{b}" for b in ("HIP", "THIGH", "SHANK", "FOOT") for leg in _LEGS],
    default_joint_pos={".*HAA": 0.0, ".*F_HFE": 0.4, ".*H_HFE": -0.4, ".*F_KFE": -0.8, ".*H_KFE": 0.8},
    default_root_height=0.6,
    soft_joint_pos_limit_factor=0.95,
    joint_vel_limit=7.5,
)

_G1_JOINTS = [
    "left_hip_pitch_joint", "right_hip_pitch_joint", "torso_joint",
    "left_hip_roll_joint", "right_hip_roll_joint", "left_shoulder_pitch_joint", "right_shoulder_pitch_joint",
    "left_hip_yaw_joint", "right_hip_yaw_joint", "left_shoulder_roll_joint", "right_shoulder_roll_joint",
    "left_knee_joint", "right_knee_joint", "left_shoulder_yaw_joint", "right_shoulder_yaw_joint",
    "left_ankle_pitch_joint", "right_ankle_pitch_joint", "left_elbow_pitch_joint", "right_elbow_pitch_joint",
    "left_ankle_roll_joint", "right_ankle_roll_joint", "left_elbow_roll_joint", "right_elbow_roll_joint",
    "left_five_joint", "left_three_joint", "left_zero_joint", "right_five_joint", "right_three_joint",
    "right_zero_joint", "left_six_joint", "left_four_joint", "left_one_joint", "right_six_joint",
    "right_four_joint", "right_one_joint", "left_two_joint", "right_two_joint",
]

G1 = RobotSpec(
    name="g1",
    joint_names=_G1_JOINTS,
    body_names=["pelvis"] + [j.replace("_joint", "_link") for j in _G1_JOINTS],
    default_joint_pos={
        ".*_hip_pitch_joint": -0.20, ".*_knee_joint": 0.42, ".*_ankle_pitch_joint": -0.23,
        ".*_elbow_pitch_joint": 0.87, "left_shoulder_roll_joint": 0.16, "left_shoulder_pitch_joint": 0.35,
        "right_shoulder_roll_joint": -0.16, "right_shoulder_pitch_joint": 0.35, "left_one_joint": 1.0,
        "right_one_joint": -1.0, "left_two_joint": 0.52, "right_two_joint": -0.52,
    },
    default_root_height=0.74,
    soft_joint_pos_limit_factor=0.9,
)

CARTPOLE = RobotSpec(
    name="cartpole",
    joint_names=["slider_to_cart", "cart_to_pole"],
    body_names=["rail", "cart", "pole"],
    default_joint_pos={"slider_to_cart": 0.0, "cart_to_pole": 0.0},
    default_root_height=2.0,
    joint_pos_limits=(-4.0, 4.0),
)

_SPOT_LEGS = ("fl", "fr", "hl", "hr")

SPOT = RobotSpec(
    name="spot",
    # synthetic breadth-first order: hip_x, hip_y, knee of the four legs; the body below the base, one link level at a time
    joint_names=[f"{leg}_{j}" for j in ("hx", "hy", "kn") for leg in _SPOT_LEGS],
    body_names=["body"] + [f"{leg}_{b}" for b in ("hip", "uleg", "lleg", "foot") for leg in _SPOT_LEGS],
    default_joint_pos={"[fh]l_hx": 0.1, "[fh]r_hx": -0.1, "f[rl]_hy": 0.9, "h[rl]_hy": 1.1, ".*_kn": -1.5},
    default_root_height=0.5,
)

# The MuJoCo-style Ant and Humanoid of the classic tasks (isaaclab_assets/robots/ant.py, classic/humanoid/humanoid_env_cfg.py).  Names
# are the ones the task cfgs' regexes refer to, in a synthetic breadth-first order (the PhysX order of the USD files is not recoverable
# offline).  ``joint_pos_limits`` is a round +-1 rad here; the terms that read limits (joint_pos_limit_normalized,
# joint_pos_limits_penalty_ratio) see the state feed's soft limits, default +- 0.45 rad with positions default + U(-0.5, 0.5): about a
# fifth of the joints then lie beyond the 0.98 / 0.99 thresholds of the two cfgs.
_ANT_LEGS = ("front_left", "front_right", "left_back", "right_back")

ANT = RobotSpec(
    name="ant",
    # hips (`*_leg`), then ankles (`*_foot`); bodies: the torso, then the four legs, then the four feet (ant_env_cfg.py:86-92)
    joint_names=[f"{leg}_{j}" for j in ("leg", "foot") for leg in _ANT_LEGS],
    body_names=["torso"] + [f"{leg}_{b}" for b in ("leg", "foot") for leg in _ANT_LEGS],
    default_joint_pos={".*_leg": 0.0, "front_left_foot": 0.785398, "front_right_foot": -0.785398, "left_back_foot": -0.785398,
                       "right_back_foot": 0.785398},
    default_root_height=0.5,
    joint_pos_limits=(-1.0, 1.0),
)

HUMANOID = RobotSpec(
    name="humanoid",
    # the 21 joints the scale / gear-ratio regexes of humanoid_env_cfg.py match exactly once each, parent links first
    joint_names=["lower_waist:0", "lower_waist:1", "right_upper_arm:0", "right_upper_arm:2", "left_upper_arm:0", "left_upper_arm:2",
                 "pelvis", "right_lower_arm", "left_lower_arm", "right_thigh:0", "right_thigh:1", "right_thigh:2", "left_thigh:0",
                 "left_thigh:1", "left_thigh:2", "right_shin", "left_shin", "right_foot:0", "right_foot:1", "left_foot:0", "left_foot:1"],
    body_names=["torso", "head", "lower_waist", "right_upper_arm", "left_upper_arm", "pelvis", "right_lower_arm", "left_lower_arm",
                "right_thigh", "left_thigh", "right_hand", "left_hand", "right_shin", "left_shin", "right_foot", "left_foot"],
    default_joint_pos={".*": 0.0},
    default_root_height=1.34,
    joint_pos_limits=(-1.0, 1.0),
)

# The fixed-base arms of the Reach tasks (isaaclab_assets/robots/franka.py, universal_robots.py; manipulation/reach).  Names are the ones
# the cfgs and the USDs use, joints before fingers and bodies from the base link out, in a synthetic order; the limits are a round
# +-2 pi (terms see the state feed's soft limits).  The root sits at the env origin (init_state pos (0, 0, 0)).  command_dim = 7: the
# feed serves a UniformPoseCommand-shaped command, a position and a unit quaternion in the base frame.
FRANKA_PANDA = RobotSpec(
    name="franka_panda",
    joint_names=[f"panda_joint{i}" for i in range(1, 8)] + ["panda_finger_joint1", "panda_finger_joint2"],
    body_names=[f"panda_link{i}" for i in range(8)] + ["panda_hand", "panda_leftfinger", "panda_rightfinger"],
    default_joint_pos={"panda_joint1": 0.0, "panda_joint2": -0.569, "panda_joint3": 0.0, "panda_joint4": -2.81, "panda_joint5": 0.0,
                       "panda_joint6": 3.037, "panda_joint7": 0.741, "panda_finger_joint.*": 0.04},
    default_root_height=0.0,
    command_dim=7,
    fixed_base=True,
)

UR10 = RobotSpec(
    name="ur10",
    joint_names=["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"],
    body_names=["base_link", "shoulder_link", "upper_arm_link", "forearm_link", "wrist_1_link", "wrist_2_link", "wrist_3_link", "ee_link"],
    default_joint_pos={"shoulder_pan_joint": 0.0, "shoulder_lift_joint": -1.712, "elbow_joint": 1.712, "wrist_1_joint": 0.0,
                       "wrist_2_joint": 0.0, "wrist_3_joint": 0.0},
    default_root_height=0.0,
    command_dim=7,
    fixed_base=True,
)

# ANYmal-C under the navigation task: the same articulation; the state feed serves the (N, 4) pose-2d command (command_dim = 4)
ANYMAL_C_NAV = dataclasses.replace(ANYMAL_C, name="anymal_c_nav", command_dim=4)

# Allegro hand (isaaclab_assets/robots/allegro.py:50-58): the 16 joints in the order the reference's own tasks list them
# (isaaclab_tasks/direct/allegro_hand/allegro_hand_env_cfg.py:45-62: the four finger roots, then each finger's chain); a synthetic
# body list, the root link first.  The feed's command is the in-hand task's (N, 7) goal pose.
_FINGERS = ("index", "middle", "ring", "thumb")
ALLEGRO_HAND = RobotSpec(
    name="allegro_hand",
    joint_names=[f"{f}_joint_0" for f in _FINGERS] + [f"{f}_joint_{i}" for f in _FINGERS for i in (1, 2, 3)],
    body_names=["palm_link"] + [f"{f}_link_{i}" for i in (0, 1, 2, 3) for f in _FINGERS],
    default_joint_pos={"^(?!thumb_joint_0).*": 0.0, "thumb_joint_0": 0.28},
    default_root_height=0.5,
    command_dim=7,
    fixed_base=True,
    object_offset=(0.0, -0.19, 0.06),  # inhand_env_cfg.py: the cube's init pos (0, -0.19, 0.56) over the hand's (0, 0, 0.5)
)

# The Franka of the Open-Drawer task (manipulation/cabinet): the same articulation; the task has no command term, so the state feed
# serves the 3-wide default command no term reads (command_dim = 3)
FRANKA_PANDA_CABINET = dataclasses.replace(FRANKA_PANDA, name="franka_panda_cabinet", command_dim=3)

ROBOTS = {r.name: r for r in (ANYMAL_C, G1, CARTPOLE, SPOT, ANT, HUMANOID, FRANKA_PANDA, UR10, ANYMAL_C_NAV, ALLEGRO_HAND, FRANKA_PANDA_CABINET)}
