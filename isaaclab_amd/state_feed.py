"""Synthetic/recorded articulation-state feed: stands in for PhysX + ``InteractiveScene`` (out of scope).

The reference reads per-step tensors from ``ArticulationData`` (``isaaclab/assets/articulation/articulation_data.py``),
``ContactSensorData`` (``isaaclab/sensors/contact_sensor/contact_sensor_data.py``) and the command manager.  Here those
tensors come from a :class:`StateFeed`: ``S`` pre-generated snapshots resident in HBM, cycled one per env-step, so the
reference path (oracle) and the HIP path are fed *identical* tensors of shape ``(num_envs, dof|bodies)``.
Distributions follow SURVEY.md section 8(d); generation is on CPU with ``torch.Generator().manual_seed(seed)``.
"""

from __future__ import annotations

import math

import torch

from .robots import RobotSpec

# tensors that change every physics step (one copy per snapshot)
DYNAMIC = (
    "root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w",
    "joint_pos", "joint_vel", "joint_acc", "applied_torque", "computed_torque",
    "body_lin_vel_w", "command", "net_forces_w_history",
    "last_air_time", "current_air_time", "current_contact_time", "last_contact_time",
)
# further per-step tensors only a few optional terms read (body_lin_acc_l2, command_resample, foot_clearance_reward, body_incoming_wrench,
# the reach rewards, the lift terms' object): drawn from their own generators so that the tensors above are unchanged by their presence;
# recorded fixtures carry them only when their cfg needs them
EXTRA = ("body_lin_acc_w", "command_time_left", "command_counter", "body_pos_w", "link_incoming_joint_force", "body_quat_w", "object_root_pos_w")
# the rest of the rigid object's root state and the in-hand command's consecutive_success metric (the in-hand terms, the root
# observations on the object): served on request only (StateFeed.ensure_object_state), from a generator of their own -- a feed that is
# never asked allocates nothing and no other tensor changes by a bit
OBJECT_STATE = ("object_root_quat_w", "object_root_lin_vel_w", "object_root_ang_vel_w", "command_consecutive_success")
# the scene's second articulation (the Open-Drawer task's cabinet): ArticulationData.joint_pos / joint_vel / body_pos_w / body_quat_w of
# that asset, (N, J2), (N, J2), (N, B2, 3), (N, B2, 4) -- served on request only (StateFeed.ensure_articulation_state), from a generator of
# their own, like OBJECT_STATE.  The name without the prefix is the field of imx_articulation_state_t
ARTICULATION_STATE = ("articulation_joint_pos", "articulation_joint_vel", "articulation_body_pos_w", "articulation_body_quat_w")
# tensors fixed for the lifetime of the scene
STATIC = ("default_joint_pos", "default_joint_vel", "soft_joint_pos_limits", "soft_joint_vel_limits", "env_origins")


def _quat_from_euler(roll, pitch, yaw):
    cr, sr = torch.cos(roll * 0.5), torch.sin(roll * 0.5)
    cp, sp = torch.cos(pitch * 0.5), torch.sin(pitch * 0.5)
    cy, sy = torch.cos(yaw * 0.5), torch.sin(yaw * 0.5)
    return torch.stack(
        [cy * cr * cp + sy * sr * sp, cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp],
        dim=-1,
    )


def contact_body_groups(robot: RobotSpec) -> dict[str, list[int]]:
    """Which bodies play the 'feet' / 'thigh' / 'base' roles for the synthetic contact distribution."""
    names = robot.body_names
    feet = [i for i, n in enumerate(names) if n.endswith("FOOT") or n.endswith("_ankle_roll_link") or n.endswith("_foot")]
    thigh = [i for i, n in enumerate(names) if n.endswith("THIGH") or n.endswith("_knee_link") or n.endswith("leg")]
    base = [i for i, n in enumerate(names) if n in ("base", "torso_link", "body")]
    return {"feet": feet, "thigh": thigh, "base": base}


def generate_snapshot(robot: RobotSpec, num_envs: int, gen: torch.Generator, history: int = 3,
                      env_spacing: float = 2.5, extent_xy: tuple[float, float] | None = None) -> dict[str, torch.Tensor]:
    """One synthetic post-physics state (CPU tensors).  ``extent_xy``: half-size of the terrain the env origins
    are folded into (so the height-scanner footprint stays on the mesh)."""
    N, J, B = num_envs, robot.num_joints, robot.num_bodies
    f32 = torch.float32

    def U(lo, hi, *shape):
        return torch.rand(*shape, generator=gen, dtype=f32) * (hi - lo) + lo

    def Nrm(std, *shape):
        return torch.randn(*shape, generator=gen, dtype=f32) * std

    out: dict[str, torch.Tensor] = {}
    # env-origin grid (InteractiveScene grid cloner: square grid, spacing 2.5 m, centred)
    rows = int(math.ceil(math.sqrt(N)))
    ii = torch.arange(N)
    ox = (ii // rows).to(f32) * env_spacing
    oy = (ii % rows).to(f32) * env_spacing
    ox -= ox.mean()
    oy -= oy.mean()
    if extent_xy is not None:  # fold into the terrain extent
        ex, ey = extent_xy
        ox = torch.remainder(ox + ex, 2 * ex) - ex
        oy = torch.remainder(oy + ey, 2 * ey) - ey
    origins = torch.stack([ox, oy, torch.zeros(N)], dim=-1)
    out["env_origins"] = origins
    pos = origins.clone()
    # never lattice-aligned: irrational-ish offsets
    pos[:, 0] += U(-0.5, 0.5, N) + 0.0137
    pos[:, 1] += U(-0.5, 0.5, N) + 0.0071
    pos[:, 2] = robot.default_root_height + Nrm(0.03, N)
    out["root_pos_w"] = pos
    out["root_quat_w"] = _quat_from_euler(Nrm(0.15, N), Nrm(0.15, N), U(-math.pi, math.pi, N))
    out["root_lin_vel_w"] = Nrm(0.5, N, 3)
    out["root_ang_vel_w"] = Nrm(0.5, N, 3)

    default = torch.tensor(robot.default_joint_pos_list(), dtype=f32).repeat(N, 1)
    out["default_joint_pos"] = default
    out["default_joint_vel"] = torch.zeros(N, J, dtype=f32)
    out["joint_pos"] = default + U(-0.5, 0.5, N, J)
    out["joint_vel"] = Nrm(1.0, N, J)
    out["joint_acc"] = Nrm(20.0, N, J)
    out["computed_torque"] = Nrm(20.0, N, J)
    # actuator clipping: ~10 % of the efforts saturate (applied != computed)
    out["applied_torque"] = out["computed_torque"].clamp(-32.0, 32.0)
    lim = torch.tensor(robot.soft_joint_pos_limits(), dtype=f32)  # (J,2)
    # tighter synthetic limits so that joint_pos_limits / limit terms are exercised
    lim = torch.stack([default[0] - 0.45, default[0] + 0.45], dim=-1) if robot.name != "cartpole" else lim
    out["soft_joint_pos_limits"] = lim.unsqueeze(0).repeat(N, 1, 1).contiguous()
    out["soft_joint_vel_limits"] = torch.full((N, J), 2.0, dtype=f32)
    out["body_lin_vel_w"] = Nrm(0.5, N, B, 3)

    cmd = U(-1.0, 1.0, N, 3)
    cmd[torch.rand(N, generator=gen) < 0.02] = 0.0
    out["command"] = cmd

    groups = contact_body_groups(robot)
    forces = torch.zeros(N, history, B, 3, dtype=f32)

    def fill(ids, prob, std):
        if not ids:
            return
        k = len(ids)
        on = (torch.rand(N, history, k, generator=gen) < prob).to(f32)
        direction = torch.randn(N, history, k, 3, generator=gen, dtype=f32)
        direction = direction / direction.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        mag = Nrm(std, N, history, k).abs()
        forces[:, :, ids, :] = direction * (mag * on).unsqueeze(-1)

    fill(groups["feet"], 0.5, 60.0)
    fill(groups["thigh"], 0.05, 30.0)
    fill(groups["base"], 0.01, 30.0)
    out["net_forces_w_history"] = forces
    out["last_air_time"] = U(0.0, 0.8, N, B)
    out["current_air_time"] = U(0.0, 0.8, N, B)
    out["last_contact_time"] = U(0.0, 0.8, N, B)
    sel = torch.rand(N, B, generator=gen)
    cct = torch.where(sel < 0.34, torch.zeros(N, B), torch.where(sel < 0.67, U(0.0, 0.04, N, B), U(0.04, 1.0, N, B)))
    out["current_contact_time"] = cct
    # a body in contact has zero air time (ContactSensor bookkeeping, contact_sensor.py:352-379)
    out["current_air_time"] = torch.where(cct > 0, torch.zeros(N, B), out["current_air_time"])
    return out


def generate_extras(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> dict[str, torch.Tensor]:
    """``ArticulationData.body_lin_acc_w`` and the command term's ``time_left`` / ``command_counter`` (CommandTerm,
    isaaclab/managers/command_manager.py:55-62): N(0, 5) accelerations; time_left ~ U(0, 0.1) s and counters in {0,1,2} so that
    ``command_resample`` fires on a few envs."""
    N, B = num_envs, robot.num_bodies
    return {"body_lin_acc_w": torch.randn(N, B, 3, generator=gen) * 5.0,
            "command_time_left": torch.rand(N, generator=gen) * 0.1,
            "command_counter": torch.randint(0, 3, (N,), generator=gen, dtype=torch.int64)}


def generate_body_pos(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``ArticulationData.body_pos_w`` (N, B, 3): x, y ~ N(0, 0.5) around the world origin, heights ~ U(0, 0.3) m (feet swinging
    around a 0.1 m clearance target and links above them; only the heights enter a term)."""
    N, B = num_envs, robot.num_bodies
    xy = torch.randn(N, B, 2, generator=gen) * 0.5
    z = torch.rand(N, B, 1, generator=gen) * 0.3
    return torch.cat([xy, z], dim=-1).contiguous()


def generate_link_wrench(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``root_physx_view.get_link_incoming_joint_force()`` (N, B, 6): the wrench each body's incoming joint transmits, force N(0, 20) N
    then torque N(0, 2) N m (what body_incoming_wrench observes)."""
    N, B = num_envs, robot.num_bodies
    force = torch.randn(N, B, 3, generator=gen) * 20.0
    torque = torch.randn(N, B, 3, generator=gen) * 2.0
    return torch.cat([force, torque], dim=-1).contiguous()


def generate_body_quat(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``ArticulationData.body_quat_w`` (N, B, 4) w, x, y, z: uniform unit quaternions (normalised N(0, 1) 4-vectors), half of them
    with w < 0 -- the sign a PhysX pose carries is arbitrary."""
    q = torch.randn(num_envs, robot.num_bodies, 4, generator=gen)
    return (q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)).contiguous()


def generate_object_offset(num_envs: int, gen: torch.Generator, mean=None) -> torch.Tensor:
    """Where the scene's rigid object lies relative to the robot root (N, 3): around the Lift task's initial (0.5, 0, 0.055) m
    (lift_env_cfg.py / joint_pos_env_cfg.py), x, y ~ N(0, 0.1) about it, the height uniform in [-0.15, 0.5) m -- below the -0.05 m
    dropping threshold on a sixth of the envs, below and above the 0.04 m lifting height on the rest.  ``mean`` (a robot's
    ``object_offset``): N(mean, 0.08) on every axis instead -- for the Allegro hand's (0, -0.19, 0.06) m (inhand_env_cfg.py: the cube
    0.56 m up, the hand 0.5 m) about one env in six lies beyond the in-hand task's 0.3 m reach."""
    if mean is not None:
        return (torch.randn(num_envs, 3, generator=gen) * 0.08 + torch.tensor(mean, dtype=torch.float32)).contiguous()
    xy = torch.randn(num_envs, 2, generator=gen) * 0.1 + torch.tensor([0.5, 0.0])
    z = 0.055 + (torch.rand(num_envs, 1, generator=gen) * 0.65 - 0.205)
    return torch.cat([xy, z], dim=-1).contiguous()


def generate_object_state(num_envs: int, gen: torch.Generator) -> dict[str, torch.Tensor]:
    """The rest of ``RigidObjectData``'s root state and the in-hand command's metric: ``root_quat_w`` (N, 4) uniform unit quaternions w, x, y, z
    (normalised N(0, 1) 4-vectors: w < 0 on half of them), ``root_lin_vel_w`` ~ N(0, 0.3) m/s, ``root_ang_vel_w`` ~ N(0, 1) rad/s, and
    ``InHandReOrientationCommand.metrics["consecutive_success"]`` (N), whole numbers 0..59 as float32 (the reference keeps a float tensor):
    at or past the task's 50 on a sixth of the envs."""
    q = torch.randn(num_envs, 4, generator=gen)
    return {"object_root_quat_w": (q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)).contiguous(),
            "object_root_lin_vel_w": torch.randn(num_envs, 3, generator=gen) * 0.3,
            "object_root_ang_vel_w": torch.randn(num_envs, 3, generator=gen),
            "command_consecutive_success": torch.randint(0, 60, (num_envs,), generator=gen).to(torch.float32)}


def _quat_apply(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """quat_apply (utils/math.py:546-566) in the dtype given: v + w t + xyz x t, t = 2 xyz x v."""
    xyz, w = q[..., 1:], q[..., :1]
    t = torch.linalg.cross(xyz, v) * 2
    return v + w * t + torch.linalg.cross(xyz, t)


def frame_positions(table, body_pos_w: torch.Tensor, body_quat_w: torch.Tensor) -> torch.Tensor:
    """World positions (N, T, 3), float64, of the target frames of a resolved FrameTransformer (``robots.FrameTable``) on the body
    poses given: body position + quat_apply(body quaternion, offset position)."""
    ids = [f.body_id for f in table.targets]
    off = torch.tensor([f.pos for f in table.targets], dtype=torch.float64, device=body_pos_w.device)
    return body_pos_w[:, ids].double() + _quat_apply(body_quat_w[:, ids].double(), off.expand(body_pos_w.shape[0], -1, -1))


def generate_articulation_state(spec, num_envs: int, gen: torch.Generator, root_pos_w: torch.Tensor, body_pos_w: torch.Tensor,
                                body_quat_w: torch.Tensor, frame_tables: dict | None = None) -> dict[str, torch.Tensor]:
    """The second articulation's tensors (``spec``: a ``robots.SecondArticulation``) beside a robot snapshot (CPU tensors): joint
    positions = the defaults + U(-0.05, 0.45) (a drawer joint then lies on both sides of the Open-Drawer rewards' 0.01 / 0.2 / 0.3 m
    stages), joint velocities ~ N(0, 0.5), body quaternions uniform on the sphere, body positions = the robot root + the asset's
    initial root offset + N(0, 0.3) per body.  With ``frame_tables`` (the plan's resolved ``ee_frame`` / ``cabinet_frame``) the body
    of the cabinet_frame's first target -- the drawer handle -- is placed against the robot's frames in half of the envs, so that every
    branch of the cabinet rewards occurs at any env count: env e with e mod 4 == 0 has the handle frame within 0.06 m of the tool
    centre point (both sides of grasp_handle's 0.03 m), e mod 4 == 1 has it 0.05 .. 0.35 m away horizontally (both sides of
    approach_ee_handle's 0.2 m) at a height between the two fingertips' (graspable where the left fingertip is the upper one)."""
    N, J2, B2 = num_envs, spec.num_joints, spec.num_bodies
    f32 = torch.float32
    jp = torch.tensor(spec.default_joint_pos, dtype=f32).repeat(N, 1) + (torch.rand(N, J2, generator=gen) * 0.5 - 0.05)
    jv = torch.randn(N, J2, generator=gen) * 0.5
    q = torch.randn(N, B2, 4, generator=gen)
    q = (q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)).contiguous()
    pos = (root_pos_w + torch.tensor(spec.root_pos, dtype=f32)).unsqueeze(1) + torch.randn(N, B2, 3, generator=gen) * 0.3
    u = torch.rand(N, 4, generator=gen, dtype=torch.float64)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen, dtype=torch.float64), dim=-1)
    ee, cab = ((frame_tables or {}).get(k) for k in ("ee_frame", "cabinet_frame"))
    if ee is not None and cab is not None and ee.asset == 0 and cab.asset == 1 and len(ee.targets) >= 3:
        tips = frame_positions(ee, body_pos_w, body_quat_w)  # tool centre point, left fingertip, right fingertip
        handle = cab.targets[0]
        cls = torch.arange(N) % 4
        near = tips[:, 0] + d * (u[:, 0:1] * 0.06)
        ang = u[:, 1] * (2.0 * math.pi)
        rad = 0.05 + 0.3 * u[:, 2]
        between = torch.stack([tips[:, 0, 0] + rad * torch.cos(ang), tips[:, 0, 1] + rad * torch.sin(ang),
                               tips[:, 1, 2] + (0.1 + 0.8 * u[:, 3]) * (tips[:, 2, 2] - tips[:, 1, 2])], dim=-1)
        want = torch.where((cls == 0).unsqueeze(-1), near, between)
        # the handle body that puts the handle FRAME there: frame = body + quat_apply(body quaternion, offset)
        body = want - _quat_apply(q[:, handle.body_id].double(), torch.tensor(handle.pos, dtype=torch.float64).expand(N, 3))
        sel = cls < 2
        pos[sel, handle.body_id] = body[sel].float()
    return {"articulation_joint_pos": jp.contiguous(), "articulation_joint_vel": jv.contiguous(), "articulation_body_pos_w": pos.contiguous(),
            "articulation_body_quat_w": q}


def generate_jacobians(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``root_physx_view.get_jacobians()`` (N, NB, 6, ND), world frame: NB = the bodies (without the root body of a fixed base), ND =
    the joints (after six root columns of a floating base).  Linear rows 0-2 ~ U(-0.8, 0.8), angular rows 3-5 ~ U(-1, 1): the size of
    an arm's entries a metre from its joints."""
    NB = robot.num_bodies - 1 if robot.fixed_base else robot.num_bodies
    ND = robot.num_joints if robot.fixed_base else robot.num_joints + 6
    lin = torch.rand(num_envs, NB, 3, ND, generator=gen) * 1.6 - 0.8
    ang = torch.rand(num_envs, NB, 3, ND, generator=gen) * 2.0 - 1.0
    return torch.cat([lin, ang], dim=2).contiguous()


DYNAMICS = ("mass_matrices", "gravity_compensation_forces", "body_ang_vel_w")


def generate_dynamics(robot: RobotSpec, num_envs: int, gen: torch.Generator) -> dict[str, torch.Tensor]:
    """What an OperationalSpaceControllerAction reads beside the Jacobians (task_space_actions.py:568-574, 617-634):
    ``root_physx_view.get_generalized_mass_matrices()`` (N, NM, NM), NM = the joints, symmetric positive definite with an arm-like
    spectrum -- sym(B B^T / NM + diag(U(0.05, 1.5))), B ~ N(0, 1): condition numbers of a few to a few tens;
    ``get_gravity_compensation_forces()`` (N, NM) ~ N(0, 5) N m; ``ArticulationData.body_ang_vel_w`` (N, B, 3) ~ N(0, 0.5) rad/s like
    ``body_lin_vel_w``."""
    N, NM, B = num_envs, robot.num_joints, robot.num_bodies
    b = torch.randn(N, NM, NM, generator=gen)
    m = b @ b.transpose(1, 2) / NM + torch.diag_embed(torch.rand(N, NM, generator=gen) * 1.45 + 0.05)
    return {"mass_matrices": ((m + m.transpose(1, 2)) * 0.5).contiguous(),
            "gravity_compensation_forces": torch.randn(N, NM, generator=gen) * 5.0,
            "body_ang_vel_w": torch.randn(N, B, 3, generator=gen) * 0.5}


# UniformPoseCommand ranges of the Reach tasks (manipulation/reach/reach_env_cfg.py): the position of the end-effector target in the base
# frame; the orientation is any unit quaternion (the cfgs' roll 0, pitch pi or pi / 2, yaw +-3.14 Euler draws are a subset of it)
POSE_COMMAND_POS_RANGE = ((0.35, 0.65), (-0.2, 0.2), (0.15, 0.5))


def generate_pose_command(num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``UniformPoseCommand.command`` (N, 7): position uniform in :data:`POSE_COMMAND_POS_RANGE`, then a unit quaternion w, x, y, z in
    the base frame (w < 0 on half of the envs: ``make_quat_unique=False`` keeps either sign)."""
    pos = torch.stack([torch.rand(num_envs, generator=gen) * (hi - lo) + lo for lo, hi in POSE_COMMAND_POS_RANGE], dim=-1)
    q = torch.randn(num_envs, 4, generator=gen)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.cat([pos, q], dim=-1).contiguous()


def generate_pose_2d_command(num_envs: int, gen: torch.Generator) -> torch.Tensor:
    """``UniformPose2dCommand.command`` (N, 4) in the base frame (pose_2d_command.py): ``pos_command_b`` -- xy ~ U(-3, 3) as the
    navigation cfg's ranges, z ~ U(-0.05, 0.05) (the target sits at the robot's default root height) -- and ``heading_command_b`` ~
    U(-pi, pi)."""
    u = torch.rand(num_envs, 4, generator=gen)
    lo = torch.tensor([-3.0, -3.0, -0.05, -math.pi])
    hi = torch.tensor([3.0, 3.0, 0.05, math.pi])
    return (u * (hi - lo) + lo).contiguous()


class StateFeed:
    """``S`` snapshots of the post-physics state held on ``device``; ``advance()`` moves to the next one.

    ``feed[name]`` returns the current tensor for ``name`` (a view into the snapshot stack; static tensors are
    shared).  ``feed.index`` identifies the current snapshot so callers can cache per-snapshot pointer structs.
    """

    def __init__(self, robot: RobotSpec, num_envs: int, device: str | torch.device = "cpu", seed: int = 42,
                 num_snapshots: int = 4, history: int = 3, extent_xy: tuple[float, float] | None = None,
                 gravity=(0.0, 0.0, -9.81), jacobians: bool = False):
        self.robot = robot
        self.seed = seed
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.num_snapshots = num_snapshots
        self.history = history
        gen = torch.Generator().manual_seed(seed)
        snaps = [generate_snapshot(robot, num_envs, gen, history, extent_xy=extent_xy) for _ in range(num_snapshots)]
        self._stack: dict[str, torch.Tensor] = {}
        gen_x = torch.Generator().manual_seed(seed + 0x5EED)
        gen_p = torch.Generator().manual_seed(seed + 0xB0D7)
        gen_w = torch.Generator().manual_seed(seed + 0x1F0C)
        gen_q = torch.Generator().manual_seed(seed + 0x0A7E)
        gen_c = torch.Generator().manual_seed(seed + 0x9C3D)
        gen_o = torch.Generator().manual_seed(seed + 0x0B1E)
        for sn in snaps:
            sn.update(generate_extras(robot, num_envs, gen_x))
            sn["body_pos_w"] = generate_body_pos(robot, num_envs, gen_p)
            sn["link_incoming_joint_force"] = generate_link_wrench(robot, num_envs, gen_w)
            sn["body_quat_w"] = generate_body_quat(robot, num_envs, gen_q)
            sn["object_root_pos_w"] = generate_object_offset(num_envs, gen_o, robot.object_offset)  # (the offset; the root position is added below)
            if robot.command_dim == 7:  # a pose command (the velocity command drawn above is dropped: other tensors keep their draws)
                sn["command"] = generate_pose_command(num_envs, gen_c)
            elif robot.command_dim == 4:  # the navigation task's pose-2d command, likewise
                sn["command"] = generate_pose_2d_command(num_envs, gen_c)
            elif robot.command_dim != 3:
                raise ValueError(f"robot {robot.name}: the feed serves 3-, 4- or 7-wide commands, not {robot.command_dim}")
        for name in DYNAMIC + EXTRA:
            self._stack[name] = torch.stack([s[name] for s in snaps], dim=0).to(self.device).contiguous()
        # every snapshot keeps the same origins/defaults; root xy of later snapshots re-uses snapshot-0 origins
        self._static = {name: snaps[0][name].to(self.device).contiguous() for name in STATIC}
        for k in range(1, num_snapshots):
            delta = (snaps[k]["root_pos_w"] - snaps[k]["env_origins"]).to(self.device)
            self._stack["root_pos_w"][k] = self._static["env_origins"] + delta
        self._stack["object_root_pos_w"] += self._stack["root_pos_w"]  # RigidObjectData.root_pos_w: next to the robot, in the world frame
        g = torch.tensor(gravity, dtype=torch.float32)
        self.gravity_dir = (g / g.norm().clamp_min(1e-9)).tolist()
        self.index = 0
        if jacobians:
            self.ensure_jacobians()

    def ensure_jacobians(self) -> None:
        """Serve ``feed["jacobians"]`` (:func:`generate_jacobians`): built on the first request from a generator of its own seeded off
        the feed's seed, so no other tensor changes by a bit and a feed that never asks allocates nothing.  A recorded feed
        (``from_tensors``) has them only when its snapshots carried them."""
        if "jacobians" in self._stack:
            return
        seed = getattr(self, "seed", None)
        if seed is None:
            raise KeyError("this recorded feed carries no 'jacobians'")
        gen = torch.Generator().manual_seed(seed + 0x7AC0)
        self._stack["jacobians"] = torch.stack([generate_jacobians(self.robot, self.num_envs, gen) for _ in range(self.num_snapshots)],
                                               dim=0).to(self.device).contiguous()

    def ensure_dynamics(self) -> None:
        """Serve ``feed["mass_matrices"]``, ``feed["gravity_compensation_forces"]`` and ``feed["body_ang_vel_w"]``
        (:func:`generate_dynamics`): built on the first request from a generator of their own seeded off the feed's seed, like the
        Jacobians: no other tensor changes by a bit and a feed that never asks allocates nothing.  A recorded feed (``from_tensors``) has
        them only when its snapshots carried them."""
        if all(n in self._stack for n in DYNAMICS):
            return
        seed = getattr(self, "seed", None)
        if seed is None:
            raise KeyError(f"this recorded feed carries no {[n for n in DYNAMICS if n not in self._stack]}")
        gen = torch.Generator().manual_seed(seed + 0xD1A5)
        snaps = [generate_dynamics(self.robot, self.num_envs, gen) for _ in range(self.num_snapshots)]
        for n in DYNAMICS:
            self._stack[n] = torch.stack([sn[n] for sn in snaps], dim=0).to(self.device).contiguous()

    def ensure_object_state(self) -> None:
        """Serve the :data:`OBJECT_STATE` tensors (:func:`generate_object_state`): built on the first request from a generator of their own
        seeded off the feed's seed, like the Jacobians.  A recorded feed (``from_tensors``) has them only when its snapshots carried them."""
        if all(n in self._stack for n in OBJECT_STATE):
            return
        seed = getattr(self, "seed", None)
        if seed is None:
            raise KeyError(f"this recorded feed carries no {[n for n in OBJECT_STATE if n not in self._stack]}")
        gen = torch.Generator().manual_seed(seed + 0x0B57)
        snaps = [generate_object_state(self.num_envs, gen) for _ in range(self.num_snapshots)]
        for n in OBJECT_STATE:
            self._stack[n] = torch.stack([sn[n] for sn in snaps], dim=0).to(self.device).contiguous()

    def ensure_articulation_state(self, spec, frame_tables: dict | None = None) -> None:
        """Serve the :data:`ARTICULATION_STATE` tensors of the scene's second articulation ``spec`` (a ``robots.SecondArticulation``;
        :func:`generate_articulation_state`): built on the first request from a generator of their own seeded off the feed's seed, like
        the object state -- no other tensor changes by a bit and a feed that never asks allocates nothing.  ``frame_tables``: the plan's
        resolved FrameTransformer sensors, against which the drawer handle is placed.  A recorded feed (``from_tensors``) has the
        tensors only when its snapshots carried them."""
        if all(n in self._stack for n in ARTICULATION_STATE):
            return
        seed = getattr(self, "seed", None)
        if seed is None:
            raise KeyError(f"this recorded feed carries no {[n for n in ARTICULATION_STATE if n not in self._stack]}")
        gen = torch.Generator().manual_seed(seed + 0xCAB1)
        cpu = lambda n, k: self._stack[n][k].cpu()  # noqa: E731
        snaps = [generate_articulation_state(spec, self.num_envs, gen, cpu("root_pos_w", k), cpu("body_pos_w", k), cpu("body_quat_w", k), frame_tables)
                 for k in range(self.num_snapshots)]
        for n in ARTICULATION_STATE:
            self._stack[n] = torch.stack([sn[n] for sn in snaps], dim=0).to(self.device).contiguous()

    @classmethod
    def from_tensors(cls, robot: RobotSpec, snapshots: list[dict[str, torch.Tensor]], device="cpu",
                     gravity_dir=(0.0, 0.0, -1.0)) -> "StateFeed":
        """Recorded feed: ``snapshots[k][name]`` for every DYNAMIC name; STATIC names taken from ``snapshots[0]``."""
        self = cls.__new__(cls)
        self.robot = robot
        self.device = torch.device(device)
        self.num_snapshots = len(snapshots)
        self.num_envs = snapshots[0]["root_pos_w"].shape[0]
        self.history = snapshots[0]["net_forces_w_history"].shape[1]
        self._stack = {
            n: torch.stack([torch.as_tensor(s[n]) for s in snapshots], 0).to(self.device).contiguous()
            for n in DYNAMIC + EXTRA + ("jacobians",) + DYNAMICS + OBJECT_STATE + ARTICULATION_STATE if n in snapshots[0]
        }
        self._static = {n: torch.as_tensor(snapshots[0][n]).to(self.device).contiguous() for n in STATIC}
        self.gravity_dir = [float(x) for x in gravity_dir]
        self.index = 0
        return self

    def physx(self, name: str) -> torch.Tensor:
        """The current snapshot in the layout PhysX tensor views deliver (articulation_data.py:365-380): ``root_transforms`` (N,7) = position +
        quaternion XYZW, ``root_velocities`` (N,6) = linear + angular.  Built once per feed, resident like the snapshots."""
        if getattr(self, "_physx", None) is None:
            q = self._stack["root_quat_w"]
            self._physx = {"root_transforms": torch.cat([self._stack["root_pos_w"], q[..., 1:4], q[..., 0:1]], dim=-1).contiguous(),
                           "root_velocities": torch.cat([self._stack["root_lin_vel_w"], self._stack["root_ang_vel_w"]], dim=-1).contiguous()}
        return self._physx[name][self.index]

    def advance(self) -> int:
        self.index = (self.index + 1) % self.num_snapshots
        return self.index

    def seek(self, index: int):
        self.index = index % self.num_snapshots

    def __getitem__(self, name: str) -> torch.Tensor:
        if name in self._static:
            return self._static[name]
        return self._stack[name][self.index]

    def snapshot(self, index: int | None = None) -> dict[str, torch.Tensor]:
        k = self.index if index is None else index
        d = {n: t[k] for n, t in self._stack.items()}
        d.update(self._static)
        return d

    def names(self):
        return tuple(self._stack) + tuple(STATIC)
