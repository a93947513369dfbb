"""Host-side mirrors of the reference's per-step input producers, running on libimx:

* :class:`ContactSensorState` -- ``ContactSensor`` data buffers + ``update(dt)`` (reference
  isaaclab/sensors/contact_sensor/contact_sensor.py:140-210,320-379; isaaclab/sensors/sensor_base.py:182-205,287-297)
* :class:`UniformVelocityCommand` -- ``CommandTerm.reset/compute`` + the uniform velocity command
  (isaaclab/managers/command_manager.py:119-187; isaaclab/envs/mdp/commands/velocity_command.py:37-160)
* :class:`UniformPoseCommand` -- the same two steps for the uniform pose command of the Reach tasks
  (isaaclab/envs/mdp/commands/pose_command.py:25-127)
* :class:`UniformPose2dCommand`, :class:`TerrainBasedPose2dCommand` -- the same two steps for the pose-2d commands of the Navigation
  task (isaaclab/envs/mdp/commands/pose_2d_command.py:26-203)
* :class:`InHandReOrientationCommand` -- the same two steps for the in-hand re-orientation command of the Repose-Cube task
  (isaaclab_tasks .../manipulation/inhand/mdp/commands/orientation_command.py:22-124), stand-alone: no env runs it yet
* :class:`FrameTransformer` -- the sensor's six data tensors from an articulation's body poses
  (isaaclab/sensors/frame_transformer/frame_transformer.py:337-384)
* :class:`RayCaster` -- the ray-caster sensor with any ray pattern (grid, Bpearl, lidar) and the full orientation of its body, one
  launch per update (isaaclab/sensors/ray_caster/ray_caster.py:107-114,201-260; isaaclab/sensors/sensor_base.py:182-205,287-296)

Attribute names follow the reference so that term functions reading ``sensor.data.*`` / ``command_manager`` keep working.
"""

from __future__ import annotations

import ctypes
import types

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


class ContactSensorState:
    def __init__(self, num_envs: int, num_bodies: int, history_length: int = 0, track_air_time: bool = False,
                 update_period: float = 0.0, force_threshold: float = 1.0, device="cuda:0"):
        N, B, H = num_envs, num_bodies, history_length
        self.num_envs, self.num_bodies, self.history_length = N, B, H
        self.cfg = types.SimpleNamespace(track_air_time=track_air_time, update_period=update_period,
                                         force_threshold=force_threshold, history_length=H)
        dev = torch.device(device)
        self.device = dev
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self._timestamp, self._timestamp_last_update = z(N), z(N)
        self._is_outdated = torch.ones(N, dtype=torch.bool, device=dev)  # sensor_base.py:_initialize_impl
        d = types.SimpleNamespace()
        d.net_forces_w = z(N, B, 3)
        d.net_forces_w_history = z(N, max(H, 1), B, 3)
        d.last_air_time, d.current_air_time = z(N, B), z(N, B)
        d.last_contact_time, d.current_contact_time = z(N, B), z(N, B)
        self.data = d

    def update(self, new_net_forces_w: torch.Tensor, dt: float):
        """``SensorBase.update(dt)`` with PhysX's ``get_net_contact_forces`` result passed in as ``(N,B,3)``."""
        d = self.data
        f = new_net_forces_w.reshape(self.num_envs, self.num_bodies, 3).contiguous()
        H = self.history_length
        check(lib().imx_contact_sensor_update(
            self.num_envs, self.num_bodies, H, f.data_ptr(), float(dt), float(self.cfg.update_period),
            float(self.cfg.force_threshold), int(self.cfg.track_air_time), self._timestamp.data_ptr(),
            self._timestamp_last_update.data_ptr(), self._is_outdated.data_ptr(), d.net_forces_w.data_ptr(),
            d.net_forces_w_history.data_ptr() if H > 0 else None, d.last_air_time.data_ptr(), d.current_air_time.data_ptr(),
            d.last_contact_time.data_ptr(), d.current_contact_time.data_ptr(), _lib.current_stream(self.device)))
        if H == 0:  # contact_sensor.py:302: history is a view of the current forces
            d.net_forces_w_history = d.net_forces_w.unsqueeze(1)

    def reset(self, env_ids=None):
        """contact_sensor.py:143-165 + sensor_base.py:182-194"""
        ids = slice(None) if env_ids is None else env_ids
        self._timestamp[ids] = 0.0
        self._timestamp_last_update[ids] = 0.0
        self._is_outdated[ids] = True
        d = self.data
        d.net_forces_w[ids] = 0.0
        d.net_forces_w_history[ids] = 0.0
        if self.cfg.track_air_time:
            d.current_air_time[ids] = 0.0
            d.last_air_time[ids] = 0.0
            d.current_contact_time[ids] = 0.0
            d.last_contact_time[ids] = 0.0

    def compute_first_contact(self, dt: float, abs_tol: float = 1.0e-8) -> torch.Tensor:
        """contact_sensor.py:176-210"""
        if not self.cfg.track_air_time:
            raise RuntimeError("The contact sensor is not configured to track contact time."
                               "Please enable the 'track_air_time' in the sensor configuration.")
        c = self.data.current_contact_time
        return (c > 0.0) * (c < (dt + abs_tol))


class UniformVelocityCommand:
    """``cfg``: dict / object with the fields of ``UniformVelocityCommandCfg`` (velocity_command_cfg.py)."""

    def __init__(self, cfg, num_envs: int, step_dt: float, device="cuda:0", seed: int = 0):
        get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        rng = get("ranges")
        rget = (lambda k: rng.get(k)) if isinstance(rng, dict) else (lambda k: getattr(rng, k))
        self.heading_command = bool(get("heading_command", False))
        heading = rget("heading")
        if self.heading_command and heading is None:
            raise ValueError("The velocity command has heading commands active (heading_command=True) but the "
                             "`ranges.heading` parameter is set to None.")
        heading = heading or (0.0, 0.0)
        rt = get("resampling_time_range")
        self._cfg15 = np.asarray([rt[0], rt[1], *rget("lin_vel_x"), *rget("lin_vel_y"), *rget("ang_vel_z"), *heading,
                                  get("rel_standing_envs", 0.0), get("rel_heading_envs", 1.0),
                                  get("heading_control_stiffness", 1.0), rt[1] / step_dt, 0.0], dtype=np.float32)
        N = num_envs
        dev = torch.device(device)
        self.num_envs, self.device, self.seed = N, dev, int(seed)
        self.vel_command_b = torch.zeros(N, 3, device=dev)
        self.heading_target = torch.zeros(N, device=dev)
        self.is_heading_env = torch.zeros(N, dtype=torch.bool, device=dev)
        self.is_standing_env = torch.zeros(N, dtype=torch.bool, device=dev)
        self.time_left = torch.zeros(N, device=dev)
        self.command_counter = torch.zeros(N, dtype=torch.long, device=dev)
        self.metrics = {"error_vel_xy": torch.zeros(N, device=dev), "error_vel_yaw": torch.zeros(N, device=dev)}
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)

    @property
    def command(self) -> torch.Tensor:
        return self.vel_command_b

    def compute(self, dt: float, root_quat_w, root_lin_vel_w, root_ang_vel_w, reset_mask=None, uniforms=None,
                do_compute: bool = True):
        """``reset(ids of reset_mask)`` then (``do_compute``) ``compute(dt)``; ``uniforms``: optional (2,N,7) parity samples."""
        self._step += 1
        check(lib().imx_velocity_command(
            self.num_envs, self._cfg15.ctypes.data, int(self.heading_command), float(dt), int(do_compute), root_quat_w.data_ptr(),
            root_lin_vel_w.data_ptr(), root_ang_vel_w.data_ptr(), _lib.ptr(reset_mask), _lib.ptr(uniforms), self.seed,
            self._step.data_ptr(), self.vel_command_b.data_ptr(), self.heading_target.data_ptr(),
            self.is_heading_env.data_ptr(), self.is_standing_env.data_ptr(), self.time_left.data_ptr(),
            self.command_counter.data_ptr(), self.metrics["error_vel_xy"].data_ptr(),
            self.metrics["error_vel_yaw"].data_ptr(), _lib.current_stream(self.device)))
        return self.vel_command_b


class UniformPoseCommand:
    """``cfg``: dict / object with the fields of ``UniformPoseCommandCfg`` (commands_cfg.py); ``robot``: a ``RobotSpec`` (or anything with
    ``body_names``) through which ``cfg.body_name`` is resolved as ``robot.find_bodies(cfg.body_name)[0][0]`` does (pose_command.py:58-59).

    The ``CommandTerm`` surface of the reference class: ``command`` (= ``pose_command_b``, (N, 7) position + w, x, y, z quaternion in the
    base frame), ``pose_command_w``, ``time_left``, ``command_counter`` and ``metrics`` (``position_error``, ``orientation_error``)."""

    def __init__(self, cfg, num_envs: int, step_dt: float, device="cuda:0", seed: int = 0, robot=None):
        from .robots import resolve_matching_names

        get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        rng = get("ranges")
        rget = (lambda k: rng.get(k)) if isinstance(rng, dict) else (lambda k: getattr(rng, k))
        if robot is None:
            raise ValueError("UniformPoseCommand needs robot= (its body names resolve cfg.body_name)")
        self.body_name = get("body_name")
        self.num_bodies = len(robot.body_names)
        self.body_idx = int(resolve_matching_names(self.body_name, list(robot.body_names))[0][0])
        self.make_quat_unique = bool(get("make_quat_unique", False))
        rt = get("resampling_time_range")
        self._cfg16 = np.asarray([rt[0], rt[1], *rget("pos_x"), *rget("pos_y"), *rget("pos_z"), *rget("roll"), *rget("pitch"),
                                  *rget("yaw"), 0.0, 0.0], dtype=np.float32)
        N = num_envs
        dev = torch.device(device)
        self.num_envs, self.device, self.seed, self.step_dt = N, dev, int(seed), float(step_dt)
        self.pose_command_b = torch.zeros(N, 7, device=dev)
        self.pose_command_b[:, 3] = 1.0  # pose_command.py:63-64
        self.pose_command_w = torch.zeros(N, 7, device=dev)
        self.time_left = torch.zeros(N, device=dev)
        self.command_counter = torch.zeros(N, dtype=torch.long, device=dev)
        self.metrics = {"position_error": torch.zeros(N, device=dev), "orientation_error": torch.zeros(N, device=dev)}
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)

    @property
    def command(self) -> torch.Tensor:
        return self.pose_command_b

    def compute(self, dt: float, root_pos_w, root_quat_w, body_pos_w, body_quat_w, reset_mask=None, uniforms=None,
                do_compute: bool = True):
        """``reset(ids of reset_mask)`` then (``do_compute``) ``compute(dt)``; ``body_pos_w`` (N, NB, 3) / ``body_quat_w`` (N, NB, 4);
        ``uniforms``: optional (2,N,7) parity samples."""
        N, NB = self.num_envs, self.num_bodies
        for name, t, shape in (("root_pos_w", root_pos_w, (N, 3)), ("root_quat_w", root_quat_w, (N, 4)),
                               ("body_pos_w", body_pos_w, (N, NB, 3)), ("body_quat_w", body_quat_w, (N, NB, 4))):
            if tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError(f"UniformPoseCommand.compute: {name} is {tuple(t.shape)} {t.dtype}, expected {shape} float32")
        if reset_mask is not None and reset_mask.numel() != N:
            raise ValueError(f"UniformPoseCommand.compute: reset_mask has {reset_mask.numel()} entries for {N} envs")
        if uniforms is not None and (tuple(uniforms.shape) != (2, N, 7) or uniforms.dtype != torch.float32):
            raise ValueError(f"UniformPoseCommand.compute: uniforms is {tuple(uniforms.shape)} {uniforms.dtype}, expected (2, {N}, 7) float32")
        self._step += 1
        check(lib().imx_pose_command(
            N, self._cfg16.ctypes.data, int(self.make_quat_unique), self.body_idx, NB, float(dt), int(do_compute),
            _lib.ptr(root_pos_w), _lib.ptr(root_quat_w), _lib.ptr(body_pos_w), _lib.ptr(body_quat_w), _lib.ptr(reset_mask),
            _lib.ptr(uniforms), self.seed, self._step.data_ptr(), self.pose_command_b.data_ptr(), self.pose_command_w.data_ptr(),
            self.time_left.data_ptr(), self.command_counter.data_ptr(), self.metrics["position_error"].data_ptr(),
            self.metrics["orientation_error"].data_ptr(), _lib.current_stream(self.device)))
        return self.pose_command_b


class UniformPose2dCommand:
    """``cfg``: dict / object with the fields of ``UniformPose2dCommandCfg`` (commands_cfg.py): ``resampling_time_range``,
    ``simple_heading``, ``ranges`` {pos_x, pos_y, heading}.  ``env_origins`` (N, 3) is ``scene.env_origins`` and ``default_root_z`` (a
    number or (N)) ``robot.data.default_root_state[:, 2]``; left None, an env that is handed the term (``command_term=``) fills in its
    own.  ``robot``: anything with ``data.root_pos_w`` / ``data.root_quat_w`` (or the two attributes themselves, as
    ``ArticulationRootState`` has them), read by ``reset`` / ``compute`` in stand-alone use.

    The ``CommandTerm`` surface of the reference class (pose_2d_command.py:26-143): ``command`` (N, 4) = ``pos_command_b`` +
    ``heading_command_b`` (views of it), ``pos_command_w``, ``heading_command_w``, ``time_left``, ``command_counter`` and ``metrics``.
    The metrics follow the reference to the letter: the constructor creates ``error_pos`` and ``error_heading``, ``_update_metrics``
    writes ``error_pos_2d`` -- that key exists only after the first compute -- and ``error_pos`` stays zero for ever."""

    kind = 0

    def __init__(self, cfg, num_envs: int, step_dt: float, device="cuda:0", seed: int = 0, robot=None, env_origins=None,
                 default_root_z=None):
        get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        rng = get("ranges")
        rget = (lambda k, d=None: rng.get(k, d)) if isinstance(rng, dict) else (lambda k, d=None: getattr(rng, k, d))
        self.simple_heading = bool(get("simple_heading", False))
        rt = get("resampling_time_range")
        if not float(rt[1]) > 0.0:
            raise ValueError(f"{type(self).__name__}: resampling_time_range[1] must be positive (it is {rt[1]})")
        pos_x, pos_y, heading = rget("pos_x") or (0.0, 0.0), rget("pos_y") or (0.0, 0.0), rget("heading")
        if heading is None:
            if not self.simple_heading:
                raise ValueError(f"{type(self).__name__}: simple_heading is off but `ranges.heading` is None")
            heading = (0.0, 0.0)
        if self.kind == 0 and (rget("pos_x") is None or rget("pos_y") is None):
            raise ValueError("UniformPose2dCommand: `ranges.pos_x` and `ranges.pos_y` are needed")
        self._cfg8 = np.asarray([rt[0], rt[1], *pos_x, *pos_y, *heading], dtype=np.float32)
        N = num_envs
        dev = torch.device(device)
        self.num_envs, self.device, self.seed, self.step_dt, self.robot = N, dev, int(seed), float(step_dt), robot
        self.env_origins_given, self.default_root_z_given = env_origins is not None, default_root_z is not None
        self.env_origins = torch.zeros(N, 3, device=dev)
        if env_origins is not None:
            if tuple(env_origins.shape) != (N, 3):
                raise ValueError(f"{type(self).__name__}: env_origins is {tuple(env_origins.shape)}, expected ({N}, 3)")
            self.env_origins.copy_(env_origins)
        self.default_root_z = torch.zeros(N, device=dev)
        if default_root_z is not None:
            self.default_root_z.copy_(torch.as_tensor(default_root_z, dtype=torch.float32).expand(N))
        self._command = torch.zeros(N, 4, device=dev)
        self.pos_command_b, self.heading_command_b = self._command[:, :3], self._command[:, 3]
        self.pos_command_w = torch.zeros(N, 3, device=dev)
        self.heading_command_w = torch.zeros(N, device=dev)
        self.time_left = torch.zeros(N, device=dev)
        self.command_counter = torch.zeros(N, dtype=torch.long, device=dev)
        self.metrics = {"error_pos": torch.zeros(N, device=dev), "error_heading": torch.zeros(N, device=dev)}
        self._error_pos_2d = torch.zeros(N, device=dev)  # metrics["error_pos_2d"] from the first compute on
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)
        self._struct = None

    @property
    def command(self) -> torch.Tensor:
        return self._command

    def struct(self, uniforms=None, patch_ids=None) -> "_lib.ImxPose2dCommand":
        """The term as ``imx_pose2d_command`` / ``imx_reset_orchestrate_pose2d`` take it (it points at the term's own tensors)."""
        p = _lib.ptr
        c = _lib.ImxPose2dCommand(kind=self.kind, simple_heading=int(self.simple_heading), env_origins_d=p(self.env_origins),
                                  default_root_z_d=p(self.default_root_z), uniforms_d=p(uniforms), patch_ids_d=p(patch_ids),
                                  command_d=p(self._command), pos_command_w_d=p(self.pos_command_w),
                                  heading_command_w_d=p(self.heading_command_w), time_left_d=p(self.time_left),
                                  command_counter_d=p(self.command_counter), metric_error_pos_2d_d=p(self._error_pos_2d),
                                  metric_error_heading_d=p(self.metrics["error_heading"]))
        for k, v in enumerate(self._cfg8):
            c.cfg[k] = float(v)
        return c

    def mark_computed(self):
        """After a launch that ran ``compute``: ``_update_metrics`` has written ``error_pos_2d`` (pose_2d_command.py:84)."""
        self.metrics.setdefault("error_pos_2d", self._error_pos_2d)

    def _root(self, root_pos_w, root_quat_w):
        if root_pos_w is None or root_quat_w is None:
            if self.robot is None:
                raise ValueError(f"{type(self).__name__}: pass root_pos_w / root_quat_w or build the term with robot=")
            data = getattr(self.robot, "data", self.robot)
            root_pos_w, root_quat_w = data.root_pos_w, data.root_quat_w
        N = self.num_envs
        for name, t, shape in (("root_pos_w", root_pos_w, (N, 3)), ("root_quat_w", root_quat_w, (N, 4))):
            if tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError(f"{type(self).__name__}: {name} is {tuple(t.shape)} {t.dtype}, expected {shape} float32")
        return root_pos_w, root_quat_w

    def _launch(self, dt, do_compute, reset_mask, uniforms, patch_ids, root_pos_w, root_quat_w):
        N = self.num_envs
        root_pos_w, root_quat_w = self._root(root_pos_w, root_quat_w)
        if reset_mask is not None and (reset_mask.numel() != N or reset_mask.element_size() != 1):
            raise ValueError(f"{type(self).__name__}: reset_mask must hold {N} one-byte entries")
        if uniforms is not None and (tuple(uniforms.shape) != (2, N, 4) or uniforms.dtype != torch.float32):
            raise ValueError(f"{type(self).__name__}: uniforms is {tuple(uniforms.shape)} {uniforms.dtype}, expected (2, {N}, 4) float32")
        if patch_ids is not None and (tuple(patch_ids.shape) != (2, N) or patch_ids.dtype != torch.int64):
            raise ValueError(f"{type(self).__name__}: patch_ids is {tuple(patch_ids.shape)} {patch_ids.dtype}, expected (2, {N}) int64")
        self._step += 1
        if self._struct is None:  # (the term's own tensors never move: built once, the draw tables re-pointed per call)
            self._struct = self.struct()
        c = self._struct
        c.uniforms_d, c.patch_ids_d = _lib.ptr(uniforms), _lib.ptr(patch_ids)
        check(lib().imx_pose2d_command(N, ctypes.byref(c), float(dt), int(do_compute), _lib.ptr(root_pos_w), _lib.ptr(root_quat_w),
                                       _lib.ptr(reset_mask), self.seed, self._step.data_ptr(), _lib.current_stream(self.device)))
        if do_compute:
            self.mark_computed()

    def reset(self, env_ids=None, uniforms=None, patch_ids=None, root_pos_w=None, root_quat_w=None) -> dict:
        """``CommandTerm.reset(env_ids)`` (command_manager.py:120-149): returns the metrics' means over ``env_ids`` as they stood."""
        ids = slice(None) if env_ids is None else env_ids
        log = {k: float(torch.mean(v[ids])) for k, v in self.metrics.items()}
        mask = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        mask[ids] = True
        self._launch(0.0, False, mask, uniforms, patch_ids, root_pos_w, root_quat_w)
        return log

    def compute(self, dt: float, reset_mask=None, uniforms=None, patch_ids=None, root_pos_w=None, root_quat_w=None, do_compute: bool = True):
        """``reset(ids of reset_mask)`` then (``do_compute``) ``CommandTerm.compute(dt)`` in ONE launch; ``uniforms``: optional (2, N, 4)
        parity samples, ``patch_ids``: optional (2, N) int64 patch draws of the terrain-based class."""
        self._launch(dt, do_compute, reset_mask, uniforms, patch_ids, root_pos_w, root_quat_w)
        return self._command


class TerrainBasedPose2dCommand(UniformPose2dCommand):
    """``TerrainBasedPose2dCommand`` (pose_2d_command.py:146-203): the position is one of the P valid patches ``valid_targets`` (L, T, P, 3)
    (``terrain.flat_patches["target"]``) of the env's terrain cell (``terrain_levels``, ``terrain_types``: (N) int64), at the default
    root height above it."""

    kind = 1

    def __init__(self, cfg, num_envs: int, step_dt: float, device="cuda:0", seed: int = 0, robot=None, env_origins=None,
                 default_root_z=None, valid_targets=None, terrain_levels=None, terrain_types=None):
        super().__init__(cfg, num_envs, step_dt, device, seed, robot, env_origins, default_root_z)
        if valid_targets is None or terrain_levels is None or terrain_types is None:
            raise ValueError("TerrainBasedPose2dCommand needs valid_targets=, terrain_levels= and terrain_types=")
        if valid_targets.dim() != 4 or valid_targets.shape[-1] != 3 or 0 in valid_targets.shape:
            raise ValueError(f"TerrainBasedPose2dCommand: valid_targets is {tuple(valid_targets.shape)}, expected (L, T, P, 3)")
        L, T = valid_targets.shape[:2]
        for name, t, n in (("terrain_levels", terrain_levels, L), ("terrain_types", terrain_types, T)):
            if tuple(t.shape) != (num_envs,) or t.dtype != torch.int64:
                raise ValueError(f"TerrainBasedPose2dCommand: {name} is {tuple(t.shape)} {t.dtype}, expected ({num_envs},) int64")
            if int(t.min()) < 0 or int(t.max()) >= n:
                raise ValueError(f"TerrainBasedPose2dCommand: {name} has entries outside [0, {n})")
        self.valid_targets = valid_targets.to(self.device, torch.float32).contiguous()
        self.terrain_levels, self.terrain_types = terrain_levels.to(self.device).contiguous(), terrain_types.to(self.device).contiguous()

    def struct(self, uniforms=None, patch_ids=None):
        c = super().struct(uniforms, patch_ids)
        c.valid_targets_d, c.terrain_levels_d, c.terrain_types_d = _lib.ptr(self.valid_targets), _lib.ptr(self.terrain_levels), _lib.ptr(self.terrain_types)
        c.num_levels, c.num_types, c.num_patches = (int(x) for x in self.valid_targets.shape[:3])
        return c


class InHandReOrientationCommand:
    """``InHandReOrientationCommand`` (isaaclab_tasks .../manipulation/inhand/mdp/commands/orientation_command.py:22-124) as a stand-alone
    producer: ``k_inhand_command`` runs ``CommandTerm.reset`` on a mask and / or ``CommandTerm.compute(dt)`` in one launch.  No env runs
    it yet (the orchestration launch does not know the term): an env on the in-hand task takes its command from the state feed.

    ``cfg``: dict / object with the fields of ``InHandReOrientationCommandCfg`` (commands_cfg.py:19-71): ``resampling_time_range``,
    ``init_pos_offset``, ``make_quat_unique``, ``orientation_success_threshold``, ``update_goal_on_success``.  ``env_origins`` (N, 3) is
    ``scene.env_origins``, ``default_object_pos`` (3 numbers or (N, 3)) ``object.data.default_root_state[:, :3]``; both are fixed at
    construction, as in the reference (:43-45).

    The ``CommandTerm`` surface of the reference class: ``command`` (N, 7) = ``pos_command_e`` + ``quat_command_w`` (views of it),
    ``pos_command_w``, ``time_left``, ``command_counter`` and ``metrics`` with ``orientation_error``, ``position_error``,
    ``consecutive_success`` in the reference's order."""

    def __init__(self, cfg, num_envs: int, step_dt: float, device="cuda:0", seed: int = 0, env_origins=None, default_object_pos=None):
        get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        rt = get("resampling_time_range", (1.0e6, 1.0e6))
        if not float(rt[1]) > 0.0 or float(rt[0]) > float(rt[1]):
            raise ValueError(f"InHandReOrientationCommand: resampling_time_range {tuple(rt)} must be ordered and its upper end positive")
        for key in ("make_quat_unique", "orientation_success_threshold", "update_goal_on_success"):  # (MISSING fields of the configclass)
            if get(key) is None:
                raise ValueError(f"InHandReOrientationCommand: the cfg has no '{key}'")
        if env_origins is None or default_object_pos is None:
            raise ValueError("InHandReOrientationCommand needs env_origins= and default_object_pos= (both are fixed at construction)")
        N, dev = num_envs, torch.device(device)
        self.num_envs, self.device, self.seed, self.step_dt = N, dev, int(seed), float(step_dt)
        self.make_quat_unique, self.update_goal_on_success = bool(get("make_quat_unique")), bool(get("update_goal_on_success"))
        self.orientation_success_threshold = float(get("orientation_success_threshold"))
        self._cfg4 = np.asarray([rt[0], rt[1], self.orientation_success_threshold, 0.0], dtype=np.float32)
        if tuple(env_origins.shape) != (N, 3):
            raise ValueError(f"InHandReOrientationCommand: env_origins is {tuple(env_origins.shape)}, expected ({N}, 3)")
        default = torch.as_tensor(default_object_pos, dtype=torch.float32).to(dev)
        if tuple(default.shape) not in ((3,), (N, 3)):
            raise ValueError(f"InHandReOrientationCommand: default_object_pos is {tuple(default.shape)}, expected (3,) or ({N}, 3)")
        self._command = torch.zeros(N, 7, device=dev)
        self.pos_command_e, self.quat_command_w = self._command[:, :3], self._command[:, 3:7]
        self.pos_command_e.copy_(default.expand(N, 3) + torch.tensor(get("init_pos_offset", (0.0, 0.0, 0.0)), dtype=torch.float32, device=dev))
        self.pos_command_w = (self.pos_command_e + env_origins.to(dev, torch.float32)).contiguous()
        self.quat_command_w[:, 0] = 1.0
        self.time_left = torch.zeros(N, device=dev)
        self.command_counter = torch.zeros(N, dtype=torch.long, device=dev)
        self.metrics = {k: torch.zeros(N, device=dev) for k in ("orientation_error", "position_error", "consecutive_success")}
        self.log_part = torch.zeros((N + 63) // 64, 4, device=dev)  # per 64 envs: the reset envs' metric sums before the reset, their count
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)
        self._struct = None

    @property
    def command(self) -> torch.Tensor:
        return self._command

    def struct(self) -> "_lib.ImxInhandCommand":
        """The term as ``imx_inhand_command`` takes it (it points at the term's own tensors; the per-call pointers are NULL)."""
        p = _lib.ptr
        c = _lib.ImxInhandCommand(make_quat_unique=int(self.make_quat_unique), update_goal_on_success=int(self.update_goal_on_success),
                                  pos_command_w_d=p(self.pos_command_w), seed=self.seed, step_counter_d=self._step.data_ptr(),
                                  command_d=p(self._command), time_left_d=p(self.time_left), command_counter_d=p(self.command_counter),
                                  metric_orientation_error_d=p(self.metrics["orientation_error"]),
                                  metric_position_error_d=p(self.metrics["position_error"]),
                                  metric_consecutive_success_d=p(self.metrics["consecutive_success"]), log_part_d=p(self.log_part))
        for k, v in enumerate(self._cfg4):
            c.cfg[k] = float(v)
        return c

    def _launch(self, dt, do_compute, reset_mask, uniforms, object_root_pos_w, object_root_quat_w):
        N = self.num_envs
        for name, t, shape in (("object_root_pos_w", object_root_pos_w, (N, 3)), ("object_root_quat_w", object_root_quat_w, (N, 4))):
            if t is None and not do_compute:
                continue
            if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device:
                raise ValueError(f"InHandReOrientationCommand: {name} must be {shape} float32 on {self.device}")
        if reset_mask is not None and (reset_mask.numel() != N or reset_mask.element_size() != 1 or reset_mask.device != self.device):
            raise ValueError(f"InHandReOrientationCommand: reset_mask must hold {N} one-byte entries on {self.device}")
        if uniforms is not None and (tuple(uniforms.shape) != (3, N, 3) or uniforms.dtype != torch.float32 or uniforms.device != self.device):
            raise ValueError(f"InHandReOrientationCommand: uniforms must be (3, {N}, 3) float32 on {self.device}")
        self._step += 1
        if self._struct is None:  # (the term's own tensors never move: built once, the per-call pointers re-pointed)
            self._struct = self.struct()
        c = self._struct
        c.object_root_pos_w_d, c.object_root_quat_w_d = _lib.ptr(object_root_pos_w), _lib.ptr(object_root_quat_w)
        c.reset_mask_d, c.uniforms_d = _lib.ptr(reset_mask), _lib.ptr(uniforms)
        check(lib().imx_inhand_command(ctypes.byref(c), N, float(dt), int(bool(do_compute)), _lib.current_stream(self.device)))

    def reset(self, env_ids=None, uniforms=None, object_root_pos_w=None, object_root_quat_w=None) -> dict:
        """``CommandTerm.reset(env_ids)`` (command_manager.py:120-149): returns the metrics' means over ``env_ids`` as they stood."""
        ids = slice(None) if env_ids is None else env_ids
        log = {k: float(torch.mean(v[ids])) for k, v in self.metrics.items()}
        mask = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        mask[ids] = True
        self._launch(0.0, False, mask, uniforms, object_root_pos_w, object_root_quat_w)
        return log

    def compute(self, dt: float, object_root_pos_w, object_root_quat_w, reset_mask=None, uniforms=None):
        """``reset(ids of reset_mask)`` then ``CommandTerm.compute(dt)`` in ONE launch on the object's root pose; ``uniforms``: optional
        (3, N, 3) parity samples in [0, 1) -- {time_left, rand_floats[:, 0], rand_floats[:, 1]} of the reset's, the timer's and the
        reached goal's resampling."""
        self._launch(dt, True, reset_mask, uniforms, object_root_pos_w, object_root_quat_w)
        return self._command


class ArticulationRootState:
    """``ArticulationData`` root state + ``joint_acc`` from PhysX-layout tensors (reference
    isaaclab/assets/articulation/articulation_data.py:365-380,546-556), SURVEY 8f row 4.

    ``update(root_transforms (N,7 pos+quat XYZW), root_velocities (N,6), dof_velocities (N,J), dt)`` fills
    ``root_pos_w, root_quat_w (WXYZ), root_lin_vel_w, root_ang_vel_w, joint_vel, joint_acc``.
    """

    def __init__(self, num_envs: int, num_joints: int, device="cuda:0", initial_joint_vel: torch.Tensor | None = None):
        N, J = num_envs, num_joints
        dev = torch.device(device)
        self.num_envs, self.num_joints, self.device = N, J, dev
        self.root_pos_w = torch.zeros(N, 3, device=dev)
        self.root_quat_w = torch.zeros(N, 4, device=dev)
        self.root_lin_vel_w = torch.zeros(N, 3, device=dev)
        self.root_ang_vel_w = torch.zeros(N, 3, device=dev)
        self.joint_acc = torch.zeros(N, J, device=dev)
        self._previous_joint_vel = torch.zeros(N, J, device=dev) if initial_joint_vel is None else initial_joint_vel.clone()
        self.joint_vel = self._previous_joint_vel
        # TimestampedBuffer semantics (isaaclab/utils/buffers/timestamped_buffer.py): buffers start at timestamp -1.0, so
        # the reference's first finite difference divides by (dt + 1.0) -- reproduced, not "fixed"
        self._sim_timestamp = 0.0
        self._joint_acc_timestamp = -1.0

    def update(self, root_transforms, root_velocities, dof_velocities, dt: float):
        self._sim_timestamp += dt
        elapsed = self._sim_timestamp - self._joint_acc_timestamp
        self._joint_acc_timestamp = self._sim_timestamp
        check(lib().imx_articulation_update(
            self.num_envs, self.num_joints, root_transforms.data_ptr(), root_velocities.data_ptr(), dof_velocities.data_ptr(),
            float(elapsed), self.root_pos_w.data_ptr(), self.root_quat_w.data_ptr(), self.root_lin_vel_w.data_ptr(),
            self.root_ang_vel_w.data_ptr(), self._previous_joint_vel.data_ptr(), self.joint_acc.data_ptr(),
            _lib.current_stream(self.device)))
        self.joint_vel = dof_velocities


class PDActuator:
    """``IdealPDActuator`` / ``ImplicitActuator`` (reporting) / ``DCMotor`` ``.compute`` on libimx
    (reference isaaclab/actuators/actuator_pd.py:115-145,184-199,264-286): ``computed_effort`` and ``applied_effort`` (N,J)."""

    def __init__(self, stiffness, damping, effort_limit, velocity_limit=None, saturation_effort: float | None = None):
        self.stiffness, self.damping, self.effort_limit = stiffness.contiguous(), damping.contiguous(), effort_limit.contiguous()
        self.velocity_limit = None if velocity_limit is None else velocity_limit.contiguous()
        self.saturation_effort = saturation_effort
        if stiffness.device.type != "cuda":
            raise RuntimeError("PDActuator needs a GPU: libimx has no CPU path")
        self.computed_effort = torch.zeros_like(self.stiffness)
        self.applied_effort = torch.zeros_like(self.stiffness)

    def compute(self, joint_pos_target, joint_pos, joint_vel, joint_vel_target=None, effort_ff=None):
        N, J = self.stiffness.shape
        p = _lib.ptr
        dc = self.saturation_effort is not None
        check(lib().imx_actuator_pd(N, J, int(dc), float(self.saturation_effort or 0.0), p(joint_pos_target), p(joint_vel_target),
                                    p(effort_ff), p(joint_pos), p(joint_vel), p(self.stiffness), p(self.damping), p(self.effort_limit),
                                    p(self.velocity_limit), p(self.computed_effort), p(self.applied_effort),
                                    _lib.current_stream(self.stiffness.device)))
        return self.applied_effort


class DelayedPDActuator:
    """``DelayedPDActuator`` / ``RemotizedPDActuator`` ``.reset`` + ``.compute`` on libimx (reference
    isaaclab/actuators/actuator_pd.py:289-412): the position / velocity / feed-forward commands pass through one shared delay ring
    with a per-env lag re-drawn at reset, then the PD law; ``joint_parameter_lookup`` (K,3) adds the remotized angle-dependent
    torque limit.  One launch per physics step, no host sync (the reference's ``CircularBuffer.append`` has a ``.tolist()``)."""

    def __init__(self, stiffness, damping, min_delay: int, max_delay: int, effort_limit=None, joint_parameter_lookup=None):
        if stiffness.device.type != "cuda":
            raise RuntimeError("DelayedPDActuator needs a GPU: libimx has no CPU path")
        if not 0 <= int(min_delay) <= int(max_delay):
            raise ValueError(f"The minimum time lag cannot be negative or above the maximum. Received: {min_delay}, {max_delay}")
        dev = stiffness.device
        N, J = stiffness.shape
        self.stiffness, self.damping = stiffness.contiguous(), damping.contiguous()
        self.min_delay, self.max_delay = int(min_delay), int(max_delay)
        self.lookup = None
        if joint_parameter_lookup is not None:  # RemotizedPDActuator removes the box limits (:373-380)
            self.lookup = torch.as_tensor(joint_parameter_lookup, dtype=torch.float32, device=dev).contiguous()
            x = self.lookup[:, 0]
            if self.lookup.numel() == 0:
                raise ValueError("Input tensor x is empty!")
            if bool(torch.any(x[1:] < x[:-1])):
                raise ValueError("Input tensor x is not sorted in ascending order!")
            effort_limit = None
        self.effort_limit = None if effort_limit is None else effort_limit.contiguous()
        self.ring = torch.zeros(self.max_delay + 1, N, 3, J, device=dev)
        self.time_lags = torch.zeros(N, dtype=torch.int32, device=dev)
        self.reset_step = torch.zeros(N, dtype=torch.int64, device=dev)
        self.step = 0
        self.computed_effort = torch.zeros_like(self.stiffness)
        self.applied_effort = torch.zeros_like(self.stiffness)

    def reset(self, env_ids=None, time_lags=None):
        """New random lag in [min_delay, max_delay] for ``env_ids`` (``time_lags`` overrides the draw: parity tests) and an empty
        delay line: the next sample fills it."""
        N = self.stiffness.shape[0]
        ids = slice(None) if env_ids is None else env_ids
        n = N if env_ids is None else len(env_ids)
        if time_lags is None:
            time_lags = torch.randint(self.min_delay, self.max_delay + 1, (n,), dtype=torch.int32, device=self.stiffness.device)
        self.time_lags[ids] = time_lags.to(self.time_lags)
        self.reset_step[ids] = self.step

    def compute(self, joint_pos_target, joint_pos, joint_vel, joint_vel_target=None, effort_ff=None):
        N, J = self.stiffness.shape
        p = _lib.ptr
        check(lib().imx_actuator_delayed_pd(N, J, self.max_delay, self.step, p(self.time_lags), p(self.reset_step), p(self.ring),
                                            p(joint_pos_target), p(joint_vel_target), p(effort_ff), p(joint_pos), p(joint_vel),
                                            p(self.stiffness), p(self.damping), p(self.effort_limit), p(self.lookup),
                                            0 if self.lookup is None else self.lookup.shape[0], p(self.computed_effort),
                                            p(self.applied_effort), _lib.current_stream(self.stiffness.device)))
        self.step += 1
        return self.applied_effort


_NET_ACT = {"identity": 0, None: 0, "softsign": 1, "tanh": 2, "relu": 3, "elu": 4}


def _pack_dense(layers) -> tuple[list[torch.Tensor], list[int]]:
    """[(weight (out,in), bias (out)), ...] -> flat pieces + widths."""
    pieces, widths = [], []
    for w, b in layers:
        pieces += [w.detach().float().reshape(-1), b.detach().float().reshape(-1)]
        widths.append(int(w.shape[0]))
    return pieces, widths


def _dense_from_module(net, skip_prefix: str | None) -> list:
    """The Linear layers of a (TorchScript) network in definition order: every 2-D ``*.weight`` with its ``*.bias``."""
    sd = net.state_dict()
    layers = []
    for name, w in sd.items():
        if name.endswith("weight") and w.dim() == 2 and not (skip_prefix and name.startswith(skip_prefix)):
            layers.append((w, sd[name[: -len("weight")] + "bias"]))
    if not layers:
        raise ValueError("no Linear layers found in the actuator network")
    return layers


class ActuatorNetLSTM:
    """``ActuatorNetLSTM.reset`` / ``.compute`` on libimx (reference isaaclab/actuators/actuator_net.py:29-104; the ANYdrive 3 actuator
    of ANYmal-B/C, isaaclab_assets/robots/anymal.py:45-51): every (env, joint) sample runs through the LSTM stack and the dense head
    in one launch; hidden and cell states live in ``sea_hidden_state`` / ``sea_cell_state`` (num_layers, N*J, H) like the reference's.

    ``network``: the reference's TorchScript module (``network.lstm`` = ``nn.LSTM(2, H, L, batch_first=True)``, the remaining Linear
    layers = the head, ``head_activation`` between them) or ``None`` with ``lstm_layers`` = [(w_ih, w_hh, b_ih, b_hh), ...] and
    ``head`` = [(weight, bias), ...] given directly."""

    def __init__(self, num_envs: int, num_joints: int, effort_limit, velocity_limit, saturation_effort: float, network=None,
                 lstm_layers=None, head=None, head_activation: str | None = "softsign", device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ActuatorNetLSTM needs a GPU: libimx has no CPU path")
        if network is not None:
            sd = network.lstm.state_dict()
            L = len(sd) // 4  # actuator_net.py:54
            lstm_layers = [(sd[f"weight_ih_l{k}"], sd[f"weight_hh_l{k}"], sd[f"bias_ih_l{k}"], sd[f"bias_hh_l{k}"]) for k in range(L)]
            head = _dense_from_module(network, "lstm.")
        if not lstm_layers or not head:
            raise ValueError("ActuatorNetLSTM needs a network (or lstm_layers and head)")
        self.num_envs, self.num_joints = int(num_envs), int(num_joints)
        self.hidden_dim = int(lstm_layers[0][1].shape[1])
        self.num_layers = len(lstm_layers)
        pieces = []
        for w_ih, w_hh, b_ih, b_hh in lstm_layers:
            pieces += [t.detach().float().reshape(-1) for t in (w_ih, w_hh, b_ih, b_hh)]
        hp, self._dense_out = _pack_dense(head)
        self._weights = torch.cat(pieces + hp).to(dev).contiguous()
        self._dense_arr = (ctypes.c_int32 * len(self._dense_out))(*self._dense_out)
        self._act = _NET_ACT[head_activation]
        full = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev).expand(self.num_envs, self.num_joints).contiguous()  # noqa: E731
        self.effort_limit, self.velocity_limit = full(effort_limit), full(velocity_limit)
        self.saturation_effort = float(saturation_effort)
        n = self.num_envs * self.num_joints
        self.sea_hidden_state = torch.zeros(self.num_layers, n, self.hidden_dim, device=dev)
        self.sea_cell_state = torch.zeros(self.num_layers, n, self.hidden_dim, device=dev)
        shape = (self.num_layers, self.num_envs, self.num_joints, self.hidden_dim)
        self.sea_hidden_state_per_env = self.sea_hidden_state.view(shape)
        self.sea_cell_state_per_env = self.sea_cell_state.view(shape)
        self.computed_effort = torch.zeros(self.num_envs, self.num_joints, device=dev)
        self.applied_effort = torch.zeros(self.num_envs, self.num_joints, device=dev)

    def reset(self, env_ids=None):
        ids = slice(None) if env_ids is None else env_ids
        self.sea_hidden_state_per_env[:, ids] = 0.0
        self.sea_cell_state_per_env[:, ids] = 0.0

    def compute(self, joint_pos_target, joint_pos, joint_vel):
        p = _lib.ptr
        check(lib().imx_actuator_net_lstm(self.num_envs, self.num_joints, self.num_layers, self.hidden_dim, len(self._dense_out),
                                          self._dense_arr, self._act, p(self._weights), self._weights.numel(), p(joint_pos_target),
                                          p(joint_pos), p(joint_vel), p(self.sea_hidden_state), p(self.sea_cell_state),
                                          self.saturation_effort, p(self.effort_limit), p(self.velocity_limit), p(self.computed_effort),
                                          p(self.applied_effort), _lib.current_stream(self._weights.device)))
        return self.applied_effort


class ActuatorNetMLP:
    """``ActuatorNetMLP.reset`` / ``.compute`` on libimx (reference isaaclab/actuators/actuator_net.py:107-195): the position-error and
    velocity histories (N, history, J) are rolled and topped up, the ``input_idx`` entries of both scaled and stacked per
    (env, joint) sample, the dense network evaluated and its torque clipped by the DC-motor model -- one launch.
    ``network``: the TorchScript module (its Linear layers in order, ``activation`` between them) or ``None`` with ``layers`` given."""

    def __init__(self, num_envs: int, num_joints: int, effort_limit, velocity_limit, saturation_effort: float, input_idx, pos_scale: float,
                 vel_scale: float, torque_scale: float, input_order: str = "pos_vel", network=None, layers=None,
                 activation: str | None = "softsign", device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ActuatorNetMLP needs a GPU: libimx has no CPU path")
        if input_order not in ("pos_vel", "vel_pos"):  # actuator_net.py:186-189
            raise ValueError(f"Invalid input order for MLP actuator net: {input_order}. Must be 'pos_vel' or 'vel_pos'.")
        if network is not None:
            layers = _dense_from_module(network, None)
        if not layers:
            raise ValueError("ActuatorNetMLP needs a network (or layers)")
        self.num_envs, self.num_joints = int(num_envs), int(num_joints)
        self.input_idx = [int(i) for i in input_idx]
        self.history_length = max(self.input_idx) + 1  # :145
        pieces, self._dense_out = _pack_dense(layers)
        self._weights = torch.cat(pieces).to(dev).contiguous()
        self._dense_arr = (ctypes.c_int32 * len(self._dense_out))(*self._dense_out)
        self._act = _NET_ACT[activation]
        self._idx = torch.tensor(self.input_idx, dtype=torch.int32, device=dev)
        self.pos_scale, self.vel_scale, self.torque_scale = float(pos_scale), float(vel_scale), float(torque_scale)
        self._vel_first = int(input_order == "vel_pos")
        full = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev).expand(self.num_envs, self.num_joints).contiguous()  # noqa: E731
        self.effort_limit, self.velocity_limit = full(effort_limit), full(velocity_limit)
        self.saturation_effort = float(saturation_effort)
        self._joint_pos_error_history = torch.zeros(self.num_envs, self.history_length, self.num_joints, device=dev)
        self._joint_vel_history = torch.zeros(self.num_envs, self.history_length, self.num_joints, device=dev)
        self.computed_effort = torch.zeros(self.num_envs, self.num_joints, device=dev)
        self.applied_effort = torch.zeros(self.num_envs, self.num_joints, device=dev)

    def reset(self, env_ids=None):
        ids = slice(None) if env_ids is None else env_ids
        self._joint_pos_error_history[ids] = 0.0
        self._joint_vel_history[ids] = 0.0

    def compute(self, joint_pos_target, joint_pos, joint_vel):
        p = _lib.ptr
        check(lib().imx_actuator_net_mlp(self.num_envs, self.num_joints, len(self._dense_out), self._dense_arr, self._act, p(self._weights),
                                         self._weights.numel(), self.history_length, p(self._idx), len(self.input_idx), self.pos_scale,
                                         self.vel_scale, self.torque_scale, self._vel_first, p(joint_pos_target), p(joint_pos), p(joint_vel),
                                         p(self._joint_pos_error_history), p(self._joint_vel_history), self.saturation_effort,
                                         p(self.effort_limit), p(self.velocity_limit), p(self.computed_effort), p(self.applied_effort),
                                         _lib.current_stream(self._weights.device)))
        return self.applied_effort


class FrameTransformer:
    """``FrameTransformer`` (isaaclab/sensors/frame_transformer/frame_transformer.py:337-384): ``update`` fills the six
    ``FrameTransformerData`` tensors from the body poses of the articulation its frames sit on, in one launch (``imx_frame_transformer``,
    lane = (env, target frame)).

    ``cfg``: the scene entity's name in ``resolver`` (a ``robots.SceneEntityResolver`` that knows the sensor), or an already resolved
    ``robots.FrameTable``.  ``data``: ``source_pos_w`` (N, 3), ``source_quat_w`` (N, 4), ``target_pos_w`` / ``target_pos_source``
    (N, T, 3), ``target_quat_w`` / ``target_quat_source`` (N, T, 4) and ``target_frame_names``, as ``FrameTransformerData``.  ``asset``: 0
    = the frames sit on the robot, 1 = on the scene's second articulation (whose ``body_pos_w`` / ``body_quat_w`` ``update`` then takes)."""

    def __init__(self, cfg, resolver, num_envs: int, device="cuda:0"):
        table = resolver.frame_table(cfg) if isinstance(cfg, str) else cfg
        N, T, dev = int(num_envs), len(table.targets), torch.device(device)
        self.table, self.asset, self.num_envs, self.device = table, table.asset, N, dev
        words = np.zeros((1 + T, _lib.FRAME_WORDS), np.int32)
        for row, f in zip(words, [table.source] + list(table.targets)):
            w = f.words()
            row[:2] = w[:2]
            row[2:] = np.asarray(w[2:], np.float32).view(np.int32)
        self._frames_h = np.ascontiguousarray(words)
        self._frames_d = torch.from_numpy(self._frames_h).to(dev)
        z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        self.data = types.SimpleNamespace(source_pos_w=z(N, 3), source_quat_w=z(N, 4), target_pos_w=z(N, T, 3), target_quat_w=z(N, T, 4),
                                          target_pos_source=z(N, T, 3), target_quat_source=z(N, T, 4),
                                          target_frame_names=list(table.target_frame_names))

    def update(self, body_pos_w: torch.Tensor, body_quat_w: torch.Tensor):
        """One launch on ``body_pos_w`` (N, B, 3) / ``body_quat_w`` (N, B, 4) of the articulation the frames sit on; returns ``data``."""
        N, d = self.num_envs, self.data
        if body_pos_w.dim() != 3 or tuple(body_pos_w.shape) != (N, body_pos_w.shape[1], 3) or tuple(body_quat_w.shape) != (N, body_pos_w.shape[1], 4):
            raise ValueError(f"FrameTransformer '{self.table.entity}': body_pos_w / body_quat_w must be ({N}, B, 3) / ({N}, B, 4), got "
                             f"{tuple(body_pos_w.shape)} / {tuple(body_quat_w.shape)}")
        for t in (body_pos_w, body_quat_w):
            if t.dtype != torch.float32 or t.device != self.device:
                raise ValueError(f"FrameTransformer '{self.table.entity}': body poses must be float32 on {self.device}")
        p = _lib.ptr
        check(lib().imx_frame_transformer(N, len(self.table.targets), int(body_pos_w.shape[1]), p(body_pos_w), p(body_quat_w), p(self._frames_d),
                                          self._frames_h.ctypes.data, p(d.source_pos_w), p(d.source_quat_w), p(d.target_pos_w), p(d.target_quat_w),
                                          p(d.target_pos_source), p(d.target_quat_source), _lib.current_stream(self.device)))
        return d


def _cfg_field(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


class RayCaster:
    """``RayCaster`` (isaaclab/sensors/ray_caster/ray_caster.py under ``SensorBase``, sensors/sensor_base.py:182-205,287-296) with any of
    the ray patterns of ``plan.ray_pattern`` (grid, Bpearl, lidar) and the full orientation of the body it sits on, in one launch
    (``imx_ray_caster``): reset, clocks, and for the outdated envs the pose, the world rays, the cast through the z-pruned grid walk and
    the optional range image.

    ``cfg``: the ``RayCasterCfg`` as object or dict -- ``pattern_cfg``, ``offset.pos`` / ``.rot``, ``attach_yaw_only``, ``max_distance``,
    ``drift_range``, ``update_period``, ``mesh_prim_paths`` (at most one).  ``mesh``: the ``TerrainMesh`` the rays are cast against.
    ``keep_world_rays``: also store the world-frame starts and directions of the last cast (``ray_starts_w`` / ``ray_directions_w``).

    ``update(dt, body_pos_w, body_quat_w)`` is ``SensorBase.update``: without ``force_recompute`` only the clocks and flags advance;
    ``data`` refreshes the outdated envs lazily, from the poses given last, and has ``pos_w`` (N, 3), ``quat_w`` (N, 4) and ``ray_hits_w``
    (N, R, 3; +inf on a miss).  ``ranges(clip)`` is the (N, R) range image ``min(||ray_hits_w - pos_w||, clip)``."""

    def __init__(self, cfg, num_envs: int, device, mesh, seed: int = 0, keep_world_rays: bool = False):
        from .plan import ray_pattern

        pc = _cfg_field(cfg, "pattern_cfg")
        if pc is None:
            raise ValueError("RayCaster: cfg.pattern_cfg is missing")
        starts, dirs = ray_pattern(pc)  # (refuses the pinhole pattern by name)
        paths = _cfg_field(cfg, "mesh_prim_paths")
        if paths is not None and not isinstance(paths, str) and len(paths) != 1:
            raise NotImplementedError(f"RayCaster currently only supports one mesh prim. Received: {len(paths)}")  # ray_caster.py:153-156
        if mesh is None:
            raise NotImplementedError("RayCaster: the terrain has no mesh (a plane): the rays are cast against a TerrainMesh; a ground plane "
                                      "as an infinite mesh is not built")
        N, dev = int(num_envs), torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        off = _cfg_field(cfg, "offset") or {}
        off_pos = torch.tensor(list(_cfg_field(off, "pos", (0.0, 0.0, 0.0))), dtype=torch.float32)
        off_rot = torch.tensor(list(_cfg_field(off, "rot", (1.0, 0.0, 0.0, 0.0))), dtype=torch.float32)
        # _initialize_rays_impl (ray_caster.py:201-212): directions through quat_apply(offset.rot), starts + offset.pos, in fp32 on the host
        d = torch.from_numpy(np.ascontiguousarray(dirs, np.float32))
        xyz = off_rot[1:].repeat(len(d), 1)
        t = xyz.cross(d, dim=-1) * 2
        d = d + off_rot[0] * t + xyz.cross(t, dim=-1)
        s = torch.from_numpy(np.ascontiguousarray(starts, np.float32)) + off_pos
        self.num_envs, self.device, self.mesh, self.seed = N, dev, mesh, int(seed)
        self.num_rays = R = int(d.shape[0])
        self.ray_starts, self.ray_directions = s.contiguous().to(dev), d.contiguous().to(dev)  # (R, 3): every env has the same pattern
        dr = tuple(float(x) for x in _cfg_field(cfg, "drift_range", (0.0, 0.0)))
        self.cfg = types.SimpleNamespace(attach_yaw_only=bool(_cfg_field(cfg, "attach_yaw_only", False)),
                                         max_distance=float(_cfg_field(cfg, "max_distance", 1.0e6)), drift_range=dr,
                                         update_period=float(_cfg_field(cfg, "update_period", 0.0)), pattern_cfg=pc)
        if dr[0] > dr[1]:
            raise ValueError(f"RayCaster: drift_range {dr}: the lower bound exceeds the upper")
        z = lambda *sh, dtype=torch.float32: torch.zeros(*sh, dtype=dtype, device=dev)  # noqa: E731
        self._timestamp, self._timestamp_last_update = z(N), z(N)
        self._is_outdated = torch.ones(N, dtype=torch.bool, device=dev)  # sensor_base.py:_initialize_impl
        self.drift = z(N, 3)
        self._reset_count = z(N, dtype=torch.int32)
        self._all = torch.ones(N, dtype=torch.bool, device=dev)
        self._data = types.SimpleNamespace(pos_w=z(N, 3), quat_w=z(N, 4), ray_hits_w=z(N, R, 3))
        self._ranges = z(N, R)
        self.ray_starts_w = z(N, R, 3) if keep_world_rays else None
        self.ray_directions_w = z(N, R, 3) if keep_world_rays else None
        self._pose = None
        self.bounds_info = None
        if dev.type == "cuda":  # the walk's z-bounds, once per mesh (allocates and synchronises: here, not in a launch that may be captured)
            info = (ctypes.c_int64 * 4)()
            check(lib().imx_mesh_build_ray_bounds(mesh.handle, _lib.current_stream(dev), info))
            self.bounds_info = {"bytes": int(info[0]), "build_ns": int(info[1]), "cells": int(info[2]), "tiles": int(info[3])}
        p = _lib.ptr
        self._c = _lib.ImxRayCaster(num_rays=R, attach_yaw_only=int(self.cfg.attach_yaw_only), max_distance=self.cfg.max_distance,
                                    update_period=self.cfg.update_period, drift_lo=dr[0], drift_hi=dr[1], seed=self.seed & (2 ** 64 - 1),
                                    ray_starts_d=p(self.ray_starts), ray_directions_d=p(self.ray_directions), reset_count_d=p(self._reset_count),
                                    timestamp_d=p(self._timestamp), timestamp_last_update_d=p(self._timestamp_last_update),
                                    is_outdated_d=p(self._is_outdated), drift_d=p(self.drift), pos_w_d=p(self._data.pos_w),
                                    quat_w_d=p(self._data.quat_w), ray_hits_w_d=p(self._data.ray_hits_w),
                                    ray_starts_w_d=p(self.ray_starts_w), ray_directions_w_d=p(self.ray_directions_w))

    def _check_pose(self, body_pos_w, body_quat_w):
        N = self.num_envs
        if tuple(body_pos_w.shape) != (N, 3) or tuple(body_quat_w.shape) != (N, 4):
            raise ValueError(f"RayCaster: body_pos_w / body_quat_w must be ({N}, 3) / ({N}, 4), got {tuple(body_pos_w.shape)} / {tuple(body_quat_w.shape)}")
        for t in (body_pos_w, body_quat_w):
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"RayCaster: body poses must be contiguous float32 tensors on {self.device}")

    def _launch(self, dt=0.0, substeps=0, refresh=False, reset_mask=None, uniforms=None, range_clip=None):
        if self._pose is None:
            raise RuntimeError("RayCaster: no body pose yet: call update(dt, body_pos_w, body_quat_w) first")
        c = self._c
        c.dt, c.substeps, c.refresh = float(dt), int(substeps), int(bool(refresh))
        c.body_pos_w_d, c.body_quat_w_d = _lib.ptr(self._pose[0]), _lib.ptr(self._pose[1])
        c.reset_mask_d, c.uniforms_d = _lib.ptr(reset_mask), _lib.ptr(uniforms)
        c.ranges_d, c.range_clip = (_lib.ptr(self._ranges), float(range_clip)) if range_clip is not None else (None, 0.0)
        check(lib().imx_ray_caster(ctypes.byref(c), self.num_envs, self.mesh.handle, _lib.current_stream(self.device)))

    def _mask(self, env_ids):
        N = self.num_envs
        if env_ids is None or isinstance(env_ids, slice) and env_ids == slice(None):
            return self._all
        ids = torch.as_tensor(env_ids, device=self.device)
        if ids.dtype in (torch.bool, torch.uint8) and tuple(ids.shape) == (N,):
            return ids.contiguous()
        m = torch.zeros(N, dtype=torch.bool, device=self.device)
        m[ids.long()] = True
        return m

    def _uniforms(self, uniforms):
        if uniforms is None:
            return None
        if tuple(uniforms.shape) != (self.num_envs, 3) or uniforms.dtype != torch.float32 or uniforms.device != self.device:
            raise ValueError(f"RayCaster: uniforms must be a ({self.num_envs}, 3) float32 tensor on {self.device}")
        return uniforms.contiguous()

    def reset(self, env_ids=None, uniforms=None):
        """``SensorBase.reset`` + ``RayCaster.reset`` for ``env_ids`` (None = all; indices or an (N,) mask): clocks to zero, outdated, a new
        drift from the counter-based generator or from ``uniforms`` (N, 3) in [0, 1)."""
        if self._pose is None:  # (a reset before the first update reads no pose: the launch only needs valid pointers)
            self._pose = (self._data.pos_w, self._data.quat_w)
            try:
                self._launch(reset_mask=self._mask(env_ids), uniforms=self._uniforms(uniforms))
            finally:
                self._pose = None
            return
        self._launch(reset_mask=self._mask(env_ids), uniforms=self._uniforms(uniforms))

    def update(self, dt: float, body_pos_w: torch.Tensor, body_quat_w: torch.Tensor, force_recompute: bool = False, substeps: int = 1,
               reset_mask=None, uniforms=None):
        """``SensorBase.update(dt)``, ``substeps`` times, on the pose of the body the sensor sits on (kept by reference for ``data``);
        ``reset_mask`` (N,): those envs are reset first, in the same launch.  With ``force_recompute`` the outdated envs are refreshed."""
        self._check_pose(body_pos_w, body_quat_w)
        self._pose = (body_pos_w, body_quat_w)
        self._launch(dt=dt, substeps=substeps, refresh=force_recompute, reset_mask=None if reset_mask is None else self._mask(reset_mask),
                     uniforms=self._uniforms(uniforms))

    @property
    def data(self):
        """``SensorBase.data``: ``_update_outdated_buffers`` first (one launch; an env that is not outdated leaves it at once)."""
        self._launch(refresh=True)
        return self._data

    def ranges(self, range_clip: float) -> torch.Tensor:
        """(N, R) ``min(||ray_hits_w - pos_w||, range_clip)``, a miss = ``range_clip``, after the refresh of ``data`` (same launch)."""
        self._launch(refresh=True, range_clip=range_clip)
        return self._ranges


class Imu:
    """``Imu`` (isaaclab/sensors/imu/imu.py under ``SensorBase``, sensors/sensor_base.py:182-205,287-296) in one launch (``imx_imu``):
    reset, clocks, and for the outdated envs the sensor pose, the velocity carried from the body's centre of mass to the sensor, both
    accelerations by numerical differentiation and the four vectors in the sensor's frame.

    ``cfg``: the ``ImuCfg`` as object or dict -- ``offset.pos`` / ``.rot``, ``gravity_bias``, ``update_period``, ``history_length``
    (> 0 only makes every ``update`` recompute, as in ``SensorBase.update``).  ``body_index``: the sensor sits on column ``b`` of
    (N, B, .) inputs; None = (N, .) inputs.  ``com_pos_b``: the body's centre of mass in its link frame, (3,) or (N, 3); default zeros.

    ``update(dt, pos_w, quat_w, lin_vel_w, ang_vel_w)`` is ``Imu.update``: the link pose (quaternion w, x, y, z) and the velocities of
    the centre of mass, kept by reference for ``data`` and never written.  Without ``force_recompute`` only the clocks and flags advance;
    ``data`` refreshes the outdated envs lazily and has ``pos_w``, ``quat_w``, ``lin_vel_b``, ``ang_vel_b``, ``lin_acc_b``, ``ang_acc_b``.
    The reference's quirks are kept: the accelerations divide by the ``dt`` of the LAST ``update`` call whatever time has passed since
    the last refresh, and a reset zeroes ``quat_w`` and the four body-frame vectors but neither ``pos_w`` nor the previous velocities."""

    DATA_FIELDS = ("pos_w", "quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b")

    def __init__(self, cfg, num_envs: int, device, body_index: int | None = None, com_pos_b=None, name: str = "imu"):
        N, dev = int(num_envs), torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.name = str(name)
        if bool(_cfg_field(cfg, "debug_vis", False)):
            raise NotImplementedError(f"Imu '{self.name}': debug_vis=True: the acceleration markers are not drawn (no visualisation here)")
        off = _cfg_field(cfg, "offset") or {}
        pos = tuple(float(x) for x in _cfg_field(off, "pos", (0.0, 0.0, 0.0)))
        rot = tuple(float(x) for x in _cfg_field(off, "rot", (1.0, 0.0, 0.0, 0.0)))
        bias = tuple(float(x) for x in _cfg_field(cfg, "gravity_bias", (0.0, 0.0, 9.81)))
        if len(pos) != 3 or len(rot) != 4 or len(bias) != 3:
            raise ValueError(f"Imu '{self.name}': offset.pos / offset.rot / gravity_bias must have 3 / 4 / 3 components")
        period = float(_cfg_field(cfg, "update_period", 0.0))
        if period < 0.0:
            raise ValueError(f"Imu '{self.name}': update_period {period} is negative")
        if body_index is not None and int(body_index) < 0:
            raise ValueError(f"Imu '{self.name}': body_index {body_index} is negative")
        self.num_envs, self.device = N, dev
        self.body_index = None if body_index is None else int(body_index)
        self.cfg = types.SimpleNamespace(offset=types.SimpleNamespace(pos=pos, rot=rot), gravity_bias=bias, update_period=period,
                                         history_length=int(_cfg_field(cfg, "history_length", 0) or 0))
        self.com_pos_b = None
        if com_pos_b is not None:
            com = torch.as_tensor(com_pos_b, dtype=torch.float32)
            if tuple(com.shape) not in ((3,), (N, 3)):
                raise ValueError(f"Imu '{self.name}': com_pos_b must be (3,) or ({N}, 3), got {tuple(com.shape)}")
            self.com_pos_b = com.to(dev).contiguous()
        z = lambda *sh, dtype=torch.float32: torch.zeros(*sh, dtype=dtype, device=dev)  # noqa: E731
        self._timestamp, self._timestamp_last_update = z(N), z(N)
        self._is_outdated = torch.ones(N, dtype=torch.bool, device=dev)  # sensor_base.py:_initialize_impl
        self._all = torch.ones(N, dtype=torch.bool, device=dev)
        self._data = types.SimpleNamespace(pos_w=z(N, 3), quat_w=z(N, 4), lin_vel_b=z(N, 3), ang_vel_b=z(N, 3), lin_acc_b=z(N, 3), ang_acc_b=z(N, 3))
        self._data.quat_w[:, 0] = 1.0
        self._prev_lin_vel_w, self._prev_ang_vel_w = z(N, 3), z(N, 3)
        self._inputs = None
        self._dt = None  # Imu._dt: set by update()
        p = _lib.ptr
        d = self._data
        self._c = _lib.ImxImu(body_index=self.body_index or 0, num_bodies=1, com_per_env=int(self.com_pos_b is not None and self.com_pos_b.dim() == 2),
                              update_period=period, offset_pos=(ctypes.c_float * 3)(*pos), offset_quat=(ctypes.c_float * 4)(*rot),
                              gravity_bias=(ctypes.c_float * 3)(*bias), com_pos_b_d=p(self.com_pos_b), timestamp_d=p(self._timestamp),
                              timestamp_last_update_d=p(self._timestamp_last_update), is_outdated_d=p(self._is_outdated), pos_w_d=p(d.pos_w),
                              quat_w_d=p(d.quat_w), lin_vel_b_d=p(d.lin_vel_b), ang_vel_b_d=p(d.ang_vel_b), lin_acc_b_d=p(d.lin_acc_b),
                              ang_acc_b_d=p(d.ang_acc_b), prev_lin_vel_w_d=p(self._prev_lin_vel_w), prev_ang_vel_w_d=p(self._prev_ang_vel_w))

    def _check_inputs(self, pos_w, quat_w, lin_vel_w, ang_vel_w):
        N, b = self.num_envs, self.body_index
        B = 1
        if b is not None:
            if pos_w.dim() != 3 or pos_w.shape[1] <= b:
                raise ValueError(f"Imu '{self.name}': body_index {b} needs ({N}, B, 3) inputs with B > {b}, got pos_w {tuple(pos_w.shape)}")
            B = int(pos_w.shape[1])
        lead = (N,) if b is None else (N, B)
        for nm, t, w in (("pos_w", pos_w, 3), ("quat_w", quat_w, 4), ("lin_vel_w", lin_vel_w, 3), ("ang_vel_w", ang_vel_w, 3)):
            if tuple(t.shape) != lead + (w,):
                raise ValueError(f"Imu '{self.name}': {nm} must be {lead + (w,)}, got {tuple(t.shape)}")
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"Imu '{self.name}': {nm} must be a contiguous float32 tensor on {self.device}")
        return B

    def struct(self, dt=None, substeps=0, refresh=False, reset_mask=None) -> "_lib.ImxImu":
        """The sensor's ``imx_imu_t`` for one launch (the env packs several into one ``imx_imu`` call)."""
        c = self._c
        c.dt = float(self._dt or 0.0) if dt is None else float(dt)
        c.substeps, c.refresh = int(substeps), int(bool(refresh))
        ins = self._inputs or (None, None, None, None)
        c.body_pos_w_d, c.body_quat_w_d, c.body_lin_vel_w_d, c.body_ang_vel_w_d = (_lib.ptr(t) for t in ins)
        c.reset_mask_d = _lib.ptr(reset_mask)
        return c

    def set_inputs(self, pos_w, quat_w, lin_vel_w, ang_vel_w):
        self._c.num_bodies = self._check_inputs(pos_w, quat_w, lin_vel_w, ang_vel_w)
        self._inputs = (pos_w, quat_w, lin_vel_w, ang_vel_w)

    def _launch(self, **kw):
        c = self.struct(**kw)
        check(lib().imx_imu(ctypes.byref(c), 1, self.num_envs, _lib.current_stream(self.device)))

    def _mask(self, env_ids):
        N = self.num_envs
        if env_ids is None or isinstance(env_ids, slice) and env_ids == slice(None):
            return self._all
        ids = torch.as_tensor(env_ids, device=self.device)
        if ids.dtype in (torch.bool, torch.uint8) and tuple(ids.shape) == (N,):
            return ids.contiguous()
        m = torch.zeros(N, dtype=torch.bool, device=self.device)
        m[ids.long()] = True
        return m

    def reset(self, env_ids=None):
        """``SensorBase.reset`` + ``Imu.reset`` for ``env_ids`` (None = all; indices or an (N,) mask): clocks to zero, outdated,
        ``quat_w`` and the four body-frame vectors to zero.  No refresh, so no input is read."""
        self._launch(reset_mask=self._mask(env_ids))

    def update(self, dt: float, pos_w: torch.Tensor, quat_w: torch.Tensor, lin_vel_w: torch.Tensor, ang_vel_w: torch.Tensor,
               force_recompute: bool = False, substeps: int = 1, reset_mask=None):
        """``Imu.update(dt)``, ``substeps`` times, on the link pose and centre-of-mass velocities of the body the sensor sits on (kept
        by reference for ``data``); ``reset_mask``: those envs are reset first, in the same launch.  With ``force_recompute`` (or a
        ``history_length`` > 0) the outdated envs are refreshed."""
        self.set_inputs(pos_w, quat_w, lin_vel_w, ang_vel_w)
        self._dt = float(dt)
        self._launch(substeps=substeps, refresh=force_recompute or self.cfg.history_length > 0,
                     reset_mask=None if reset_mask is None else self._mask(reset_mask))

    @property
    def data(self):
        """``SensorBase.data``: ``_update_outdated_buffers`` first (one launch; an env that is not outdated leaves it at once)."""
        if self._dt is None or self._inputs is None:
            raise RuntimeError("The update function must be called before the data buffers are accessed the first time.")  # imu.py:144-147
        self._launch(refresh=True)
        return self._data
