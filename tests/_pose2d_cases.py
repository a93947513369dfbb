"""TEST INFRASTRUCTURE -- readers of the pose-2d command fixtures (tools/gen_golden_pose2d_command.py) and what the CPU and GPU tests of the
``UniformPose2dCommand`` / ``TerrainBasedPose2dCommand`` producers share (tests/test_pose2d_command.py, tests/test_pose2d_command_gpu.py)."""

from __future__ import annotations

import json
import math
import os
import struct

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("U0", "U1", "T1")
# the term's tensors, in the order tools/pose2d_host.cpp writes them; heading_command_w is an angle that is no decision: compared on the circle
OUT_KEYS = ("command", "pos_command_w", "heading_command_w", "time_left", "error_pos_2d", "error_heading", "command_counter")
WIDTHS = {"command": 4, "pos_command_w": 3}


def wrap_to_pi(a):
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi


def assert_outputs_close(got: dict, ref: dict, tol: float, what: str, names=OUT_KEYS):
    """``command_counter`` bit for bit, ``heading_command_w`` on the circle (|wrap_to_pi(got - ref)| <= tol: +pi and -pi are one heading),
    every other tensor within ``tol`` relative to max(|ref|, 1) (``_util.assert_close``)."""
    from _util import assert_close

    for name in names:
        g, r = got[name].cpu(), ref[name].cpu()
        if name == "command_counter":
            assert torch.equal(g, r), f"{what} {name}"
        elif name == "heading_command_w":
            err = wrap_to_pi(g.double() - r.double()).abs()
            over = err > tol * r.double().abs().clamp(min=1.0)  # (the bound of assert_close)
            assert not bool(over.any()), f"{what} {name}: max err on the circle {float(err.max()):.3e} (tol {tol}), {int(over.sum())} elements over"
        else:
            assert_close(g, r, tol, f"{what} {name}")


class Pose2dGolden:
    """tests/golden/pose2d_command.npz (results) + pose2d_command_in.npz (inputs, draws): the REAL classes, variants U0 / U1 / T1."""

    _files = None

    def __init__(self, variant: str):
        if Pose2dGolden._files is None:  # read once, shared by every test
            Pose2dGolden._files = (dict(np.load(os.path.join(GOLDEN, "pose2d_command.npz"))), dict(np.load(os.path.join(GOLDEN, "pose2d_command_in.npz"))))
        self.v = variant
        self.out, self.inp = Pose2dGolden._files
        m = json.loads(str(self.out[f"{variant}/meta"]))
        self.meta, self.cfg = m, m["cfg"]
        self.N, self.steps, self.step_dt, self.kind = m["N"], m["steps"], m["step_dt"], m["kind"]

    def t(self, key: str) -> torch.Tensor:
        z = self.inp if f"{self.v}/{key}" in self.inp else self.out
        return torch.from_numpy(np.ascontiguousarray(z[f"{self.v}/{key}"]))

    def constants(self, n: int | None = None) -> dict:
        """env_origins, default_root_z and, for T1, valid_targets / terrain_levels / terrain_types; cut to the first ``n`` envs."""
        n = self.N if n is None else n
        d = {"env_origins": self.t("env_origins")[:n].contiguous(), "default_root_z": self.t("default_root_z")[:n].contiguous()}
        if self.kind == 1:
            d.update(valid_targets=self.t("valid_targets"), terrain_levels=self.t("terrain_levels")[:n].contiguous(),
                     terrain_types=self.t("terrain_types")[:n].contiguous())
        return d

    def inputs(self, k: int, n: int | None = None) -> dict:
        n = self.N if n is None else n
        d = {"root_pos_w": self.t(f"step{k}/root_pos_w")[:n].contiguous(), "root_quat_w": self.t(f"step{k}/root_quat_w")[:n].contiguous(),
             "reset_mask": self.t(f"step{k}/reset_mask")[:n].contiguous(), "uniforms": self.t(f"step{k}/uniforms")[:, :n].contiguous(),
             "patch_ids": self.t(f"step{k}/patch_ids")[:, :n].contiguous() if self.kind == 1 else None}
        return d

    def expected(self, k: int, n: int | None = None) -> dict:
        n = self.N if n is None else n
        return {name: self.t(f"step{k}/{name}")[:n] for name in OUT_KEYS}

    def oracle(self, n: int | None = None, dtype=torch.float32):
        from _pose2d_oracle import Pose2dOracle

        n = self.N if n is None else n
        return Pose2dOracle(self.cfg, n, kind=self.kind, dtype=dtype, **self.constants(n))

    def producer(self, device, n: int | None = None, seed: int = 0):
        from isaaclab_amd import producers

        n = self.N if n is None else n
        c = {k: v.to(device) for k, v in self.constants(n).items()}
        cls = producers.TerrainBasedPose2dCommand if self.kind == 1 else producers.UniformPose2dCommand
        return cls(self.cfg, n, self.step_dt, device, seed=seed, **c)

    def host_file(self, path: str):
        """The flat input file of tools/pose2d_host.cpp for every step of this variant."""
        c, cfg = self.constants(), self.cfg
        L, T, P = tuple(c["valid_targets"].shape[:3]) if self.kind == 1 else (0, 0, 0)
        r = cfg["ranges"]
        cfg8 = np.asarray([*cfg["resampling_time_range"], *(r.get("pos_x") or (0, 0)), *(r.get("pos_y") or (0, 0)), *r["heading"]], np.float32)
        with open(path, "wb") as f:
            f.write(struct.pack("<8i", 0x31443250, self.N, self.steps, self.kind, int(cfg["simple_heading"]), L, T, P))
            f.write(cfg8.tobytes())
            f.write(np.float32(self.step_dt).tobytes())
            f.write(c["env_origins"].numpy().astype(np.float32).tobytes())
            f.write(c["default_root_z"].numpy().astype(np.float32).tobytes())
            if self.kind == 1:
                f.write(c["valid_targets"].numpy().astype(np.float32).tobytes())
                f.write(c["terrain_levels"].numpy().astype(np.int64).tobytes())
                f.write(c["terrain_types"].numpy().astype(np.int64).tobytes())
            for k in range(self.steps):
                d = self.inputs(k)
                f.write(d["root_pos_w"].numpy().tobytes())
                f.write(d["root_quat_w"].numpy().tobytes())
                f.write(d["reset_mask"].numpy().astype(np.int32).tobytes())
                f.write(d["uniforms"].numpy().tobytes())
                if self.kind == 1:
                    f.write(d["patch_ids"].numpy().astype(np.int64).tobytes())

    def read_host_output(self, path: str) -> list[dict]:
        raw = open(path, "rb").read()
        N, at, steps = self.N, 0, []
        for _ in range(self.steps):
            d = {}
            for name in OUT_KEYS:
                w = WIDTHS.get(name, 1)
                dt, size = (np.int64, 8) if name == "command_counter" else (np.float32, 4)
                a = np.frombuffer(raw, dt, N * w, at).copy()
                at += N * w * size
                d[name] = torch.from_numpy(a.reshape(N, w) if w > 1 else a)
            steps.append(d)
        assert at == len(raw), "the host program wrote more than the steps asked for"
        return steps


class NavOrchGolden:
    """tests/golden/navigation_orchestration.npz (results), navigation_orchestration_in.npz (inputs, actions, draws) and
    navigation_orchestration.json (the cfg): the REAL ``_reset_idx`` / EventManager / CommandManager + UniformPose2dCommand."""

    def __init__(self):
        from isaaclab_amd.env import load_task_cfg
        from isaaclab_amd.robots import ROBOTS

        self.z = np.load(os.path.join(GOLDEN, "navigation_orchestration.npz"))
        self.zi = np.load(os.path.join(GOLDEN, "navigation_orchestration_in.npz"))
        self.meta = json.loads(str(self.z["meta_json"]))
        self.fixture = load_task_cfg(os.path.join(GOLDEN, "navigation_orchestration.json"))
        self.robot = ROBOTS[self.fixture["robot"]]
        self.N, self.steps = self.meta["num_envs"], self.meta["steps"]

    def t(self, key) -> torch.Tensor:
        z = self.zi if key in self.zi.files else self.z
        return torch.from_numpy(np.ascontiguousarray(z[key]))

    def reset_mask(self, tag: str) -> torch.Tensor:
        """The envs ``_reset_idx`` ran on: all of them in ``reset``, the recorded ``reset_env_ids`` in a step."""
        m = torch.zeros(self.N, dtype=torch.bool)
        m[self.t(f"{tag}/reset_env_ids") if tag != "reset" else slice(None)] = True
        return m

    def log(self, tag: str) -> dict:
        return json.loads(str(self.z[f"{tag}/log_json"]))

    def feed(self, device):
        """The synthetic feed with the recorded tensors written over it: snapshot 0 = the state of reset(), 1 + t = of step t."""
        from isaaclab_amd.state_feed import STATIC, StateFeed

        feed = StateFeed(self.robot, self.N, device, seed=self.meta["seed"], num_snapshots=self.steps + 1)
        for n in STATIC:
            feed._static[n] = self.t(f"static/{n}").to(device).contiguous()
        for k, tag in enumerate(["reset"] + [f"step{s}" for s in range(self.steps)]):
            for key in self.zi.files:
                if key.startswith(f"{tag}/in/"):
                    feed._stack[key[len(tag) + 4:]][k] = self.t(key).to(device)
        return feed


def term_outputs(term) -> dict:
    """The seven tensors of a ``producers.UniformPose2dCommand`` (after its first compute) or a ``Pose2dOracle``."""
    return {"command": term.command, "pos_command_w": term.pos_command_w, "heading_command_w": term.heading_command_w,
            "time_left": term.time_left, "error_pos_2d": term.metrics["error_pos_2d"], "error_heading": term.metrics["error_heading"],
            "command_counter": term.command_counter}


def zero_struct(N: int, device, kind: int = 0):
    """A valid ``ImxPose2dCommand`` over zero buffers (resampling_time_range (1, 2)) and the tensors that keep it alive."""
    from isaaclab_amd import _lib

    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)  # noqa: E731
    keep = dict(env_origins_d=z(N, 3), default_root_z_d=z(N), command_d=z(N, 4), pos_command_w_d=z(N, 3), heading_command_w_d=z(N),
                time_left_d=z(N), command_counter_d=z(N, dtype=torch.long), metric_error_pos_2d_d=z(N), metric_error_heading_d=z(N))
    if kind == 1:
        keep.update(valid_targets_d=z(2, 2, 3, 3), terrain_levels_d=z(N, dtype=torch.long), terrain_types_d=z(N, dtype=torch.long))
    c = _lib.ImxPose2dCommand(kind=kind, **{k: v.data_ptr() for k, v in keep.items()})
    if kind == 1:
        c.num_levels, c.num_types, c.num_patches = 2, 2, 3
    for k, v in enumerate((1.0, 2.0, -1.0, 1.0, -1.0, 1.0, -3.0, 3.0)):
        c.cfg[k] = v
    return c, keep
