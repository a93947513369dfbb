"""TEST INFRASTRUCTURE -- readers of the operational-space fixtures (tools/gen_golden_osc.py), the tolerances of the issue that introduced
the term, and the three ways the tests run the recorded schedule: the torch restatement (tests/_osc_oracle.py), the host program
(tools/osc_host.cpp) and the gfx950 kernel (``imx_osc``).  Shared by tests/test_osc.py and tests/test_osc_gpu.py.

Tolerances.  ``processed_actions``: equal to the fp32 recording.  Command state (desired pose, Kp, Kd, wrench): against the fp64
recording, within 4 E_ref with a floor of 2^-23 max(1, |x|), E_ref = the fp32 reference's own largest error against fp64 (osc.json).
``joint_efforts``: per env and substep rho = (||got - tau64||_inf - ulp) / (kappa 2^-24 max(||tau64||_inf, 1e-6)) <= 4 rho_ref of the
variant, ulp = one fp32 spacing at the env's largest |tau64|, kappa = the recorded fp64 cond2(M) cond2(J M^-1 J^T) (partial decoupling:
the larger block's; no decoupling: 1).  No env is excluded.
"""

from __future__ import annotations

import json
import os
import struct

import numpy as np
import torch

import _task_space_cases as tsc
from _task_space_cases import SENTINEL, calls as host_calls, host_compiler, schedule, sentinels_intact  # noqa: F401 (the tests use oc.*)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
VARIANTS = ("O1", "O2", "O3", "O4", "O5")
TASK = "Isaac-Reach-Franka-OSC-v0"
FACTOR = 4.0
CMD_SLICES = {"pose_des": slice(0, 7), "kp": slice(7, 13), "kd": slice(13, 19), "wrench": slice(19, 25)}
STATE_ORDER = ("root_pos_w", "root_quat_w", "root_lin_vel_w", "root_ang_vel_w", "body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w",
               "jacobians", "mass_matrices", "gravity_compensation_forces", "joint_pos", "joint_vel")

with open(os.path.join(GOLDEN, "osc.json")) as _f:
    META = json.load(_f)


def task_path(task: str = TASK) -> str:
    return os.path.join(GOLDEN, task + ".json")


def nullspace_target(osc, soft_limits, default_joint_pos):
    """_resolve_nullspace_joint_pos_targets (task_space_actions.py:539-566): (N, n), or None for 'zero' / 'none'."""
    if osc.nullspace_joint_pos_target == "center":
        return torch.mean(soft_limits[:, osc.joint_ids, :], dim=-1).contiguous()
    if osc.nullspace_joint_pos_target == "default":
        return default_joint_pos[:, osc.joint_ids].contiguous()
    return None


class OscGolden:
    """osc_<V>.npz (results, fp32 and fp64), osc_<V>_in.npz, osc_<V>_dyn.npz of one variant, cut to the first ``n`` envs."""

    def __init__(self, variant: str, n: int | None = None):
        from isaaclab_amd.plan import resolve_osc_term
        from isaaclab_amd.robots import RobotSpec

        self.v, self.meta = variant, META[variant]
        m = self.meta
        self.N = m["N"] if n is None else n
        self.steps, self.substeps = m["steps"], m["substeps"]
        self.out = np.load(os.path.join(GOLDEN, f"osc_{variant}.npz"))
        self.inp = np.load(os.path.join(GOLDEN, f"osc_{variant}_in.npz"))
        self.dyn = np.load(os.path.join(GOLDEN, f"osc_{variant}_dyn.npz"))
        self.robot = RobotSpec(name=m["robot"], joint_names=m["joint_names"], body_names=m["body_names"], default_joint_pos={".*": 0.0},
                               default_root_height=0.0, fixed_base=m["fixed_base"])
        self.osc = resolve_osc_term("arm_action", m["cfg"], self.robot)
        self.NB, self.ND, self.NM, self.J, self.B = m["NB"], m["ND"], m["NM"], m["num_joints"], m["num_bodies"]
        self.target = nullspace_target(self.osc, self.t(self.inp, "soft_joint_pos_limits"), self.t(self.inp, "default_joint_pos"))

    def t(self, z, key):
        return torch.from_numpy(np.ascontiguousarray(z[key][: self.N]))

    def raw(self, t):
        return self.t(self.inp, f"step{t}/raw")

    def reset_ids(self, t):
        return self.t(self.inp, f"step{t}/reset_mask").nonzero().flatten()

    def state(self, t, s, fill: float = 0.0) -> dict:
        """The tensors the term reads at substep ``s`` of step ``t``, in the full layouts; ``fill`` goes wherever it must not read: every
        other body, Jacobian row and column, joint, and mass-matrix row and column (and the mass matrix's strict upper triangle)."""
        tag = f"step{t}/sub{s}"
        o = self.osc
        b = o.body_idx
        body = {k: torch.full((self.N, self.B, w), fill) for k, w in (("body_pos_w", 3), ("body_quat_w", 4), ("body_lin_vel_w", 3), ("body_ang_vel_w", 3))}
        ev, rv = self.t(self.inp, f"{tag}/ee_vel_w"), self.t(self.inp, f"{tag}/root_vel_w")
        body["body_pos_w"][:, b], body["body_quat_w"][:, b] = self.t(self.inp, f"{tag}/ee_pos_w"), self.t(self.inp, f"{tag}/ee_quat_w")
        body["body_lin_vel_w"][:, b], body["body_ang_vel_w"][:, b] = ev[:, :3], ev[:, 3:]
        jac = torch.full((self.N, self.NB, 6, self.ND), fill)
        jac[:, o.jacobi_body_idx] = self.t(self.dyn, f"step{t}/jac_row")
        M, g = self.t(self.dyn, f"step{t}/mass_matrices").clone(), self.t(self.dyn, f"step{t}/gravity_compensation_forces").clone()
        jp, jv = self.t(self.inp, f"{tag}/joint_pos").clone(), self.t(self.inp, f"{tag}/joint_vel").clone()
        if fill != 0.0:
            keep = torch.zeros(self.ND, dtype=torch.bool)
            keep[o.jacobi_joint_ids] = True
            jac[:, o.jacobi_body_idx][:, :, ~keep] = fill
            keepj = torch.zeros(self.J, dtype=torch.bool)
            keepj[o.joint_ids] = True
            jp[:, ~keepj], jv[:, ~keepj], g[:, ~keepj] = fill, fill, fill
            M[:, ~keepj, :], M[:, :, ~keepj] = fill, fill
            M[:, torch.triu(torch.ones(self.NM, self.NM, dtype=torch.bool), diagonal=1)] = fill
        out = {"root_pos_w": self.t(self.inp, f"{tag}/root_pos_w"), "root_quat_w": self.t(self.inp, f"{tag}/root_quat_w"),
               "root_lin_vel_w": rv[:, :3], "root_ang_vel_w": rv[:, 3:], **body, "jacobians": jac, "mass_matrices": M,
               "gravity_compensation_forces": g, "joint_pos": jp, "joint_vel": jv}
        return {k: v.contiguous() for k, v in out.items()}

    def ref(self, key, prec="f64"):
        return self.out[f"{prec}/{key}"][: self.N]


def check_command_state(g: OscGolden, t: int, cmd, who: str):
    cmd = np.asarray(cmd, np.float64)
    for name, sl in CMD_SLICES.items():
        ref, got = g.ref(f"step{t}/{name}"), cmd[:, sl]
        tol = np.maximum(FACTOR * g.meta["E_ref"][name], 2.0 ** -23 * np.maximum(1.0, np.abs(ref)))
        err = np.abs(got - ref)
        assert np.isfinite(got).all() and (err <= tol).all(), (f"{who} {g.v} step {t} {name}: max error {err.max():.3g} against fp64, tolerance "
                                                                f"{tol[np.unravel_index(err.argmax(), err.shape)]:.3g}")


def rho(got, ref64, kappa):
    err = np.abs(np.asarray(got, np.float64) - ref64).max(axis=1)
    top = np.abs(ref64).max(axis=1)
    ulp = np.spacing(top.astype(np.float32)).astype(np.float64)
    return np.maximum(err - ulp, 0.0) / (kappa * 2.0 ** -24 * np.maximum(top, 1.0e-6))


def check_efforts(g: OscGolden, t: int, s: int, got, who: str) -> float:
    tag = f"step{t}/sub{s}"
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{who} {g.v} {tag}: joint_efforts is not finite"
    r = rho(got, g.ref(f"{tag}/joint_efforts"), g.ref(f"{tag}/kappa"))
    bound = FACTOR * g.meta["rho_ref"]
    print(f"{who} {g.v} {tag}: rho {r.max():.3g} (bound {bound:.3g})")
    assert (r <= bound).all(), f"{who} {g.v} {tag}: rho {r.max():.3g} at env {int(r.argmax())} (kappa {g.ref(f'{tag}/kappa')[int(r.argmax())]:.3g}), bound {bound:.3g}"
    return float(r.max())


def run_oracle(g: OscGolden) -> float:
    """The restatement over the whole recorded schedule, checked call by call.  Returns the largest rho."""
    from _osc_oracle import OscOracle

    orc = OscOracle(g.osc, g.N, g.target)
    worst = 0.0
    for t in range(g.steps):
        orc.reset(g.reset_ids(t))
        assert np.array_equal(orc.raw_actions.numpy(), g.ref(f"step{t}/raw_after_reset", "f32"))
        orc.process_actions(g.raw(t))
        assert np.array_equal(orc.processed_actions.numpy(), g.ref(f"step{t}/processed_actions", "f32")), f"{g.v} step {t}: processed_actions"
        orc.set_command(g.state(t, 0))
        check_command_state(g, t, orc.command_state.numpy(), "restatement")
        for s in range(g.substeps):
            worst = max(worst, check_efforts(g, t, s, orc.apply_actions(g.state(t, s)).numpy(), "restatement"))
    return worst


# ---------------------------------------------------------------------------------------------------- the host program
def build_host_program(out_dir: str, extra=()) -> str:
    return tsc.build_host_program("osc_host", out_dir, extra)


def processed_full(g: OscGolden, t: int, PA: int | None = None):
    return tsc.processed_full(g, g.osc, t, PA)


def target_or_zeros(g: OscGolden):
    return g.target if g.target is not None else torch.zeros(g.N, len(g.osc.joint_ids))


def host_outputs(exe: str, g: OscGolden, tmp_dir: str, merged_first: bool = False):
    """The host program over the schedule: ``[(t, s, mode, command_state (N, 25), joint_efforts (N, n))]`` as they stand after each call."""
    import subprocess

    from isaaclab_amd._lib import ImxOsc

    o = g.osc
    PA = o.processed_col + o.width
    calls = list(host_calls(g, merged_first))
    tag = f"{g.v}_{g.N}" + ("_merged" if merged_first else "")
    path_in, path_out = os.path.join(tmp_dir, tag + ".in"), os.path.join(tmp_dir, tag + ".out")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<12i", 0x3143534F, g.N, PA, g.B, g.NB, g.ND, g.NM, g.J, len(calls), 0, 0, 0))
        f.write(bytes(ImxOsc.from_term(o)))
        f.write(target_or_zeros(g).numpy().astype("<f4").tobytes())
        for t, s, mode in calls:
            st = g.state(t, s)
            f.write(struct.pack("<i", mode))
            for x in (processed_full(g, t, PA), *(st[k] for k in STATE_ORDER)):
                f.write(x.contiguous().numpy().astype("<f4").tobytes())
    subprocess.check_call([exe, path_in, path_out])
    n = len(o.joint_ids)
    out = np.fromfile(path_out, "<f4").reshape(len(calls), g.N * (25 + n))
    return [(t, s, mode, out[k, : g.N * 25].reshape(g.N, 25), out[k, g.N * 25:].reshape(g.N, n)) for k, (t, s, mode) in enumerate(calls)]


def run_host_program(exe: str, g: OscGolden, tmp_dir: str) -> float:
    worst = 0.0
    for t, s, mode, cmd, eff in host_outputs(exe, g, tmp_dir):
        check_command_state(g, t, cmd, "host program")  # (untouched by a mode 2 call)
        if mode & 2:
            worst = max(worst, check_efforts(g, t, s, eff, "host program"))
    return worst


# ---------------------------------------------------------------------------------------------------- the kernel
class KernelTerm:
    """``imx_osc`` over device tensors of its own.  The output tensors carry a sentinel row after N and a sentinel column after their
    last column."""

    def __init__(self, osc, N: int, target=None, device="cuda:0"):
        from isaaclab_amd._lib import ImxOsc

        self.osc, self.N, self.dev = osc, N, torch.device(device)
        self.cfg = ImxOsc.from_term(osc)
        self.n = len(osc.joint_ids)
        self.target = (target if target is not None else torch.zeros(N, self.n)).to(self.dev).contiguous()
        self.command_state = torch.full((N + 1, 26), SENTINEL, device=self.dev)
        self.joint_efforts = torch.full((N + 1, self.n + 1), SENTINEL, device=self.dev)

    def call(self, mode: int, proc, st: dict, cfg=None, **over) -> int:
        """Returns the status; 0 = launched."""
        import ctypes

        from isaaclab_amd import _lib

        d = {k: v.to(self.dev).contiguous() for k, v in st.items()}
        p = proc.to(self.dev).contiguous()
        self._keep = (d, p)
        a = dict(N=self.N, PA=p.shape[1], processed=_lib.ptr(p), B=d["body_pos_w"].shape[1], NB=d["jacobians"].shape[1], ND=d["jacobians"].shape[3],
                 NM=d["mass_matrices"].shape[1], J=d["joint_pos"].shape[1], target=_lib.ptr(self.target), cmd=_lib.ptr(self.command_state), ld_cmd=26,
                 eff=_lib.ptr(self.joint_efforts), ld_eff=self.n + 1, **{k: _lib.ptr(v) for k, v in d.items()})
        a.update(over)
        return _lib.lib().imx_osc(ctypes.byref(cfg if cfg is not None else self.cfg), a["N"], mode, a["processed"], a["PA"], a["root_pos_w"], a["root_quat_w"],
                                  a["root_lin_vel_w"], a["root_ang_vel_w"], a["body_pos_w"], a["body_quat_w"], a["body_lin_vel_w"], a["body_ang_vel_w"],
                                  a["B"], a["jacobians"], a["NB"], a["ND"], a["mass_matrices"], a["gravity_compensation_forces"], a["NM"],
                                  a["joint_pos"], a["joint_vel"], a["J"], a["target"], a["cmd"], a["ld_cmd"], a["eff"], a["ld_eff"],
                                  _lib.current_stream(self.dev))

    def outputs(self):
        cmd, eff = self.command_state.cpu(), self.joint_efforts.cpu()
        sentinels_intact(self.N, (cmd, 25), (eff, self.n))
        return cmd[: self.N, :25], eff[: self.N, : self.n]


def run_kernel(g: OscGolden, fill: float = 0.0, merged_first: bool = False):
    """The kernel over the recorded schedule, checked call by call; ``merged_first``: mode 3 for (mode 1, first mode 2).  Returns every
    call's outputs (for the bit-for-bit comparisons) and the largest rho."""
    k = KernelTerm(g.osc, g.N, g.target)
    outs, worst = [], 0.0
    for t, s, mode in host_calls(g, merged_first):
        assert k.call(mode, processed_full(g, t), g.state(t, s, fill)) == 0
        cmd, eff = k.outputs()
        outs.append((cmd.clone(), eff.clone()))
        if mode & 1:
            check_command_state(g, t, cmd.numpy(), "kernel")
        if mode & 2:
            worst = max(worst, check_efforts(g, t, s, eff.numpy(), "kernel"))
    return outs, worst
