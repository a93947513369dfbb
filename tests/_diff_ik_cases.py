"""TEST INFRASTRUCTURE -- readers of the differential-IK fixtures (tools/gen_golden_diff_ik.py), the tolerances of the issue that
introduced the term, and the three ways the tests run the recorded schedule: the torch restatement (tests/_diff_ik_oracle.py), the host
program (tools/diff_ik_host.cpp) and the gfx950 kernel (``imx_diff_ik``).  Shared by tests/test_diff_ik.py and tests/test_diff_ik_gpu.py.

Tolerances.  ``processed_actions``: equal to the fp32 recording.  ``ee_pos_des`` / ``ee_quat_des``: against the fp64 recording, within
4 E_ref with a floor of 2^-23 max(1, |x|), E_ref = the fp32 reference's own largest error against fp64 (diff_ik.json).
``joint_pos_des``: per env and substep rho = (||got - ref64||_inf - ulp) / (kappa 2^-24 max(||dq_ref64||_inf, 1e-6)) <= 4 rho_ref of the
variant, ulp = one fp32 spacing at the env's largest |joint_pos_des|, kappa = the recorded fp64 condition number of J J^T + lambda^2 I.
No env is excluded.
"""

from __future__ import annotations

import json
import os
import struct

import numpy as np
import torch

import _task_space_cases as tsc
from _task_space_cases import SENTINEL, calls, host_compiler, schedule, sentinels_intact  # noqa: F401 (the tests use ikc.*)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
VARIANTS = ("V1", "V2", "V3", "V4", "V5")
IK_TASKS = ("Isaac-Reach-Franka-IK-Abs-v0", "Isaac-Reach-Franka-IK-Rel-v0", "Isaac-Lift-Cube-Franka-IK-Abs-v0", "Isaac-Lift-Cube-Franka-IK-Rel-v0")
FACTOR = 4.0

with open(os.path.join(GOLDEN, "diff_ik.json")) as _f:
    META = json.load(_f)


def task_path(task: str) -> str:
    return os.path.join(GOLDEN, task + ".json")


def full_layout(rows, NB: int, jb: int, fill: float = 0.0):
    """(N, NB, 6, ND) with the recorded block in row ``jb``: the fixtures keep only that row."""
    N, _, ND = rows.shape
    jac = torch.full((N, NB, 6, ND), fill)
    jac[:, jb] = rows
    return jac.contiguous()


class IkGolden:
    """diff_ik_<V>.npz (results, fp32 and fp64), diff_ik_<V>_in.npz, diff_ik_<V>_jac.npz of one variant, cut to the first ``n`` envs."""

    def __init__(self, variant: str, n: int | None = None):
        from isaaclab_amd.plan import resolve_ik_term
        from isaaclab_amd.robots import RobotSpec

        self.v, self.meta = variant, META[variant]
        m = self.meta
        self.N = m["N"] if n is None else n
        self.steps, self.substeps = m["steps"], m["substeps"]
        self.out = np.load(os.path.join(GOLDEN, f"diff_ik_{variant}.npz"))
        self.inp = np.load(os.path.join(GOLDEN, f"diff_ik_{variant}_in.npz"))
        self.jac = np.load(os.path.join(GOLDEN, f"diff_ik_{variant}_jac.npz"))
        self.robot = RobotSpec(name=m["robot"], joint_names=m["joint_names"], body_names=m["body_names"], default_joint_pos={".*": 0.0},
                               default_root_height=0.0, fixed_base=m["fixed_base"])
        self.ik = resolve_ik_term("arm_action", m["cfg"], self.robot)
        self.NB, self.ND, self.J, self.B = m["NB"], m["ND"], m["num_joints"], m["num_bodies"]

    def t(self, z, key):
        return torch.from_numpy(np.ascontiguousarray(z[key][: self.N]))

    def raw(self, t):
        return self.t(self.inp, f"step{t}/raw")

    def reset_ids(self, t):
        return self.t(self.inp, f"step{t}/reset_mask").nonzero().flatten()

    def state(self, t, s, fill: float = 0.0) -> dict:
        """The tensors the term reads at substep ``s`` of step ``t``, in the full layouts; ``fill`` goes wherever it must not read."""
        tag = f"step{t}/sub{s}"
        ik = self.ik
        bp = torch.full((self.N, self.B, 3), fill)
        bq = torch.full((self.N, self.B, 4), fill)
        bp[:, ik.body_idx], bq[:, ik.body_idx] = self.t(self.inp, f"{tag}/ee_pos_w"), self.t(self.inp, f"{tag}/ee_quat_w")
        rows = self.t(self.jac, f"step{t}/jac_row")
        jac = full_layout(rows, self.NB, ik.jacobi_body_idx, fill)
        jp = self.t(self.inp, f"{tag}/joint_pos").clone()
        if fill != 0.0:
            keep = torch.zeros(self.ND, dtype=torch.bool)
            keep[ik.jacobi_joint_ids] = True
            jac[:, ik.jacobi_body_idx][:, :, ~keep] = fill
            keepj = torch.zeros(self.J, dtype=torch.bool)
            keepj[ik.joint_ids] = True
            jp[:, ~keepj] = fill
        return {"root_pos_w": self.t(self.inp, f"{tag}/root_pos_w"), "root_quat_w": self.t(self.inp, f"{tag}/root_quat_w"), "body_pos_w": bp.contiguous(),
                "body_quat_w": bq.contiguous(), "jacobians": jac.contiguous(), "joint_pos": jp.contiguous()}

    def ref(self, key, prec="f64"):
        return self.out[f"{prec}/{key}"][: self.N]


def check_pose_des(g: IkGolden, t: int, pos, quat, who: str):
    for name, got in (("ee_pos_des", pos), ("ee_quat_des", quat)):
        ref = g.ref(f"step{t}/{name}")
        got = np.asarray(got, np.float64)
        tol = np.maximum(FACTOR * g.meta["E_ref"][name], 2.0 ** -23 * np.maximum(1.0, np.abs(ref)))
        err = np.abs(got - ref)
        assert np.isfinite(got).all() and (err <= tol).all(), (f"{who} {g.v} step {t} {name}: max error {err.max():.3g} against fp64, tolerance "
                                                                f"{tol[np.unravel_index(err.argmax(), err.shape)]:.3g}")


def rho(got, ref64, dq64, kappa):
    err = np.abs(np.asarray(got, np.float64) - ref64).max(axis=1)
    ulp = np.spacing(np.abs(ref64).max(axis=1).astype(np.float32)).astype(np.float64)
    return np.maximum(err - ulp, 0.0) / (kappa * 2.0 ** -24 * np.maximum(np.abs(dq64).max(axis=1), 1.0e-6))


def check_joint_des(g: IkGolden, t: int, s: int, got, who: str) -> float:
    tag = f"step{t}/sub{s}"
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{who} {g.v} {tag}: joint_pos_des is not finite"
    r = rho(got, g.ref(f"{tag}/joint_pos_des"), g.ref(f"{tag}/dq"), g.ref(f"{tag}/kappa"))
    bound = FACTOR * g.meta["rho_ref"]
    assert (r <= bound).all(), f"{who} {g.v} {tag}: rho {r.max():.3g} at env {int(r.argmax())} (kappa {g.ref(f'{tag}/kappa')[int(r.argmax())]:.3g}), bound {bound:.3g}"
    return float(r.max())


def run_oracle(g: IkGolden) -> float:
    """The restatement over the whole recorded schedule, checked call by call.  Returns the largest rho."""
    from _diff_ik_oracle import DiffIKOracle

    orc = DiffIKOracle(g.ik, g.N)
    worst = 0.0
    for t in range(g.steps):
        orc.reset(g.reset_ids(t))
        assert np.array_equal(orc.raw_actions.numpy(), g.ref(f"step{t}/raw_after_reset", "f32"))
        orc.process_actions(g.raw(t))
        assert np.array_equal(orc.processed_actions.numpy(), g.ref(f"step{t}/processed_actions", "f32")), f"{g.v} step {t}: processed_actions"
        orc.set_command(g.state(t, 0))
        check_pose_des(g, t, orc.ee_pos_des.numpy(), orc.ee_quat_des.numpy(), "restatement")
        for s in range(g.substeps):
            worst = max(worst, check_joint_des(g, t, s, orc.apply_actions(g.state(t, s)).numpy(), "restatement"))
    return worst


# ---------------------------------------------------------------------------------------------------- the host program
def build_host_program(out_dir: str) -> str:
    return tsc.build_host_program("diff_ik_host", out_dir)


def processed_full(g: IkGolden, t: int, PA: int | None = None):
    return tsc.processed_full(g, g.ik, t, PA)


def run_host_program(exe: str, g: IkGolden, tmp_dir: str) -> float:
    import subprocess

    from isaaclab_amd._lib import ImxDiffIk

    ik = g.ik
    PA = ik.processed_col + ik.width
    calls = list(schedule(g))
    path_in, path_out = os.path.join(tmp_dir, f"{g.v}_{g.N}.in"), os.path.join(tmp_dir, f"{g.v}_{g.N}.out")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<8i", 0x314B4944, g.N, PA, g.B, g.NB, g.ND, g.J, len(calls)))
        f.write(bytes(ImxDiffIk.from_term(ik)))
        for t, s, mode in calls:
            st = g.state(t, s)
            f.write(struct.pack("<i", mode))
            for x in (processed_full(g, t, PA), st["root_pos_w"], st["root_quat_w"], st["body_pos_w"], st["body_quat_w"], st["jacobians"], st["joint_pos"]):
                f.write(x.contiguous().numpy().astype("<f4").tobytes())
    subprocess.check_call([exe, path_in, path_out])
    n = len(ik.joint_ids)
    out = np.fromfile(path_out, "<f4").reshape(len(calls), g.N * (7 + n))
    worst = 0.0
    for k, (t, s, mode) in enumerate(calls):
        pos, quat, des = out[k, : g.N * 3].reshape(g.N, 3), out[k, g.N * 3: g.N * 7].reshape(g.N, 4), out[k, g.N * 7:].reshape(g.N, n)
        check_pose_des(g, t, pos, quat, "host program")  # (untouched by a mode 2 call)
        if mode & 2:
            worst = max(worst, check_joint_des(g, t, s, des, "host program"))
    return worst


# ---------------------------------------------------------------------------------------------------- the kernel
class KernelTerm:
    """``imx_diff_ik`` over device tensors of its own.  The output tensors carry a sentinel row after N and ``joint_pos_des`` a sentinel
    column after the term's joints."""

    def __init__(self, ik, N: int, device="cuda:0"):
        from isaaclab_amd._lib import ImxDiffIk

        self.ik, self.N, self.dev = ik, N, torch.device(device)
        self.cfg = ImxDiffIk.from_term(ik)
        self.n = len(ik.joint_ids)
        self.ee_pos_des = torch.full((N + 1, 3), SENTINEL, device=self.dev)
        self.ee_quat_des = torch.full((N + 1, 4), SENTINEL, device=self.dev)
        self.joint_pos_des = torch.full((N + 1, self.n + 1), SENTINEL, device=self.dev)

    def call(self, mode: int, proc, st: dict, cfg=None, **over) -> int:
        """Returns the status; 0 = launched."""
        import ctypes

        from isaaclab_amd import _lib

        d = {k: v.to(self.dev).contiguous() for k, v in st.items()}
        p = proc.to(self.dev).contiguous()
        self._keep = (d, p)
        a = dict(N=self.N, PA=p.shape[1], processed=_lib.ptr(p), root_pos=_lib.ptr(d["root_pos_w"]), root_quat=_lib.ptr(d["root_quat_w"]),
                 body_pos=_lib.ptr(d["body_pos_w"]), body_quat=_lib.ptr(d["body_quat_w"]), B=d["body_pos_w"].shape[1], jac=_lib.ptr(d["jacobians"]),
                 NB=d["jacobians"].shape[1], ND=d["jacobians"].shape[3], joint_pos=_lib.ptr(d["joint_pos"]), J=d["joint_pos"].shape[1],
                 pos_des=_lib.ptr(self.ee_pos_des), quat_des=_lib.ptr(self.ee_quat_des), q_des=_lib.ptr(self.joint_pos_des), ld=self.n + 1)
        a.update(over)
        return _lib.lib().imx_diff_ik(ctypes.byref(cfg if cfg is not None else self.cfg), a["N"], mode, a["processed"], a["PA"], a["root_pos"], a["root_quat"],
                                      a["body_pos"], a["body_quat"], a["B"], a["jac"], a["NB"], a["ND"], a["joint_pos"], a["J"], a["pos_des"],
                                      a["quat_des"], a["q_des"], a["ld"], _lib.current_stream(self.dev))

    def outputs(self):
        pos, quat, des = self.ee_pos_des.cpu(), self.ee_quat_des.cpu(), self.joint_pos_des.cpu()
        sentinels_intact(self.N, (pos, 3), (quat, 4), (des, self.n))
        return pos[: self.N], quat[: self.N], des[: self.N, : self.n]


def run_kernel(g: IkGolden, fill: float = 0.0, merged_first: bool = False):
    """The kernel over the recorded schedule, checked call by call; ``merged_first``: mode 3 for (mode 1, first mode 2).  Returns every
    call's outputs (for the bit-for-bit comparisons) and the largest rho."""
    k = KernelTerm(g.ik, g.N)
    outs, worst = [], 0.0
    for t, s, mode in calls(g, merged_first):
        assert k.call(mode, processed_full(g, t), g.state(t, s, fill)) == 0
        pos, quat, des = k.outputs()
        outs.append((pos.clone(), quat.clone(), des.clone()))
        if mode & 1:
            check_pose_des(g, t, pos.numpy(), quat.numpy(), "kernel")
        if mode & 2:
            worst = max(worst, check_joint_des(g, t, s, des.numpy(), "kernel"))
    return outs, worst
