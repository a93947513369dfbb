"""TEST INFRASTRUCTURE -- what the differential-IK and the operational-space case modules (tests/_diff_ik_cases.py, tests/_osc_cases.py)
share: building a host program of tools/, the processed action of a recorded step, the recorded schedule and the sentinel of the kernels'
output tensors.  ``g`` is an ``IkGolden`` or an ``OscGolden``."""

from __future__ import annotations

import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77.25


def host_compiler():
    import shutil

    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def build_host_program(name: str, out_dir: str, extra=()) -> str:
    import subprocess

    exe = os.path.join(out_dir, name)
    subprocess.check_call([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", *extra, os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe])
    return exe


def processed_full(g, term, t: int, PA: int | None = None):
    """(N, PA) processed action with the recorded fp32 columns of the term at its processed column."""
    PA = term.processed_col + term.width if PA is None else PA
    p = torch.zeros(g.N, PA)
    p[:, term.processed_col:term.processed_col + term.width] = torch.from_numpy(np.ascontiguousarray(g.ref(f"step{t}/processed_actions", "f32")))
    return p.contiguous()


def schedule(g):
    """The env's schedule: per step mode 1 on substep 0's state, then mode 2 on every substep's."""
    for t in range(g.steps):
        yield t, 0, 1
        for s in range(g.substeps):
            yield t, s, 2


def calls(g, merged_first: bool = False):
    """``schedule``; ``merged_first``: mode 3 for (mode 1, first mode 2), as the fused rollout launches."""
    for t, s, mode in schedule(g):
        if merged_first and mode == 2 and s == 0:
            continue
        yield t, s, 3 if merged_first and mode == 1 else mode


def sentinels_intact(N: int, *outputs) -> None:
    """``outputs``: (tensor, columns the kernel may write); the row after N and the columns after those must still hold SENTINEL."""
    for x, n in outputs:
        assert (x[N] == SENTINEL).all() and (x[:, n:] == SENTINEL).all(), "a sentinel was overwritten"
