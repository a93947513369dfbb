"""TEST INFRASTRUCTURE (build container only): tests/golden/live_cfg_plans.npz -- the plan blobs the term compiler makes from the
reference's own cfg OBJECTS (the ``@configclass`` instances its gym registry entries name, isaaclab_tasks/.../__init__.py), with the
simulator packages stubbed (oracle/ref_import.py).  tests/test_plan_and_terrain.py compiles the committed ``cfg.to_dict()`` dumps
(isaaclab_amd/configs) and requires the very same blobs, so the test needs neither the reference nor its stubs.
"""

from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

LIVE_CFGS = {  # task id -> (module, class) of the reference cfg its gym registry entry names (isaaclab_tasks/.../__init__.py)
    "Isaac-Cartpole-v0": ("isaaclab_tasks.manager_based.classic.cartpole.cartpole_env_cfg", "CartpoleEnvCfg"),
    "Isaac-Velocity-Flat-Anymal-C-v0": ("isaaclab_tasks.manager_based.locomotion.velocity.config.anymal_c.flat_env_cfg", "AnymalCFlatEnvCfg"),
    "Isaac-Velocity-Rough-Anymal-C-v0": ("isaaclab_tasks.manager_based.locomotion.velocity.config.anymal_c.rough_env_cfg", "AnymalCRoughEnvCfg"),
    "Isaac-Velocity-Rough-G1-v0": ("isaaclab_tasks.manager_based.locomotion.velocity.config.g1.rough_env_cfg", "G1RoughEnvCfg"),
}


def main():
    ref_import.install()
    from isaaclab_amd.env import load_task_cfg
    from isaaclab_amd.plan import compile_plan
    from isaaclab_amd.robots import ROBOTS

    rec, meta = {}, {}
    for task, (mod, cls) in LIVE_CFGS.items():
        cfg = getattr(importlib.import_module(mod), cls)()  # the LIVE reference cfg object (configclass instance)
        live = compile_plan(cfg, ROBOTS[load_task_cfg(task)["robot"]])
        rec[f"{task}/blob"] = np.ascontiguousarray(live.blob, np.int32)
        meta[task] = {"module": mod, "class": cls, "obs_dim": int(live.obs_dim)}
    rec["meta_json"] = np.array(json.dumps(meta))
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "live_cfg_plans.npz"), **rec)
    print({t: (m["obs_dim"], int(rec[f"{t}/blob"].size)) for t, m in meta.items()})


if __name__ == "__main__":
    main()
