"""Cases for the term compiler, shared by tests/test_plan_and_terrain.py and tools/gen_golden_plan_outcomes.py: the random cfgs of
tools/cfg_cases.py (``mutate``, which tools/fuzz_cfg.py draws from as well) and the fixed case list whose outcomes
tests/golden/plan_outcomes.npz pins.  Importing it pulls in neither the env nor the oracle."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cfg_cases import mutate  # noqa: E402


# ------------------------------------------------------------------------------------------------ the term compiler's outcomes
# tests/golden/plan_outcomes.npz pins what the term compiler makes of a fixed list of cfgs: one uint64 per case, the first 8 bytes of the
# SHA-256 of the outcome.  Recorded by tools/gen_golden_plan_outcomes.py, recomputed by tests/test_plan_and_terrain.py.
_PLAN_SCALARS = ("num_joints", "num_bodies", "history", "action_dim", "obs_dim", "num_rays", "cmd_dim", "step_dt", "max_episode_length",
                 "max_episode_length_s", "is_finite_horizon", "enable_corruption", "ray_direction", "ray_max_distance", "n_ext_rew",
                 "n_ext_term", "n_ext_obs", "mod_state_dim", "gravity_dir", "obs_dim_total", "scan_stateful", "scan_drift_range",
                 "term_slots", "obs_term_dims")
_TERM_LISTS = ("action_terms", "termination_terms", "reward_terms", "obs_terms")


def _term_mirror(terms) -> list:
    return [(t.name, t.func, int(t.op), int(t.dim), float(t.weight), bool(t.time_out)) for t in terms]


def plan_outcome(compile_plan, env_cfg: dict, robot) -> tuple[bool, bytes]:
    """(compiled?, outcome bytes) of one cfg: the blob as little-endian int32 followed by a canonical JSON of the ``Plan`` mirror, or the
    refusal as ``"ExceptionType: message"``.  The cfg is compiled from a copy."""
    import numpy as np

    try:
        plan = compile_plan(copy.deepcopy(env_cfg), robot)
    except Exception as e:  # noqa: BLE001 -- every refusal is an outcome
        return False, f"{type(e).__name__}: {e}".encode()
    mirror = {k: getattr(plan, k) for k in _PLAN_SCALARS}
    mirror.update({k: _term_mirror(getattr(plan, k)) for k in _TERM_LISTS})
    mirror["obs_groups"] = [(g.name, g.dim, g.term_dims, g.term_widths, g.concatenate, g.enable_corruption, g.first_record, g.num_records,
                             _term_mirror(g.terms)) for g in plan.obs_groups]
    return True, np.asarray(plan.blob).astype("<i4").tobytes() + json.dumps(mirror, sort_keys=True).encode()


def task_fixtures(configs_dir: str) -> list[dict]:
    """Every ``configs/*.json`` with an ``"env"`` key, in sorted file order."""
    out = []
    for f in sorted(os.listdir(configs_dir)):
        if f.endswith(".json"):
            fx = json.load(open(os.path.join(configs_dir, f)))
            if isinstance(fx, dict) and "env" in fx:
                out.append(fx)
    return out


def drop_one_param(fx: dict):
    """For every reward, termination and observation term of a fixture (cfg order) and every key of its ``params`` (cfg order): the
    fixture with that one key deleted."""
    env = fx["env"]
    paths = [("rewards", n) for n in (env.get("rewards") or {})] + [("terminations", n) for n in (env.get("terminations") or {})]
    paths += [("observations", g, n) for g, grp in (env.get("observations") or {}).items() if isinstance(grp, dict) for n in grp]
    for path in paths:
        term = env
        for k in path:
            term = term[k]
        if not isinstance(term, dict) or not isinstance(term.get("params"), dict):
            continue
        for key in term["params"]:
            cut = copy.deepcopy(fx)
            t = cut["env"]
            for k in path:
                t = t[k]
            del t["params"][key]
            yield cut


def plan_outcomes() -> dict:
    """The three pinned arrays -- ``fuzz`` (``mutate`` seeds 0..1999), ``configs``, ``drop_param`` -- plus, beside each, ``*_compiled``
    (bool per case), computed with whichever ``isaaclab_amd`` is first on ``sys.path``."""
    import hashlib

    import numpy as np

    import isaaclab_amd.plan as planmod
    from isaaclab_amd.robots import ROBOTS

    fixtures = task_fixtures(os.path.join(os.path.dirname(planmod.__file__), "configs"))
    cases = {"fuzz": [mutate(np.random.default_rng(seed))[0] for seed in range(2000)], "configs": fixtures,
             "drop_param": [cut for fx in fixtures for cut in drop_one_param(fx)]}
    out = {}
    for key, fxs in cases.items():
        res = [plan_outcome(planmod.compile_plan, fx["env"], ROBOTS[fx["robot"]]) for fx in fxs]
        out[key] = np.array([int.from_bytes(hashlib.sha256(b).digest()[:8], "little") for _, b in res], np.uint64)
        out[key + "_compiled"] = np.array([ok for ok, _ in res], bool)
    return out
