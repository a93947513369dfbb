"""Random env cfgs for the term compiler, shared by tools/fuzz_cfg.py, tools/gen_golden_plan_outcomes.py and (through
tests/_cfg_cases.py) the test suite.

``mutate(rng)`` draws one cfg: the rough-terrain Anymal-C scene with random subsets (order kept) of the reward / termination /
observation terms of the kitchen-sink fixture, random weights (incl. 0), scale / clip / the three noise kinds, modifier chains,
per-term and per-group history, episode length and the six joint action classes in random combinations.  It reads the committed
task configs only: importing it pulls in neither the env nor the oracle."""
import copy
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "isaaclab_amd", "configs")
BASE = json.load(open(os.path.join(CFG, "Isaac-Velocity-Rough-Anymal-C-v0.json")))
POOL = json.load(open(os.path.join(CFG, "Isaac-Velocity-Rough-Anymal-C-v0-kitchen.json")))["env"]
NOISE = "isaaclab.utils.noise.noise_model:uniform_noise"
ACTIONS = json.load(open(os.path.join(CFG, "Isaac-Velocity-Flat-Anymal-C-v0-actions.json")))["env"]["actions"]


def mutate(rng):
    fx = copy.deepcopy(BASE)
    env = fx["env"]
    what = []
    names = list(POOL["terminations"])
    keep_t = [n for n in names if n == "time_out" or rng.random() < 0.5]
    env["terminations"] = {n: copy.deepcopy(POOL["terminations"][n]) for n in keep_t}
    names = list(POOL["rewards"])
    keep = [n for n in names if rng.random() < 0.6] or ["alive"]
    env["rewards"] = {}
    for n in keep:
        t = copy.deepcopy(POOL["rewards"][n])
        tk = (t.get("params") or {}).get("term_keys")
        if tk is not None and any(k not in env["terminations"] for k in ([tk] if isinstance(tk, str) else tk)):
            continue
        if rng.random() < 0.4:
            t["weight"] = float(rng.choice([0.0, 1.0, -0.5, 2.5e-5, -3.0]))
        env["rewards"][n] = t
    if not env["rewards"]:
        env["rewards"] = {"alive": copy.deepcopy(POOL["rewards"]["alive"])}
    what.append(f"{len(env['rewards'])} rewards, {len(env['terminations'])} terminations")
    env["observations"] = {}
    for gname in (["policy", "critic"] if rng.random() < 0.5 else ["policy"]):
        src = POOL["observations"][gname]
        terms = [k for k, v in src.items() if isinstance(v, dict)]
        keep_o = [k for k in terms if rng.random() < 0.6] or [terms[int(rng.integers(0, len(terms)))]]
        grp = {k: copy.deepcopy(v) for k, v in src.items() if not isinstance(v, dict)}
        grp["enable_corruption"] = bool(rng.random() < 0.6)
        if rng.random() < 0.3:
            grp["history_length"] = int(rng.choice([2, 3]))
            grp["flatten_history_dim"] = True
        for k in keep_o:
            t = copy.deepcopy(src[k])
            if rng.random() < 0.25:
                t["scale"] = float(rng.choice([0.25, 2.0, -1.0]))
            if rng.random() < 0.25:
                lo = -float(rng.choice([0.5, 1.0, 3.0]))
                t["clip"] = [lo, -lo * float(rng.choice([1.0, 0.5]))]
            r = rng.random()
            op = str(rng.choice(["add", "add", "scale", "abs"]))
            if r < 0.25:
                a = float(rng.choice([0.01, 0.1, 0.5]))
                t["noise"] = {"func": NOISE, "operation": op, "n_min": -a, "n_max": a}
            elif r < 0.35:
                t["noise"] = {"func": NOISE.replace("uniform_noise", "gaussian_noise"), "operation": op, "mean": float(rng.choice([0.0, 0.01, 1.0])), "std": float(rng.choice([0.05, 0.3]))}
            elif r < 0.42:
                t["noise"] = {"func": NOISE.replace("uniform_noise", "constant_noise"), "operation": op, "bias": float(rng.choice([0.05, 0.9, 0.25]))}
            elif r < 0.55:
                t["noise"] = None
            if rng.random() < 0.25:  # a chain of modifiers (isaaclab.utils.modifiers): stateless ones and the two stateful classes
                M = "isaaclab.utils.modifiers.modifier:"
                chain = []
                for _ in range(int(rng.integers(1, 4))):
                    kind = str(rng.choice(["scale", "bias", "clip", "clip1", "DigitalFilter", "Integrator"]))
                    if kind == "scale":
                        chain.append({"func": M + "scale", "params": {"multiplier": float(rng.choice([2.0, 0.5, -1.0]))}})
                    elif kind == "bias":
                        chain.append({"func": M + "bias", "params": {"value": float(rng.choice([0.25, -0.1]))}})
                    elif kind == "clip":
                        chain.append({"func": M + "clip", "params": {"bounds": [-float(rng.choice([0.01, 0.8])), float(rng.choice([0.015, 1.0]))]}})
                    elif kind == "clip1":
                        chain.append({"func": M + "clip", "params": {"bounds": [-0.8, None] if rng.random() < 0.5 else [None, 0.5]}})
                    elif kind == "DigitalFilter":
                        na, nb = int(rng.integers(1, 3)), int(rng.integers(1, 4))
                        chain.append({"func": M + "DigitalFilter", "params": {}, "A": [float(x) for x in rng.uniform(-0.5, 0.6, na).round(2)],
                                      "B": [float(x) for x in rng.uniform(0.0, 1.0, nb).round(2)]})
                    else:
                        chain.append({"func": M + "Integrator", "params": {}, "dt": float(rng.choice([0.02, 0.005]))})
                t["modifiers"] = chain
            if grp.get("history_length") is None and rng.random() < 0.2:
                t["history_length"] = int(rng.choice([2, 3]))
                t["flatten_history_dim"] = True
            grp[k] = t
        env["observations"][gname] = grp
        what.append(f"{gname}: {len(keep_o)} terms, group history {grp.get('history_length')}, corruption {grp['enable_corruption']}")
    env["episode_length_s"] = float(rng.choice([20.0, 5.0, 0.5]))
    # (decimation stays: with a shorter env step the height scanner's update_period gates its refresh -- SensorBase, reproduced by the
    #  product and pinned by the kitchen fixture -- while this harness hands the oracle every step's hits)
    if rng.random() < 0.6:
        act = env["actions"]["joint_pos"]
        act["scale"] = float(rng.choice([0.5, 0.25, 1.0]))
        if rng.random() < 0.3:
            act["clip"] = {".*": [-1.0, 1.0]}
        what.append("JointPositionAction")
    else:  # a random combination of the other joint action classes (the `-actions` fixture's terms with other numbers)
        pool = copy.deepcopy(ACTIONS)
        keep_a = [n for n in pool if rng.random() < 0.6] or ["all_ema"]
        env["actions"] = {}
        for n in keep_a:
            a = pool[n]
            if isinstance(a.get("scale"), float):
                a["scale"] = float(rng.choice([0.3, 0.9, 2.0]))
            if "offset" in a and isinstance(a["offset"], float):
                a["offset"] = float(rng.choice([0.0, 0.7, -0.2]))
            if n == "all_ema":
                a["alpha"] = {".*HAA": float(rng.choice([0.3, 1.0])), ".*HFE": float(rng.choice([0.75, 0.1])), ".*KFE": 1.0} if rng.random() < 0.7 else float(rng.choice([0.5, 1.0]))
            if rng.random() < 0.3:
                a["clip"] = None
            env["actions"][n] = a
        what.append("actions " + "+".join(keep_a))
    return fx, "; ".join(what)
