"""GPU: every observation, reward and termination op of the env step against the oracle run in float64 (tests/_step_cases.py), at the
env counts, cfgs and column widths that take each branch of k_action, k_term_rew + step_tail and the six k_obs* instantiations."""

import pytest

from _step_cases import FLAT, KITCHEN, ROUGH, run_case

pytestmark = pytest.mark.gpu

H3, MOD, NOISE, ACT, SHAPES = (FLAT + s for s in ("-hist3", "-mod", "-noise", "-actions", "-shapes"))
LEAN_V, LEAN_G, OBS_VL, OBS_VN, OBS_GL, OBS_GN = ("k_obs_lean<false>", "k_obs_lean<true>", "k_obs<false,true>", "k_obs<false,false>",
                                                   "k_obs<true,true>", "k_obs<true,false>")

# (task, N, step-tail mode, cfg variant, observation kernel).  Group size G: 16 up to 8192 envs, 32 up to 16384, 64 beyond; the
# single-wave kernel goes role-major for 2 <= N <= 8192.  Kitchen: two groups, 32 work items and 32 log entries (the tail's stride).
CASES = [
    (ROUGH, 1, "deferred", None, LEAN_V), (ROUGH, 2, "in_kernel", None, LEAN_V), (ROUGH, 15, "deferred", None, LEAN_V),
    (ROUGH, 16, "in_kernel", None, LEAN_V), (ROUGH, 8191, "deferred", None, LEAN_V), (ROUGH, 8192, "in_kernel", None, LEAN_V),
    (ROUGH, 8193, "deferred", None, LEAN_V), (ROUGH, 16385, "in_kernel", None, LEAN_V),
    (KITCHEN, 17, "deferred", None, OBS_VN), (KITCHEN, 63, "in_kernel", None, OBS_VN), (KITCHEN, 65, "deferred", None, OBS_VN),
    (KITCHEN, 16384, "in_kernel", None, OBS_VN), (KITCHEN, 8193, "deferred", None, OBS_VN),
    (FLAT, 64, "in_kernel", None, OBS_VL), (FLAT, 16384, "deferred", None, OBS_VL), (FLAT, 100_003, "deferred", None, OBS_VL),
    (FLAT, 100_003, "in_kernel", None, OBS_VL),
    ("Isaac-Cartpole-v0", 3, "deferred", None, OBS_VL), (H3, 65, "deferred", None, OBS_VN), (MOD, 63, "in_kernel", None, OBS_VN),
    (NOISE, 17, "deferred", None, OBS_VN), (ACT, 65, "deferred", None, OBS_VL), (SHAPES, 15, "in_kernel", None, OBS_VN),
    ("Isaac-Velocity-Rough-G1-v0", 63, "deferred", None, LEAN_V),
    (FLAT, 65, "deferred", "single_reward", OBS_VL), (FLAT, 2, "in_kernel", "single_reward", OBS_VL),
    (ROUGH, 64, "deferred", "tilted", LEAN_G), (ROUGH, 17, "in_kernel", "no_yaw", LEAN_G),
    (ROUGH, 16, "deferred", "wide_rays", OBS_GL), (KITCHEN, 17, "deferred", "tilted", OBS_GN),
] + [(FLAT, 17, "deferred", f"cols{w}", OBS_VL) for w in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)]


def _id(c):
    return f"{c[0].replace('Isaac-', '').replace('-v0', '')}-{c[1]}-{c[2]}" + (f"-{c[3]}" if c[3] else "")


def test_the_cases_cover_every_observation_kernel():
    assert {c[4] for c in CASES} == {LEAN_V, LEAN_G, OBS_VL, OBS_VN, OBS_GL, OBS_GN}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_step_terms_against_fp64(case):
    task, N, tail, kind, kernel = case
    check = {}
    seen = run_case(task, N, seed=N % 97, tail=tail, kind=kind, check=check)
    print(f"{_id(case)}: {check['kernel']} DC={check['DC']} G={check['G']} items={check['items']} resets={seen['resets']} near={seen['near']}")
    assert check["kernel"] == kernel, check["kernel"]
    if kind and kind.startswith("cols"):
        assert check["DC"] == int(kind[4:])
    if kind == "single_reward":
        assert check["items"] == 1  # NW = 2 waves for one work item
    if N < 64:
        return
    # non-vacuity: the edge pass put every decision on both sides, every weighted term is seen non-zero
    tot = N * seen["steps"]
    for name, v in seen["rew_nonzero"].items():
        assert v >= 0.01 * tot or v == 0 and _weight(task, kind, name) == 0.0, (name, v)
    for name in seen["term_true"]:
        assert seen["term_true"][name] > 0 and seen["term_false"][name] > 0, name
    assert min(seen["moving"]) > 0 and min(seen["first_contact"]) > 0
    assert seen["resets"] > 0 or kind == "single_reward"


def _weight(task, kind, name):
    from _step_cases import variant
    from isaaclab_amd.env import load_task_cfg

    return variant(load_task_cfg(task), kind)["env"]["rewards"][name]["weight"]
