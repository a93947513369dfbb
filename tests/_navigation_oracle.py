"""A torch restatement, in fp32 or fp64, of what the navigation task computes on the torch side of the reference: the low-level step of
``PreTrainedPolicyAction`` (isaaclab_tasks .../navigation/mdp/pre_trained_policy_action.py:53-100: the masked zero, the low-level
observation group term by term through noise -> clip -> scale, the policy MLP, ``JointPositionAction.process_actions``) and the env
step's observation, reward and termination terms of ``NavigationEnvCfg``.  Written from the reference's formulas, driven by the cfg dict
alone (no plan, no kernel); tools/gen_golden_navigation.py holds the REAL classes to it, the tests hold the kernels to it."""

from __future__ import annotations

import math

import torch

from isaaclab_amd.robots import resolve_matching_names, resolve_matching_names_values


def up(x, dtype):
    return x.to(dtype) if x.is_floating_point() else x


def quat_rotate_inverse(q, v):  # isaaclab/utils/math.py:605-625
    w, xyz = q[:, 0], q[:, 1:]
    a = v * (2.0 * w ** 2 - 1.0).unsqueeze(-1)
    b = torch.cross(xyz, v, dim=-1) * w.unsqueeze(-1) * 2.0
    c = xyz * torch.bmm(xyz.view(-1, 1, 3), v.view(-1, 3, 1)).squeeze(-1) * 2.0
    return a - b + c


class LowLevelOracle:
    """One ``PreTrainedPolicyAction`` over a robot's name tables.  ``term_cfg``: the action term's cfg dict (``low_level_observations``,
    ``low_level_actions``, ``low_level_decimation``); ``layers``: ``[(W, b)]`` of the policy, ``alpha`` its ELU alpha."""

    def __init__(self, term_cfg: dict, joint_names, layers, alpha: float = 1.0, gravity_dir=(0.0, 0.0, -1.0), dtype=torch.float32):
        self.dtype, self.joint_names = dtype, list(joint_names)
        self.group = term_cfg["low_level_observations"]
        self.corrupt = bool(self.group.get("enable_corruption", False))
        self.terms = [(n, c) for n, c in self.group.items() if isinstance(c, dict) and "func" in c]
        self.layers = [(torch.as_tensor(w).to(dtype), torch.as_tensor(b).to(dtype)) for w, b in layers]
        self.alpha = float(alpha)
        self.low_level_decimation = int(term_cfg.get("low_level_decimation", 4))
        self.gravity = torch.tensor(gravity_dir, dtype=dtype)
        a = term_cfg["low_level_actions"]
        assert str(a["class_type"]).endswith("JointPositionAction")
        self.act_ids, names = resolve_matching_names(a["joint_names"], self.joint_names, bool(a.get("preserve_order")))
        n = len(self.act_ids)
        self.scale = a.get("scale", 1.0)
        if isinstance(self.scale, dict):  # joint_actions.py:78-86: a tensor of ones with the matched entries set
            s = torch.ones(n, dtype=dtype)
            idx, _, vals = resolve_matching_names_values(self.scale, names)
            s[idx] = torch.tensor(vals, dtype=torch.float32).to(dtype)  # (the reference's tensor is fp32)
            self.scale = s
        self.use_default_offset = bool(a.get("use_default_offset", True))
        self.offset = a.get("offset", 0.0)
        self.clip = None
        if a.get("clip") is not None:  # :99-110
            c = torch.tensor([[-math.inf, math.inf]], dtype=dtype).repeat(n, 1)
            idx, _, vals = resolve_matching_names_values(a["clip"], names)
            c[idx] = torch.tensor(vals, dtype=torch.float32).to(dtype)
            self.clip = c
        self.counter = 0

    # ---- the group's width and term columns
    def term_width(self, name: str, cfg: dict, A: int) -> int:
        fn = str(cfg["func"]).rpartition(":")[2]
        if name == "actions":
            return A
        if name == "velocity_commands" or fn in ("base_lin_vel", "base_ang_vel", "projected_gravity"):
            return 3
        return len(self._jids(cfg))

    def _jids(self, cfg: dict):
        ent = (cfg.get("params") or {}).get("asset_cfg") or {}
        names = ent.get("joint_names")
        return list(range(len(self.joint_names))) if names is None else resolve_matching_names(names, self.joint_names, bool(ent.get("preserve_order")))[0]

    @property
    def obs_dim(self) -> int:
        return sum(self.term_width(n, c, len(self.act_ids)) for n, c in self.terms)

    def _value(self, name: str, cfg: dict, st: dict, raw, lla):
        if name == "actions":  # (remapped by the term, :63-64)
            return lla
        if name == "velocity_commands":  # (:65-66)
            return raw
        fn = str(cfg["func"]).rpartition(":")[2]
        q = st["root_quat_w"]
        if fn == "base_lin_vel":
            return quat_rotate_inverse(q, st["root_lin_vel_w"])
        if fn == "base_ang_vel":
            return quat_rotate_inverse(q, st["root_ang_vel_w"])
        if fn == "projected_gravity":
            return quat_rotate_inverse(q, self.gravity.expand(q.shape[0], 3))
        ids = self._jids(cfg)
        if fn == "joint_pos_rel":
            return st["joint_pos"][:, ids] - st["default_joint_pos"][:, ids]
        if fn == "joint_vel_rel":
            return st["joint_vel"][:, ids] - st["default_joint_vel"][:, ids]
        if fn == "joint_pos":
            return st["joint_pos"][:, ids]
        if fn == "joint_vel":
            return st["joint_vel"][:, ids]
        raise NotImplementedError(fn)

    def observations(self, st: dict, raw, lla, noise_u=None):
        """ObservationManager.compute_group (observation_manager.py:260-335): per term value -> noise -> clip -> scale; ``noise_u``: the
        (N, D) uniforms behind every ``rand_like``, one column per observation column."""
        out, col = [], 0
        for name, cfg in self.terms:
            v = self._value(name, cfg, st, raw, lla).clone()
            w = v.shape[1]
            noise = cfg.get("noise")
            if noise and self.corrupt:
                assert str(noise["func"]).endswith("uniform_noise") and noise.get("operation", "add") == "add"
                u = noise_u[:, col:col + w].to(self.dtype)
                v = v + u * (noise["n_max"] - noise["n_min"]) + noise["n_min"]  # noise_model.py:62-64
            if cfg.get("clip") is not None:
                v = v.clip(min=cfg["clip"][0], max=cfg["clip"][1])
            if cfg.get("scale") is not None:
                v = v * cfg["scale"]
            out.append(v)
            col += w
        return torch.cat(out, dim=-1)

    def policy(self, x):
        for i, (w, b) in enumerate(self.layers):
            x = torch.nn.functional.linear(x, w, b)
            if i + 1 < len(self.layers):
                x = torch.nn.functional.elu(x, alpha=self.alpha)
        return x

    def low_level_step(self, st: dict, raw, lla, episode_length_buf, noise_u=None):
        """pre_trained_policy_action.py:53-57 and :95-97 -> (observation rows, low_level_actions, joint position targets)."""
        st = {k: up(torch.as_tensor(v), self.dtype) for k, v in st.items()}
        lla = up(lla, self.dtype).clone()
        lla[episode_length_buf == 0, :] = 0
        obs = self.observations(st, up(raw, self.dtype), lla, noise_u)
        lla = self.policy(obs)
        offset = st["default_joint_pos"][:, self.act_ids] if self.use_default_offset else self.offset
        target = lla * self.scale + offset  # joint_actions.py:130-139
        if self.clip is not None:
            target = torch.clamp(target, min=self.clip[:, 0], max=self.clip[:, 1])
        return obs, lla, target

    def launches(self, decimation: int) -> int:
        """How many of the next ``decimation`` apply_actions calls run a low-level step (:94-100), advancing the counter."""
        n = 0
        for _ in range(decimation):
            if self.counter % self.low_level_decimation == 0:
                n += 1
                self.counter = 0
            self.counter += 1
        return n


# ---- the env step of NavigationEnvCfg (navigation_env_cfg.py) on one state: observations, terminations, rewards
def policy_observation(st: dict, gravity_dir=(0.0, 0.0, -1.0), dtype=torch.float32):
    """PolicyCfg: base_lin_vel 3, projected_gravity 3, pose_command 4 (no noise)."""
    q = up(st["root_quat_w"], dtype)
    g = torch.tensor(gravity_dir, dtype=dtype).expand(q.shape[0], 3)
    return torch.cat([quat_rotate_inverse(q, up(st["root_lin_vel_w"], dtype)), quat_rotate_inverse(q, g), up(st["command"], dtype)], dim=-1)


def terminations(st: dict, episode_length_buf, max_episode_length: int, base_ids, threshold: float, dtype=torch.float32):
    """time_out (terminations.py:25-30) and illegal_contact on the base (:150-160) -> (time_outs, base_contact)."""
    f = up(st["net_forces_w_history"], dtype)
    contact = torch.any(torch.max(torch.norm(f[:, :, base_ids], dim=-1), dim=1)[0] > threshold, dim=1)
    return episode_length_buf >= max_episode_length, contact


def rewards(cfg_rewards: dict, st: dict, terminated, dt: float, dtype=torch.float32):
    """RewardManager.compute (reward_manager.py:128-157) over the cfg's terms -> (reward, per-term value / dt)."""
    cmd = up(st["command"], dtype)
    total, terms = torch.zeros(cmd.shape[0], dtype=dtype), []
    for name, c in cfg_rewards.items():
        if c is None:
            continue
        fn, p = str(c["func"]).rpartition(":")[2], c.get("params") or {}
        if fn == "is_terminated":
            f = terminated.to(dtype)
        elif fn == "position_command_error_tanh":  # navigation/mdp/rewards.py:17-22
            f = 1 - torch.tanh(torch.norm(cmd[:, :3], dim=1) / p["std"])
        elif fn == "heading_command_error_abs":  # :25-29
            f = cmd[:, 3].abs()
        else:
            raise NotImplementedError(fn)
        value = f * c["weight"] * dt
        total = total + value
        terms.append(value / dt)
    return total, torch.stack(terms, dim=1)
