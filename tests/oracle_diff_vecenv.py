"""Test-only differentiable VecEnv backed by the CPU oracle: OracleVecEnv plus the tape of the diff_rl workflow through
the torch path of generalizableracing_amd.diff_rl.diff_ops (record before the step from the oracle's env fields, loss
after it from the post-step gate id / level / type and the host gate table), with RacingEnv's surface: extras
"losses" / "losses_detached" / "log_losses", detach(), loss_action_grad()."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from generalizableracing_amd import _abi
from generalizableracing_amd.diff_rl.diff_ops import LOSS_TERMS, DiffTape
from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg, SceneCfg, SimCfg, TerrainCfg
from generalizableracing_amd.envs.tracks import build_tracks
from oracle_vecenv import OracleVecEnv


class OracleDiffVecEnv(OracleVecEnv):
    def __init__(self, num_envs=16, stage=1, lag=1, t_max=48, seed=42, types=4, levels=10, dtype=torch.float64,
                 weights=(1.0, 0.05, 0.5), gamma=0.92, episode_length_s=None):
        super().__init__(num_envs=num_envs, stage=stage, seed=seed, types=types, levels=levels)
        self.cfg = RacingEnvCfg(scene=SceneCfg(num_envs=num_envs), sim=SimCfg(device="cpu"), stage=stage,
                                terrain=TerrainCfg(num_cols=types, num_rows=levels), seed=seed,
                                episode_length_s=episode_length_s, overrides=dict(action_lag=lag), is_differentiable_physics=True, diff_window=t_max,
                                diff_fused=False)
        c = self.cfg.to_gr_config()
        gates, recs, ot = build_tracks(num_types=types, num_levels=levels, num_gates=8, seed=42)
        self.gates = torch.from_numpy(gates)
        self.orc = oracle.Oracle(c, gates, recs, ot.records, ot.counts)
        self.orc.init()
        self.orc.reset(None)
        self.gr_config = c
        self.max_episode_length = self.cfg.max_episode_length
        # the lag buffer in the tape's dtype: tanh(a_{t-1}) as the float64 window sees it (the oracle's own lag plane
        # holds its float32 rounding), so float64 comparisons of the window are exact to rounding
        self._u_prev = None
        self.diff = DiffTape(None, c, t_max, "cpu", fused=False, weights=weights, gamma=gamma, dtype=dtype)

    def planes(self):
        state, istate = oracle.envs_to_planes(self.orc.envs)
        return torch.from_numpy(state), torch.from_numpy(istate)

    def step(self, actions: torch.Tensor):
        self.diff.check_room()
        state, _ = self.planes()
        u = self._u_prev if (self.gr_config.action_lag and self.diff.tape.dtype == torch.float64) else None
        self.diff.record(state, actions.detach(), u)
        self._u_prev = torch.tanh(actions.detach().to(self.diff.tape.dtype))
        obs, rew, dones, extras = super().step(actions)
        _, istate = self.planes()
        losses, terms = self.diff.loss(self.gates, istate[:, _abi.I_PACKED], dones)
        extras["losses"] = losses.to(torch.float32)
        extras["losses_detached"] = torch.zeros_like(extras["losses"])
        extras["log_losses"] = {k: terms[:, j].mean() for j, k in enumerate(LOSS_TERMS)}
        return obs, rew, dones, extras

    def detach(self):
        self.diff.rewind()

    def loss_action_grad(self, scale=None):
        T = self.diff.cursor
        return self.diff.backward(1.0 / (max(T, 1) * self.num_envs) if scale is None else float(scale))
