"""Shared by the diff_rl tests and scripts/bptt_error_budget.py: the window shapes, the forced resets, the per-env
error of an action gradient, and the window driven on the CPU oracle."""
from __future__ import annotations

import json
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_FILE = os.path.join(ROOT, "profiles", "bptt_error_budget.json")
SHAPES = ((1, 1), (2, 65), (7, 321), (48, 64))   # (T, N): one lane; a wave + 1; a block tail and a wave tail; the recipe's T
BPTT_SHAPE = (8, 256, 1)                         # (T, N, lag) of tests/test_gpu_bptt.py's iteration
FORCED = ((0, 0), (3, 64), (5, 320))             # (step, env) timed out through episode_length_buf
BOUND_FACTOR = 4.0


def forced_resets(T: int, N: int):
    """The forced (step, env) pairs clipped to the window."""
    return [(t, min(e, N - 1)) for t, e in FORCED if t < T]


def force_timeouts(env, t: int, T: int, N: int):
    """Before step t: the forced envs' episode length one short of the limit, so the step times them out."""
    hit = [e for tt, e in forced_resets(T, N) if tt == t]
    if hit:
        buf = env.episode_length_buf.clone()
        buf[hit] = int(env.max_episode_length) - 1
        env.episode_length_buf = buf


def per_env_error(G: torch.Tensor, G_ref: torch.Tensor):
    """||dG[:, n, :]|| / ||G_ref[:, n, :]|| per env -> (errors of the envs whose reference is non-zero, mask of them);
    where the reference is exactly zero the gradient must be too (checked by the caller)."""
    d = (G.double() - G_ref.double()).permute(1, 0, 2).flatten(1).norm(dim=1)
    r = G_ref.double().permute(1, 0, 2).flatten(1).norm(dim=1)
    nz = r > 0
    return d[nz] / r[nz], nz


def budget() -> dict:
    with open(BUDGET_FILE) as f:
        return json.load(f)


def case_bound(T: int, N: int, lag: int) -> float:
    """BOUND_FACTOR x the case's own measured fp32 floor (profiles/bptt_error_budget.json)."""
    for c in budget()["cases"]:
        if (c["T"], c["N"], c["lag"]) == (T, N, lag):
            return BOUND_FACTOR * c["max_rel_err_per_env"]
    raise KeyError((T, N, lag))


def oracle_window(T: int, N: int, lag: int, seed: int, dtype=torch.float32):
    """A window of N(0, 1) actions with the forced resets on the CPU oracle through the torch path -> the env."""
    from oracle_diff_vecenv import OracleDiffVecEnv

    env = OracleDiffVecEnv(num_envs=N, lag=lag, t_max=T, dtype=dtype, types=min(4, N), seed=42 + seed)
    g = torch.Generator().manual_seed(seed)
    env.detach()
    for t in range(T):
        force_timeouts(env, t, T, N)
        env.step(torch.randn(N, 4, generator=g))
    return env
