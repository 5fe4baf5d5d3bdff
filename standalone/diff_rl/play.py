"""Play a checkpoint of the diff_rl workflow (reference: standalone/diff_rl/play.py): load the latest (or the given)
checkpoint under logs/diff_rl/<experiment>/ and step the env with the policy's mean action.

    python standalone/diff_rl/play.py --task DiffLab-Quadcopter-CTBR-Racing-State-v0 --num_envs 64 --steps 200
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cli_args  # noqa: E402  isort: skip


def main(argv=None):
    p = argparse.ArgumentParser(description="Play a DIFF-RL checkpoint.")
    p.add_argument("--num_envs", type=int, default=None)
    p.add_argument("--task", type=str, default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--log_root", type=str, default="logs")
    p.add_argument("--steps", type=int, default=200, help="Env steps to play.")
    p.add_argument("--headless", action="store_true", default=False)
    cli_args.add_rsl_rl_args(p)
    args, _unknown = p.parse_known_args(argv)
    import importlib

    import torch

    registry = importlib.import_module("generalizableracing_amd.registry")
    from generalizableracing_amd.diff_rl import AlgoRunner
    from generalizableracing_amd.envs.racing_env import RslRlVecEnvWrapper

    task = args.task or "DiffLab-Quadcopter-CTBR-Racing-State-v0"
    agent_cfg = cli_args.update_rsl_rl_cfg(registry.load_cfg_from_registry(task, "diff_rl_cfg_entry_point"), args)
    device = args.device or "cuda:0"
    env_cfg = registry.load_cfg_from_registry(task, "env_cfg_entry_point")
    if args.num_envs is not None:
        env_cfg.scene.num_envs = args.num_envs
    env_cfg.seed = agent_cfg.seed
    env_cfg.sim.device = device
    env = RslRlVecEnvWrapper(registry.make(task, cfg=env_cfg))
    log_root_path = os.path.abspath(os.path.join(args.log_root, "diff_rl", agent_cfg.experiment_name))
    resume_path = cli_args.get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)
    print(f"[INFO]: Loading model checkpoint from: {resume_path}")
    runner = AlgoRunner(env, agent_cfg.to_dict(), log_dir=None, device=device)
    runner.load(resume_path, load_optimizer=False)
    policy = runner.get_inference_policy(device=device)
    obs, _ = env.get_observations()
    total = torch.zeros((), device=device)
    with torch.inference_mode():
        for _ in range(args.steps):
            obs, rew, _, _ = env.step(policy(obs))
            total += rew.mean()
    print(f"[INFO]: played {args.steps} steps, mean reward per step {float(total) / max(args.steps, 1):.4f}")
    env.close()


if __name__ == "__main__":
    main()
