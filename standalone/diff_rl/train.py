"""Train the racing policy by BPTT through the analytic step (reference: standalone/diff_rl/train.py:87-149).

    python standalone/diff_rl/train.py --task DiffLab-Quadcopter-CTBR-Racing-State-v0 --num_envs 4096 --headless

The task's `diff_rl_cfg_entry_point` gives the runner cfg (window of 48 steps, AdamW at 5e-4 under a cosine schedule,
MLP [256, 128]); the env is made with `is_differentiable_physics`, so every step also records a tape row and the
three differentiable losses, and each iteration closes with one reverse-time adjoint launch.  The env's periodic terrain
regeneration is switched off (the differentiable step is not built for the interval step; the env refuses the pair).  Logs go under
`logs/diff_rl/<experiment>/<time stamp>[_<run name>]/`.  `--torch_path` runs the torch autograd path instead of the
HIP kernels (the A/B baseline).  `--headless` and the other AppLauncher flags are accepted and ignored.
"""
from __future__ import annotations

import argparse
import os
import sys
from datetime import datetime

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cli_args  # noqa: E402  isort: skip


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train an RL agent with DIFF-RL.")
    p.add_argument("--video", action="store_true", default=False, help="Accepted; recording is rsl_rl/train.py's.")
    p.add_argument("--video_length", type=int, default=200)
    p.add_argument("--video_interval", type=int, default=2000)
    p.add_argument("--num_envs", type=int, default=None, help="Number of environments to simulate.")
    p.add_argument("--task", type=str, default=None, help="Name of the task.")
    p.add_argument("--seed", type=int, default=42, help="Seed used for the environment")
    p.add_argument("--max_iterations", type=int, default=None, help="Policy training iterations.")
    p.add_argument("--device", type=str, default=None, help="cuda:N")
    p.add_argument("--log_root", type=str, default="logs", help="Root of logs/diff_rl/<experiment>.")
    p.add_argument("--torch_path", action="store_true", default=False,
                   help="The torch autograd path of the tape instead of the HIP kernels (fused=False).")
    p.add_argument("--headless", action="store_true", default=False)
    p.add_argument("--enable_cameras", action="store_true", default=False)
    p.add_argument("--livestream", type=int, default=None)
    cli_args.add_rsl_rl_args(p)
    return p


def make_env(registry, task, agent_cfg, num_envs, device):
    """The task's env with the differentiable step on, its tape sized to the runner's window."""
    env_cfg = registry.load_cfg_from_registry(task, "env_cfg_entry_point")
    if getattr(env_cfg, "camera", None) is not None:
        raise NotImplementedError("the diff_rl workflow is built for the state task "
                                  "(DiffLab-Quadcopter-CTBR-Racing-State-v0): the vision policy under BPTT is not")
    if num_envs is not None:
        env_cfg.scene.num_envs = num_envs
    env_cfg.seed = agent_cfg.seed
    env_cfg.sim.device = device
    env_cfg.is_differentiable_physics = True
    if env_cfg.terrain.regen_interval_s is not None:
        print("[INFO] diff_rl: periodic terrain regeneration is off (the differentiable step is not built for it)")
        env_cfg.terrain.regen_interval_s = None
    env_cfg.diff_window = int(agent_cfg.num_steps_per_env)
    env_cfg.diff_fused = bool(agent_cfg.fused)
    return registry.make(task, cfg=env_cfg), env_cfg


def main(argv=None):
    args, _unknown = build_parser().parse_known_args(argv)
    import importlib

    import torch
    import yaml

    registry = importlib.import_module("generalizableracing_amd.registry")
    from generalizableracing_amd.diff_rl import AlgoRunner
    from generalizableracing_amd.envs.racing_env import RslRlVecEnvWrapper

    task = args.task or "DiffLab-Quadcopter-CTBR-Racing-State-v0"
    agent_cfg = registry.load_cfg_from_registry(task, "diff_rl_cfg_entry_point")
    agent_cfg = cli_args.update_rsl_rl_cfg(agent_cfg, args)
    if args.max_iterations is not None:
        agent_cfg.max_iterations = args.max_iterations
    if args.torch_path:
        agent_cfg.fused = False
    device = args.device or "cuda:0"
    agent_cfg.device = device
    log_root_path = os.path.abspath(os.path.join(args.log_root, "diff_rl", agent_cfg.experiment_name))
    print(f"[INFO] Logging experiment in directory: {log_root_path}")
    log_dir = datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
    if agent_cfg.run_name:
        log_dir += f"_{agent_cfg.run_name}"
    log_dir = os.path.join(log_root_path, log_dir)
    torch.manual_seed(args.seed)
    env, env_cfg = make_env(registry, task, agent_cfg, args.num_envs, device)
    env = RslRlVecEnvWrapper(env)
    runner = AlgoRunner(env, agent_cfg.to_dict(), log_dir=log_dir, device=device)
    if agent_cfg.resume:
        resume_path = cli_args.get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)
        print(f"[INFO]: Loading model checkpoint from: {resume_path}")
        runner.load(resume_path)
    os.makedirs(os.path.join(log_dir, "params"), exist_ok=True)
    from dataclasses import asdict

    with open(os.path.join(log_dir, "params", "env.yaml"), "w") as f:
        yaml.safe_dump(asdict(env_cfg), f)
    with open(os.path.join(log_dir, "params", "agent.yaml"), "w") as f:
        yaml.safe_dump(agent_cfg.to_dict(), f)
    runner.learn(num_learning_iterations=agent_cfg.max_iterations,
                 init_at_random_ep_len=agent_cfg.init_at_random_ep_len)
    env.close()
    return log_dir


if __name__ == "__main__":
    main()
