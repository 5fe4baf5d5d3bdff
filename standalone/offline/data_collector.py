"""Play a trained checkpoint and collect the auxiliary head's dataset (reference: standalone/offline/data_collector.py).

The reference's flow: resolve and load the checkpoint as play.py does, then loop policy(obs) -> (actions, feature),
env.step, and store the feature of every env whose auxiliary label (infos["observations"]["auxiliary"], "crossing a
gate now") is set plus as many unset ones, until N_positive + N_negative rows are written.  Here the dataset stays on
the device (generalizableracing_amd.offline.FeatureCollector: one gr_offline_collect call per step, no read-back);
the row count is polled every 32 steps and the loop ends when the dataset is full or after --max_steps.

    python standalone/offline/data_collector.py --num_envs 4096 --dataset racing_data --num_samples 2000000

writes racing_data/features.npy and racing_data/supervision.npy (an .h5 path where h5py is installed) and prints a
JSON summary.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "standalone", "rsl_rl"))

import cli_args  # noqa: E402  isort: skip
import play  # noqa: E402  (its argument parser and checkpoint lookup)

POLL_STEPS = 32  # steps between reads of the device row count (the loop's only synchronisation)


def build_parser():
    p = play.build_parser()
    p.description = "Collect the auxiliary head's dataset with an RSL-RL agent."
    p.add_argument("--dataset", type=str, default="racing_data", help="dataset directory (or an .h5 file with h5py)")
    p.add_argument("--num_samples", type=int, default=2000000, help="rows to collect (N_positive + N_negative)")
    p.set_defaults(max_steps=1000000)
    return p


def main(argv=None, hook=None):
    """hook(feat, aux), when given, sees every step's feature and label tensors (tests record them)."""
    args, _ = build_parser().parse_known_args(argv)
    import importlib

    import torch

    registry = importlib.import_module("generalizableracing_amd.registry")
    from generalizableracing_amd.envs.racing_env import RslRlVecEnvWrapper
    from generalizableracing_amd.offline import FeatureCollector
    from generalizableracing_amd.rsl_rl import OnPolicyRunner

    task = args.task or "DiffLab-Quadcopter-CTBR-Racing-v0"
    env_cfg = registry.load_cfg_from_registry(task, "env_cfg_entry_point")
    agent_cfg = cli_args.update_rsl_rl_cfg(registry.load_cfg_from_registry(task, args.agent), args)
    if args.num_envs is not None:
        env_cfg.scene.num_envs = args.num_envs
    device = args.device or "cuda:0"
    agent_cfg.device = device
    env_cfg.sim.device = device

    log_root_path = os.path.abspath(os.path.join(args.log_root, "rsl_rl", agent_cfg.experiment_name))
    print(f"[INFO] Loading experiment from directory: {log_root_path}")
    resume_path = play.get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)

    env = RslRlVecEnvWrapper(registry.make(task, cfg=env_cfg))
    print(f"[INFO]: Loading model checkpoint from: {resume_path}")
    runner = OnPolicyRunner(env, agent_cfg.to_dict(), log_dir=None, device=device)
    runner.load(resume_path)
    if not hasattr(runner.alg.policy, "aux_decoder"):
        raise SystemExit(f"the policy of {task} has no auxiliary head: nothing to collect for")
    policy = runner.get_inference_policy(device=device)

    collector = FeatureCollector(args.num_samples, runner.alg.policy.aux_decoder.in_features, device)
    obs, _ = env.get_observations()
    steps = 0
    with torch.inference_mode():
        while steps < args.max_steps:
            actions, feat = policy(obs)
            obs, _, _, infos = env.step(actions)
            aux = infos["observations"]["auxiliary"]
            if hook is not None:
                hook(feat, aux)
            collector.add(feat, aux)
            steps += 1
            if steps % POLL_STEPS == 0 and collector.full():
                print("[INFO] The dataset is full, stopping data collection.")
                break
    rows, positives, negatives = collector.counts()
    collector.save(args.dataset)
    summary = {"checkpoint": resume_path, "dataset": os.path.abspath(args.dataset), "rows": rows,
               "positives": positives, "negatives": negatives, "steps": steps, "num_envs": env.num_envs}
    print(json.dumps(summary))
    env.close()
    return summary


if __name__ == "__main__":
    main()
