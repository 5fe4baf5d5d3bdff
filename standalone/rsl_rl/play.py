"""Play a trained checkpoint on the HIP env (reference: standalone/rsl_rl/play.py:60-151).

Same flow as the reference: resolve the checkpoint from logs/rsl_rl/<experiment>/<run>/model_*.pt,
build the env and the runner, load, export the policy next to the checkpoint (exported/), then step
the env with the inference policy.  There is no simulator window: the loop runs --max_steps steps
(the reference runs until the app closes) and prints a JSON summary; --show_camera writes env 0's
depth image as PGM frames instead of an OpenCV window; --video records the first --video_length steps from the
HIP viewer's chase camera as `<checkpoint dir>/videos/play/rl-video-step-0.gif` (reference play.py: RecordVideo with
a trigger at step 0).

    python standalone/rsl_rl/play.py --task DiffLab-Quadcopter-CTBR-Racing-v0 --num_envs 64
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cli_args  # noqa: E402  isort: skip
from train import get_checkpoint_path  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Play an RL agent with RSL-RL.")
    p.add_argument("--video", action="store_true", default=False, help="Record a video of the first steps.")
    p.add_argument("--video_length", type=int, default=200, help="Length of the recorded video (in steps).")
    p.add_argument("--video_env", type=int, default=0, help="Index of the env the viewer follows.")
    p.add_argument("--video_size", type=str, default="640x480", help="Frame size of the video, WxH.")
    p.add_argument("--disable_fabric", action="store_true", default=False, help="(ignored)")
    p.add_argument("--num_envs", type=int, default=None)
    p.add_argument("--task", type=str, default=None)
    p.add_argument("--show_camera", action="store_true", default=False,
                   help="write env 0's depth image every 10 steps as PGM under the checkpoint dir")
    p.add_argument("--max_steps", type=int, default=1000, help="steps to play (no app window to close)")
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--log_root", type=str, default="logs")
    p.add_argument("--agent", type=str, default="rsl_rl_cfg_entry_point")
    p.add_argument("--headless", action="store_true", default=False)
    p.add_argument("--enable_cameras", action="store_true", default=False)
    cli_args.add_rsl_rl_args(p)
    return p


def _write_pgm(path, img):
    import numpy as np

    a = (np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(f"P5 {a.shape[1]} {a.shape[0]} 255\n".encode())
        f.write(a.tobytes())


def main(argv=None):
    args, _ = build_parser().parse_known_args(argv)
    import importlib

    import torch

    registry = importlib.import_module("generalizableracing_amd.registry")
    from generalizableracing_amd.envs.racing_env import RslRlVecEnvWrapper
    from generalizableracing_amd.rsl_rl import OnPolicyRunner, VisionActorCritic
    from generalizableracing_amd.rsl_rl import exporter

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
    resume_path = get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)

    if args.video:
        from generalizableracing_amd.envs.record_video import RecordVideo
        from generalizableracing_amd.envs.viewer import ViewerCfg, parse_size

        vw, vh = parse_size(args.video_size)
        env = registry.make(task, cfg=env_cfg, render_mode="rgb_array",
                            viewer=ViewerCfg(width=vw, height=vh, env_id=args.video_env))
        print("[INFO] Recording videos during play.")
        env = RecordVideo(env, video_folder=os.path.join(os.path.dirname(resume_path), "videos", "play"),
                          step_trigger=lambda step: step == 0, video_length=args.video_length)
    else:
        env = registry.make(task, cfg=env_cfg)
    env = RslRlVecEnvWrapper(env)
    print(f"[INFO]: Loading model checkpoint from: {resume_path}")
    runner = OnPolicyRunner(env, agent_cfg.to_dict(), log_dir=None, device=device)
    runner.load(resume_path)
    policy = runner.get_inference_policy(device=device)

    # export (play.py:100-118): TorchScript here; ONNX where the `onnx` package exists
    export_dir = os.path.join(os.path.dirname(resume_path), "exported")
    pol_mod = runner.alg.policy
    norm = runner.obs_normalizer
    exported = {}
    if isinstance(pol_mod, VisionActorCritic) and not pol_mod.is_recurrent:
        exported["jit"] = exporter.export_vision_policy_as_jit(pol_mod, export_dir, norm, "vision_policy.pt")
        onnx_fn = lambda: exporter.export_vision_policy_as_onnx(  # noqa: E731
            pol_mod, export_dir, norm, "vision_policy.onnx", False, pol_mod.img_res, (16,))
    else:
        exported["jit"] = exporter.export_policy_as_jit(pol_mod, norm, export_dir, "policy.pt")
        onnx_fn = lambda: exporter.export_policy_as_onnx(pol_mod, export_dir, norm, "policy.onnx")  # noqa: E731
    try:
        exported["onnx"] = onnx_fn()
    except RuntimeError as e:
        exported["onnx"] = f"skipped: {e}"

    obs, _ = env.get_observations()
    n = env.num_envs
    ret = torch.zeros(n, device=device)
    done_ret, done_cnt = 0.0, 0
    for t in range(args.max_steps):
        with torch.inference_mode():
            out = policy(obs)
            actions = out[0] if isinstance(out, tuple) else out
            obs, rew, dones, _ = env.step(actions)
            if pol_mod.is_recurrent:  # finished envs restart from a zero memory
                pol_mod.reset(dones)
            ret += rew
            d = dones.bool()
            if bool(d.any()):
                done_ret += float(ret[d].sum())
                done_cnt += int(d.sum())
                ret[d] = 0
        if args.show_camera and getattr(env.unwrapped, "camera", None) is not None and t % 10 == 0:
            cam_dir = os.path.join(os.path.dirname(resume_path), "camera")
            os.makedirs(cam_dir, exist_ok=True)
            c = env.unwrapped.camera
            img = (env.unwrapped.depth[0] / c.max_distance).reshape(c.height, c.width).cpu().numpy()
            _write_pgm(os.path.join(cam_dir, f"depth_{t:05d}.pgm"), img)
    summary = {"checkpoint": resume_path, "steps": args.max_steps, "num_envs": n, "episodes": done_cnt,
               "mean_episode_return": done_ret / max(done_cnt, 1), "exported": exported}
    print(json.dumps(summary))
    env.close()
    return summary


if __name__ == "__main__":
    main()
