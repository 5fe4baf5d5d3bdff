"""The BPTT iteration, fused tape kernels against the torch path -> profiles/bptt_iteration_ab.json.

    python scripts/time_bptt.py                      # A/B at 4 096 and 65 536 envs, T = 48, alternated in one process
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_bptt.py --profile
                                                     # the three kernels' times, in a run of its own (fused only)
    python scripts/time_bptt.py --learn 300          # a learning run -> profiles/bptt_learning_curve.json

One iteration = env.detach(), T = 48 steps of (policy act, record, gr_step, loss), then the update (the adjoint, one
batched policy forward / backward over the T * N rows, AdamW).  `fused=True`: the three HIP kernels of gr_diff.hip;
`fused=False` (the baseline, the reference's structure, not the code under test): the record and loss in torch ops
per step and the adjoint by torch autograd over the window's graph.  Host clock around work that ends in a device
synchronise; both paths warmed up, then alternated.  The adjoint kernel's HBM traffic is counted from shapes: per
env-step 16 tape planes of 16 B read and one 16 B gradient row written.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from generalizableracing_amd.diff_rl import AlgoRunner, QuadcopterDiffRLRunnerCfg  # noqa: E402
from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg, SceneCfg, SimCfg, TerrainCfg  # noqa: E402
from generalizableracing_amd.envs.racing_env import RacingEnv, RslRlVecEnvWrapper  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM bandwidth
ADJOINT_BYTES_PER_ENV_STEP = 16 * 16 + 16


def make_runner(n, T, fused, iters, log_dir=None, seed=42):
    torch.manual_seed(seed)
    env = RacingEnv(RacingEnvCfg(scene=SceneCfg(num_envs=n), sim=SimCfg(device=DEV), seed=seed,
                                 terrain=TerrainCfg(regen_interval_s=None),
                                 is_differentiable_physics=True, diff_window=T, diff_fused=fused))
    cfg = QuadcopterDiffRLRunnerCfg(num_steps_per_env=T, max_iterations=iters, device=DEV, fused=fused,
                                    save_interval=10 ** 9)
    return AlgoRunner(RslRlVecEnvWrapper(env), cfg.to_dict(), log_dir=log_dir, device=DEV)


def iteration(runner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runner.learn(1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ab(n, T, reps):
    a, b = make_runner(n, T, True, 10 ** 6), make_runner(n, T, False, 10 ** 6)
    for r in (a, b):
        iteration(r)
        iteration(r)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(iteration(a))
        tb.append(iteration(b))
    # the adjoint launch alone, device events
    env = a.env.unwrapped
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    env.loss_action_grad()
    ev[0].record()
    for _ in range(20):
        env.loss_action_grad()
    ev[1].record()
    torch.cuda.synchronize()
    adj_s = ev[0].elapsed_time(ev[1]) * 1e-3 / 20
    nbytes = ADJOINT_BYTES_PER_ENV_STEP * n * env.diff_steps
    out = {"num_envs": n, "T": T, "reps": reps, "fused_s": sorted(ta), "torch_s": sorted(tb),
           "fused_median_s": sorted(ta)[len(ta) // 2], "torch_median_s": sorted(tb)[len(tb) // 2],
           "adjoint_launch_s": adj_s, "adjoint_steps": env.diff_steps, "adjoint_bytes": nbytes,
           "adjoint_hbm_bound_s": nbytes / HBM_BYTES_PER_S, "adjoint_share_of_hbm_bound": nbytes / HBM_BYTES_PER_S / adj_s}
    out["speedup"] = out["torch_median_s"] / out["fused_median_s"]
    for r in (a, b):
        r.env.close()
    return out


def learn(iters, n, T, out_path):
    runner = make_runner(n, T, True, iters, log_dir=os.path.join(ROOT, "logs", "diff_rl", "bptt_learn"))
    env = runner.env.unwrapped
    runner.log_history = []
    runner.learn(iters, init_at_random_ep_len=True)
    curve = []
    for it, log in enumerate(runner.log_history):
        curve.append({"it": it, "Loss/policy": log.get("Loss/policy"),
                      "Train/mean_loss_total": log.get("Train/mean_loss_total"),
                      "Train/mean_reward": log.get("Train/mean_reward"),
                      "Train/mean_episode_length": log.get("Train/mean_episode_length"),
                      "gates_per_episode": log.get("Metrics/next_gate_pose/accumulate_gates")})
    keep = curve[:20] + curve[-20:] if iters > 40 else curve
    with open(out_path, "w") as f:
        json.dump({"num_envs": n, "T": T, "iterations": iters, "stage": env.cfg.stage,
                   "note": "Loss/policy is the window's mean loss per env-step; Train/* are episode means", "curve": keep},
                  f, indent=1)
        f.write("\n")
    print(json.dumps(keep[:2] + keep[-2:]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--profile", action="store_true")
    p.add_argument("--learn", type=int, default=0)
    p.add_argument("--envs", type=int, nargs="*", default=[4096, 65536])
    p.add_argument("--T", type=int, default=48)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "timings need the GPU"
    if args.profile:
        r = make_runner(args.envs[0], args.T, True, 10 ** 6)
        for _ in range(6):
            iteration(r)
        return
    if args.learn:
        learn(args.learn, args.envs[0], args.T, args.out or os.path.join(ROOT, "profiles", "bptt_learning_curve.json"))
        return
    res = [ab(n, args.T, args.reps) for n in args.envs]
    with open(args.out or os.path.join(ROOT, "profiles", "bptt_iteration_ab.json"), "w") as f:
        json.dump({"what": "BPTT iteration time, fused tape kernels vs the torch path, alternated in one process",
                   "results": res}, f, indent=1)
        f.write("\n")
    for r in res:
        print(json.dumps({k: r[k] for k in ("num_envs", "fused_median_s", "torch_median_s", "speedup",
                                            "adjoint_launch_s", "adjoint_share_of_hbm_bound")}))


if __name__ == "__main__":
    main()
