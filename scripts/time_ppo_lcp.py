"""Time one C2 mini-batch step (24 576 rows, MLP 256 x 256, 16 observations, 4 actions) of the update with and
without PPOLCP's gradient penalty:

    ppo_eager / ppo_graphed        plain PPO on the fused losses + whole-network MLP kernels (the baseline)
    lcp_torch                      PPOLCP on the torch path (double backward through F.linear; fused ops off)
    lcp_fused / lcp_fused_graphed  PPOLCP with the fused penalty (gr_lcp_forward / gr_lcp_backward)

Each variant owns an algorithm over one synthetic rollout (4 096 envs x 24 steps, 4 mini-batches, 1 epoch); one
measurement is the host time of `--reps` update() calls, each ended by a device synchronise, divided by the steps.
The variants are alternated `--rounds` times in one process; the parameters are restored after every update so
every measurement times the same arithmetic.  Prints one JSON line per variant (median, min, max, spread =
(max - min) / median) and the ratios, and writes every per-run value to --out.

    python scripts/time_ppo_lcp.py [--rounds 5] [--reps 3] [--out profiles/ppo_lcp_step_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from generalizableracing_amd.rsl_rl import PPO, PPOLCP, ActorCritic  # noqa: E402

DEV = "cuda:0"
N, T, NMB, OBS, K = 4096, 24, 4, 16, 4
HP = dict(num_learning_epochs=1, num_mini_batches=NMB, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
          entropy_coef=0.0, learning_rate=5e-4, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive",
          desired_kl=0.01)
SCHEDULE = [0.1, 0.1, 700, 1000]


def make(variant, pol):
    import copy

    pol = copy.deepcopy(pol)
    if variant.startswith("ppo"):
        return PPO(pol, device=DEV, graph_update=variant.endswith("graphed"), **HP)
    if variant == "lcp_torch":
        return PPOLCP(pol, device=DEV, grad_penalty_coef_schedule=SCHEDULE, fused_losses=False, fused_mlp=False, **HP)
    return PPOLCP(pol, device=DEV, grad_penalty_coef_schedule=SCHEDULE, graph_update=variant.endswith("graphed"), **HP)


def fill(alg, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    alg.init_storage("rl", N, T, [OBS], [OBS], [K])
    with torch.inference_mode():
        for _ in range(T):
            obs, cobs = torch.randn(N, OBS, generator=g).to(DEV), torch.randn(N, OBS, generator=g).to(DEV)
            alg.act(obs, cobs)
            dones = (torch.rand(N, generator=g) < 0.02).to(DEV)
            alg.process_env_step((0.1 * torch.randn(N, generator=g)).to(DEV), dones, {})
        alg.compute_returns(torch.randn(N, OBS, generator=g).to(DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_lcp_step_ab.json"))
    ap.add_argument("--variants", nargs="+", default=["ppo_eager", "lcp_torch", "lcp_fused", "ppo_graphed",
                                                      "lcp_fused_graphed"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_ppo_lcp.py measures on the GPU"
    torch.manual_seed(0)
    pol = ActorCritic(OBS, OBS, K, [256, 256], [256, 256], "lrelu").to(DEV)
    algs, snaps = {}, {}
    for v in a.variants:
        algs[v] = make(v, pol)
        fill(algs[v])
        snaps[v] = [p.detach().clone() for p in algs[v].policy.parameters()]

    def update(v):
        alg = algs[v]
        alg.storage.step = T
        alg.learning_rate = HP["learning_rate"]
        out = alg.update()
        with torch.no_grad():
            for p, s in zip(alg.policy.parameters(), snaps[v]):
                p.copy_(s)
        return out

    for v in a.variants:  # warm-up: code objects, the graph capture
        for _ in range(2):
            update(v)
    torch.cuda.synchronize()
    runs = {v: [] for v in a.variants}
    for _ in range(a.rounds):
        for v in a.variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                update(v)
            torch.cuda.synchronize()
            runs[v].append((time.perf_counter() - t0) / (a.reps * NMB) * 1e6)
    summary = {}
    for v, xs in runs.items():
        med = statistics.median(xs)
        summary[v] = {"median_us_per_step": med, "min": min(xs), "max": max(xs), "spread": (max(xs) - min(xs)) / med}
        print(json.dumps({"variant": v, **summary[v]}), flush=True)
    ratios = {}
    med = lambda v: summary[v]["median_us_per_step"]  # noqa: E731
    for num, den in (("lcp_fused", "ppo_eager"), ("lcp_fused_graphed", "ppo_graphed"), ("lcp_torch", "lcp_fused"),
                     ("lcp_torch", "lcp_fused_graphed")):
        if num in summary and den in summary:
            ratios[f"{num}/{den}"] = med(num) / med(den)
    print(json.dumps({"ratios": ratios, "flop_ratio_lcp_over_ppo": 1.5}), flush=True)
    fused_steps = {v: int(getattr(algs[v], "fused_penalty_steps", 0)) for v in a.variants}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"rows_per_step": N * T // NMB, "hidden": 256, "obs": OBS, "actions": K, "rounds": a.rounds,
                   "reps_per_round": a.reps, "steps_per_update": NMB, "unit": "us per mini-batch step (host time of "
                   "update() ended by a device synchronise / steps)", "runs": runs, "summary": summary,
                   "ratios": ratios, "fused_penalty_steps": fused_steps, "device": torch.cuda.get_device_name(0)}, f,
                  indent=1)


if __name__ == "__main__":
    main()
