"""Time the recurrent policy's GRU memory at config C2's shape (4 096 envs x 24 steps, 4 mini-batches: B = 1 024
envs per mini-batch, R = 192, 16 observations; heads [128, 128]) with the fused op (gr_gru_seq_forward /
gr_gru_seq_backward, gr_gru_step) against torch's nn.GRU stepped in a loop on the same device:

    seq_forward / seq_backward   one memory over one mini-batch block [24, 1024, 16] -> [24, 1024, 192] and its BPTT
    step                         one whole recurrent mini-batch step of PPO.update() (both memories, heads, losses,
                                 backward, clip, Adam): host time of update() ended by a device synchronise / steps
    rollout_step                 one memory's rollout step over 4 096 envs (gr_gru_step against rnn on one step)

The variants are alternated `--rounds` times in one process after warm-up; the parameters are restored after every
update so every measurement times the same arithmetic.  Prints one JSON line per measurement (median, min, max,
spread = (max - min) / median) and the torch / fused ratios, and writes every per-run value to --out.

    python scripts/time_gru.py [--rounds 7] [--reps 3] [--out profiles/gru_update_ab.json]

The vision recipe's shape (VisionActorCriticRecurrent: the memories read the 192-wide feature, which trains):

    python scripts/time_gru.py --input-width 192 --input-grad --vision-step   # -> profiles/gru_wide_update_ab.json

    --input-width D   the memory legs on a [24, 1024, D] block of a [24, 4096, D] buffer (the wide family, D > 64)
    --input-grad      seq_forward_backward also differentiates in x (gx)
    --vision-step     the step leg is the whole recurrent vision mini-batch step (stem + state encoder on the rows of
                      the storage's [24, 4096, 16 + 72 x 96] buffers, both memories, heads, losses, backward, clip, Adam)
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_gru.py --profile   # the fused step's kernels
                                                     # (profiles/gru_step_kernel_stats.csv is that run's stats file)
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from generalizableracing_amd.rsl_rl import (PPO, ActorCriticRecurrent, VisionActorCriticRecurrent,  # noqa: E402
                                            fused_gru)
from generalizableracing_amd.rsl_rl.actor_critic_recurrent import Memory  # noqa: E402

DEV = "cuda:0"
N, T, NMB, OBS, K, R = 4096, 24, 4, 16, 4, 192
B = N // NMB
HP = dict(num_learning_epochs=1, num_mini_batches=NMB, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
          entropy_coef=0.0, learning_rate=5e-4, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive",
          desired_kl=0.01)


def fill(alg, seed=0, pixels=0):
    """One rollout of random rows: OBS state terms ~ N(0, 1), then `pixels` depth-like values in [0, 10] m."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    gd = torch.Generator(device=DEV).manual_seed(seed)
    width = OBS + pixels

    def rows():
        x = torch.randn(N, OBS, generator=g).to(DEV)
        if pixels:
            x = torch.cat([x, 10.0 * torch.rand(N, pixels, generator=gd, device=DEV)], dim=1)
        return x

    alg.init_storage("rl", N, T, [width], [width], [K])
    with torch.inference_mode():
        for _ in range(T):
            alg.act(rows(), rows())
            dones = (torch.rand(N, generator=g) < 0.02).to(DEV)
            alg.process_env_step((0.1 * torch.randn(N, generator=g)).to(DEV), dones, {})
        alg.compute_returns(rows())


def stats(xs):
    med = statistics.median(xs)
    return {"median_us": med, "min": min(xs), "max": max(xs), "spread": (max(xs) - min(xs)) / med}


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="only a few fused update steps (under rocprofv3)")
    ap.add_argument("--input-width", type=int, default=OBS, help="input width D of the memory legs")
    ap.add_argument("--input-grad", action="store_true", help="seq_forward_backward also differentiates in x")
    ap.add_argument("--vision-step", action="store_true", help="the step leg on VisionActorCriticRecurrent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_gru.py measures on the GPU"
    D = a.input_width
    wide = D != OBS or a.input_grad or a.vision_step
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gru_wide_update_ab.json" if wide else "gru_update_ab.json")
    torch.manual_seed(0)
    pixels = 72 * 96 if a.vision_step else 0
    if a.vision_step:
        base = VisionActorCriticRecurrent(OBS + pixels, OBS + pixels, K, dim_hidden_input=192,
                                          actor_hidden_dims=[128, 128], critic_hidden_dims=[128, 128],
                                          activation="lrelu", rnn_hidden_size=R).to(DEV)
    else:
        base = ActorCriticRecurrent(OBS, OBS, K, [128, 128], [128, 128], "lrelu", rnn_hidden_size=R).to(DEV)
    variants = ("fused",) if a.profile else ("fused", "torch")
    algs, snaps = {}, {}
    for v in variants:
        pol = copy.deepcopy(base)
        pol.fused_gru = v == "fused"
        algs[v] = PPO(pol, device=DEV, **HP)
        fill(algs[v], pixels=pixels)
        snaps[v] = [p.detach().clone() for p in pol.parameters()]

    def update(v):
        alg = algs[v]
        alg.storage.step = T
        alg.learning_rate = HP["learning_rate"]
        alg.update()
        with torch.no_grad():
            for p, s in zip(alg.policy.parameters(), snaps[v]):
                p.copy_(s)

    for v in variants:  # warm-up: code objects, allocator
        for _ in range(2):
            update(v)
    if a.profile:
        for _ in range(3):
            update("fused")
        torch.cuda.synchronize()
        return
    calls, wide_calls = fused_gru.CALLS, fused_gru.WIDE_CALLS
    update("fused")
    assert fused_gru.CALLS - calls == 2 * NMB, "the fused path was not taken"
    assert fused_gru.WIDE_CALLS - wide_calls == (2 * NMB if a.vision_step else 0)

    # one memory over one mini-batch block, and one rollout step
    st = algs["fused"].storage
    dones, h0 = st.dones[:, :B, 0], st.h0_a[:B].unsqueeze(0)
    if D == OBS and not a.vision_step:  # the policy's own memory on the stored observations
        x = st.observations[:T, :B]
        mems = {v: algs[v].policy.memory_a for v in variants}
    else:  # a memory of input width D on a block of a [T, N, D] buffer
        x = torch.randn(T, N, D, device=DEV)[:, :B]
        ref = Memory(D, R).to(DEV)
        mems = {v: copy.deepcopy(ref) for v in variants}
        for v in variants:
            mems[v].fused = v == "fused"
    if a.input_grad:
        x = x.detach().requires_grad_(True)
    gout = torch.randn(T * B, R, device=DEV)
    xs, hs = torch.randn(N, D, device=DEV), {v: torch.zeros(1, N, R, device=DEV) for v in variants}

    def seq_fwd(v):
        with torch.no_grad():
            mems[v].sequence(x, dones, h0)

    def seq_fwd_bwd(v):
        mem = mems[v]
        out = mem.sequence(x, dones, h0)
        torch.autograd.grad(out, list(mem.parameters()) + ([x] if a.input_grad else []), grad_outputs=gout)

    def rollout_step(v):
        mem = mems[v]
        with torch.inference_mode():
            if v == "fused":
                fused_gru.gru_step(mem.rnn, xs, hs[v][0])
            else:
                mem.rnn(xs.unsqueeze(0), hs[v])

    work = {"seq_forward": (seq_fwd, 1), "seq_forward_backward": (seq_fwd_bwd, 1), "step": (update, NMB),
            "rollout_step": (rollout_step, 1)}
    for fn, _ in work.values():
        for v in variants:
            fn(v)
    runs = {name: {v: [] for v in variants} for name in work}
    for _ in range(a.rounds):
        for name, (fn, div) in work.items():
            reps = a.reps * (20 if name == "rollout_step" else 1)
            for v in variants:
                runs[name][v].append(timed(lambda: fn(v), reps) / div)
    summary, ratios = {}, {}
    for name in work:
        summary[name] = {v: stats(runs[name][v]) for v in variants}
        ratios[name] = summary[name]["torch"]["median_us"] / summary[name]["fused"]["median_us"]
        print(json.dumps({"measurement": name, **summary[name], "torch/fused": ratios[name]}), flush=True)
    for v in variants:  # the backward alone: forward + backward less the forward (medians)
        summary.setdefault("seq_backward", {})[v] = {
            "median_us": summary["seq_forward_backward"][v]["median_us"] - summary["seq_forward"][v]["median_us"]}
    ratios["seq_backward"] = summary["seq_backward"]["torch"]["median_us"] / summary["seq_backward"]["fused"]["median_us"]
    print(json.dumps({"measurement": "seq_backward", **summary["seq_backward"], "torch/fused": ratios["seq_backward"]}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"envs": N, "steps": T, "mini_batches": NMB, "envs_per_mini_batch": B, "hidden": R, "obs": OBS,
                   "input_width": D, "input_grad": bool(a.input_grad), "step_policy": type(base).__name__,
                   "heads": [128, 128], "rounds": a.rounds, "reps_per_round": a.reps,
                   "unit": "us (host time ended by a device synchronise; step: update() / mini-batch steps; "
                           "seq_backward: forward + backward less forward)",
                   "runs": runs, "summary": summary, "torch_over_fused": ratios,
                   "fused_gru_default_on": bool(ratios["step"] > 1.0), "device": torch.cuda.get_device_name(0)}, f,
                  indent=1)


if __name__ == "__main__":
    main()
