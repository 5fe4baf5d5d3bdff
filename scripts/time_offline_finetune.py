"""Time the offline auxiliary-head stage on one GPU, the fused HIP ops against the eager restatement of the reference's
loops on the same device (the parent of this stage has none, so the eager loop is the baseline):

    step_fused / step_eager    one mini-batch step of the fine-tune at 256 rows x 192 (gr_offline_pgd_step, two
                               launches, against pgd_attack + BCEWithLogitsLoss + torch.optim.Adam on a gathered batch)
    epoch_fused / epoch_eager  HeadFinetuner.epoch over 20 000 rows in batches of 256 (79 steps, one read-back)
    add_fused / add_eager      FeatureCollector.add at 4 096 envs x 192, ~3 % positive labels (gr_offline_collect, two
                               launches and no read-back, against nonzero + index copies + the cursor's host read)

One measurement is the host time of `--reps` calls ended by a device synchronise, divided by the calls.  The variants
of a pair are alternated `--rounds` times in one process after a warm-up of every shape; the collectors are emptied
and the heads restored between measurements so each times the same work.  Prints one JSON line per variant (median,
min, max, spread = (max - min) / median) and the ratios, and writes every per-run value to --out.

    python scripts/time_offline_finetune.py [--rounds 7] [--out profiles/offline_finetune_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from generalizableracing_amd.offline import FeatureCollector, HeadFinetuner  # noqa: E402

DEV = "cuda:0"
D, BATCH, EPOCH_ROWS, ENVS = 192, 256, 20000, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step_reps", type=int, default=200)
    ap.add_argument("--epoch_reps", type=int, default=3)
    ap.add_argument("--add_reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offline_finetune_ab.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_offline_finetune.py measures on the GPU"
    g = torch.Generator(device=DEV).manual_seed(0)
    feats = torch.rand(EPOCH_ROWS, D, device=DEV, generator=g)
    rule = torch.randn(D, device=DEV, generator=g)
    sup = ((feats - 0.5) @ rule > 0).to(torch.int8)
    data = (feats, sup)
    torch.manual_seed(0)
    head0 = nn.Linear(D, 1)
    tuners = {}
    for v in ("fused", "eager"):
        head = nn.Linear(D, 1)
        head.load_state_dict(head0.state_dict())
        tuners[v] = HeadFinetuner(head, device=DEV, fused=(v == "fused"))
    assert tuners["fused"].fused and not tuners["eager"].fused
    index = torch.randperm(EPOCH_ROWS, device=DEV, generator=g)[:BATCH].contiguous()
    xb, yb = feats[index], sup[index].float().unsqueeze(1)
    step_feat = torch.rand(ENVS, D, device=DEV, generator=g)
    step_aux = (torch.rand(ENVS, 1, device=DEV, generator=g) < 0.03).float()
    cols = {v: FeatureCollector(2_000_000, D, DEV) for v in ("fused", "eager")}

    def step(v, reps):
        t = tuners[v]
        for _ in range(reps):
            if v == "fused":
                t.fused_step(feats, sup, index)
            else:
                t.eager_step(xb, yb)

    def epoch(v, reps):
        for r in range(reps):
            tuners[v].epoch(data, BATCH, torch.Generator(device=DEV).manual_seed(r))

    def add(v, reps):
        c = cols[v]
        c.cursor.zero_()
        for _ in range(reps):
            if v == "fused":
                c.add(step_feat, step_aux)
            else:
                c._add_eager(step_feat, step_aux[:, 0])

    work = {"step": (step, a.step_reps), "epoch": (epoch, a.epoch_reps), "add": (add, a.add_reps)}
    for fn, _ in work.values():  # warm-up: code objects, the allocator
        for v in ("fused", "eager"):
            fn(v, 2)
    torch.cuda.synchronize()
    runs = {f"{k}_{v}": [] for k in work for v in ("fused", "eager")}
    for _ in range(a.rounds):
        for k, (fn, reps) in work.items():
            for v in ("fused", "eager"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(v, reps)
                torch.cuda.synchronize()
                runs[f"{k}_{v}"].append((time.perf_counter() - t0) / reps * 1e6)
    summary = {}
    for v, xs in runs.items():
        med = statistics.median(xs)
        summary[v] = {"median_us": med, "min": min(xs), "max": max(xs), "spread": (max(xs) - min(xs)) / med}
        print(json.dumps({"variant": v, **summary[v]}), flush=True)
    ratios = {f"{k}_eager/{k}_fused": summary[f"{k}_eager"]["median_us"] / summary[f"{k}_fused"]["median_us"]
              for k in work}
    print(json.dumps({"ratios": ratios}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"dim": D, "batch_rows": BATCH, "epoch_rows": EPOCH_ROWS, "epoch_steps": -(-EPOCH_ROWS // BATCH),
                   "collector_envs": ENVS, "collector_positive_share": 0.03, "rounds": a.rounds,
                   "reps": {k: r for k, (_, r) in work.items()},
                   "unit": "us per call (host time of the calls ended by a device synchronise / calls): step = one "
                           "mini-batch step, epoch = one 20 000-row epoch, add = one collector step",
                   "launches_per_call": {"step_fused": 2, "add_fused": 2},
                   "runs": runs, "summary": summary, "ratios": ratios, "device": torch.cuda.get_device_name(0)}, f,
                  indent=1)


if __name__ == "__main__":
    main()
