"""The fp32 floor of the window's action gradient -> profiles/bptt_error_budget.json (runs on the CPU).

tests/test_gpu_diff_backward.py and tests/test_gpu_bptt.py bound the fused adjoint kernel, case by case, by 4 x the
case's own floor.  The floor is measured, not taken from the kernel: the same window (tests/diff_window.py: the tests' shapes, both action
lags, N(0, 1) actions, the forced resets) is driven on the CPU oracle, its action gradient computed once by the fp32
torch restatement (diff_ops.torch_backward) and once in float64 (tests/bptt_ref.py on the same tape, upcast), and the
error is the tests' quantity, ||dG[:, n, :]|| / ||G_ref[:, n, :]|| per env; a case's floor is its maximum over the envs and
8 seeds ("floor": the largest of them).  The factor 4 covers that the kernel's operation order differs from torch's and that the floor is a
sample.

    python scripts/bptt_error_budget.py
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import bptt_ref  # noqa: E402
import diff_window as dw  # noqa: E402

SEEDS = 8


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cases = []
    floor = 0.0
    todo = [(T, N, lag) for T, N in dw.SHAPES for lag in (0, 1)] + [dw.BPTT_SHAPE]
    for T, N, lag in todo:
        if True:
            worst = 0.0
            for seed in range(SEEDS):
                env = dw.oracle_window(T, N, lag, seed, dtype=torch.float32)
                G32 = env.loss_action_grad()
                k = dict(env.diff.k, scale=1.0 / (T * N))
                G64 = bptt_ref.window(bptt_ref.tape_fields(env.diff.tape), k)["grad"]
                err, nz = dw.per_env_error(G32, G64)
                if err.numel():
                    worst = max(worst, float(err.max()))
            cases.append({"T": T, "N": N, "lag": lag, "max_rel_err_per_env": worst})
            floor = max(floor, worst)
            print(cases[-1], flush=True)
    out = {"what": "max over envs, cases and seeds of ||G_fp32 - G_fp64|| / ||G_fp64|| per env (torch fp32 "
                   "restatement vs tests/bptt_ref.py in float64 on the same tape)",
           "seeds": SEEDS, "floor": floor, "bound_factor": dw.BOUND_FACTOR,
           "bound": "per case: bound_factor x the case's max_rel_err_per_env",
           "cases": cases}
    with open(dw.BUDGET_FILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"largest floor {floor:.3e}")


if __name__ == "__main__":
    main()
