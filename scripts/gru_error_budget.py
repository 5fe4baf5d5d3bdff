"""Write profiles/gru_error_budget.json: per case of tests/test_gpu_gru_kernels.py and per tensor (out and the four
parameter gradients), torch's own fp32 GRU error against the float64 restatement (tests/recurrent_ref.py, on the CPU),
the bound max(1e-5, 4 x that) the tests apply, and the fused kernels' achieved error; all relative to the float64
tensor's norm.

    python scripts/gru_error_budget.py [--out profiles/gru_error_budget.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recurrent_ref as rr  # noqa: E402
import test_gpu_gru_kernels as tk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_error_budget.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gru_error_budget.py measures on the GPU"
    cases = []
    for T, B, R, D in tk.CASES:
        rnn, x, h0, dones, gout = tk._inputs(T, B, R, D)
        out, grads = tk._fused(rnn, x, h0, dones, gout)
        params = [p.detach() for p in rnn.parameters()]
        ref_out, ref_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float64)
        t32_out, t32_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float32)
        tensors = {}
        for name, got, ref, t32 in [("out", out, ref_out, t32_out)] + list(zip(tk.NAMES, grads, ref_g, t32_g)):
            e_torch = rr.rel_err(t32, ref)
            tensors[name] = {"torch_fp32_error": e_torch, "bound": max(1e-5, 4.0 * e_torch),
                             "fused_error": rr.rel_err(got, ref)}
        cases.append({"T": T, "B": B, "R": R, "D": D, "tensors": tensors})
        print(json.dumps(cases[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"rule": "bound = max(1e-5, 4 x torch fp32 error); errors are |x - float64| / |float64| over the "
                           "whole tensor; torch fp32 = nn.GRU on the CPU in float32, the same masked stepping",
                   "cases": cases, "device": torch.cuda.get_device_name(0)}, f, indent=1)


if __name__ == "__main__":
    main()
