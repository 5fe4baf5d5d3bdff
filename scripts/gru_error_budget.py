"""Write profiles/gru_error_budget.json: per case of tests/test_gpu_gru_kernels.py and per tensor (out and the four
parameter gradients), torch's own fp32 GRU error against the float64 restatement (tests/recurrent_ref.py, on the CPU),
the bound max(1e-5, 4 x that) the tests apply, and the fused kernels' achieved error; all relative to the float64
tensor's norm.

    python scripts/gru_error_budget.py [--out profiles/gru_error_budget.json]
    python scripts/gru_error_budget.py --wide     # tests/test_gpu_gru_wide_kernels.py's cases, with the input
                                                  # gradient gx -> profiles/gru_wide_error_budget.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gru_wide_ref as wr  # noqa: E402
import recurrent_ref as rr  # noqa: E402
import test_gpu_gru_kernels as tk  # noqa: E402
import test_gpu_gru_wide_kernels as tw  # noqa: E402


def wide_case(T, B, R, D):
    """(name, fused, float64, torch fp32) per tensor of a wide case: out, the parameter gradients and gx."""
    rnn, xbuf, h0, dones, gout = tw._inputs(T, B, R, D)
    x = xbuf[:, 2:2 + B]
    out, grads, gx = tw._fused(rnn, xbuf, B, h0, dones, gout)
    params = [p.detach() for p in rnn.parameters()]
    ref_out, ref_g, ref_gx = wr.masked_gru_dx(x, h0, dones, *params, gout=gout, dtype=torch.float64)
    t32_out, t32_g, t32_gx = wr.masked_gru_dx(x, h0, dones, *params, gout=gout, dtype=torch.float32)
    return ([("out", out, ref_out, t32_out)] + list(zip(tw.NAMES, grads, ref_g, t32_g))
            + [("gx", gx, ref_gx, t32_gx)])


def narrow_case(T, B, R, D):
    rnn, x, h0, dones, gout = tk._inputs(T, B, R, D)
    out, grads = tk._fused(rnn, x, h0, dones, gout)
    params = [p.detach() for p in rnn.parameters()]
    ref_out, ref_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float64)
    t32_out, t32_g = rr.masked_gru(x, h0, dones, *params, gout=gout, dtype=torch.float32)
    return [("out", out, ref_out, t32_out)] + list(zip(tk.NAMES, grads, ref_g, t32_g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="the wide family's cases, with gx")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gru_wide_error_budget.json" if a.wide else "gru_error_budget.json")
    assert torch.cuda.is_available(), "gru_error_budget.py measures on the GPU"
    cases = []
    for T, B, R, D in (tw.CASES if a.wide else tk.CASES):
        tensors = {}
        for name, got, ref, t32 in (wide_case if a.wide else narrow_case)(T, B, R, D):
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
