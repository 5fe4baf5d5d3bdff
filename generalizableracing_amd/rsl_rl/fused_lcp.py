"""PPOLCP's Lipschitz gradient penalty on the actor as one device op each way (gr_lcp_forward / gr_lcp_backward,
csrc/gr_lcp.hip).

PPOLCP._calc_grad_penalty (standalone/rsl_rl/ext/algorithms/ppo_lcp.py:105-108) is
    P = mean_rows | d sum(log pi(a | x)) / dx |^2
through torch's double backward over `obs.clone().requires_grad_()`.  For the MLP actor x -> z1 = W1 x + b1 ->
h1 = lrelu(z1) -> z2 = W2 h1 + b2 -> h2 = lrelu(z2) -> mu = W3 h2 + b3 with a state-independent std, LeakyReLU's
second derivative is zero, so P and its gradient are first-order chains over the activation masks
D = (z > 0 ? 1 : slope) that the fused forward (linear._FusedMLPsFn) already saved as h1 and z2:

    penalty : delta = (a - mu) / std^2;  v2 = D2 (W3^T delta);  v1 = D1 (W2^T v2);  g = W1^T v1;  P = mean |g|^2
    gradient: gb = (2 c / rows) g;  s1 = D1 (W1 gb);  s2 = D2 (W2 s1);  dbar = W3 s2;
              gW1 = v1^T gb;  gW2 = v2^T s1;  gW3 = delta^T s2;  dmu = -dbar / std^2;  dstd = sum -2 delta dbar / std

The observations need no gradient; nothing here is differentiated twice.  dmu joins the PPO loss's gradient of the
mean and goes through the ordinary gr_mlp_backward.  The biases have no direct term.
"""
from __future__ import annotations

import torch

from .. import _abi

# the number of penalties evaluated through gr_lcp_forward (tests and the train CLI read it: the fused path was taken)
CALLS = 0


def _ld(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("fused LCP penalty: rows must have unit column stride")
    return int(t.stride(0))


class _LCPPenaltyFn(torch.autograd.Function):
    """P(mu, std, W1, W2, W3) with the backward above; act, h1, z2 and the slope are constants.  The backward leaves
    the saved tensors intact and writes new buffers, so a retained graph may run it again."""

    @staticmethod
    def forward(ctx, mu, std, w1, w2, w3, act, h1, z2, slope):
        global CALLS
        std, w1, w2, w3 = std.contiguous(), w1.contiguous(), w2.contiguous(), w3.contiguous()
        rows, k = mu.shape
        h, d = w1.shape
        dev = mu.device
        g = torch.empty(rows, d, device=dev, dtype=torch.float32)
        v1 = torch.empty(rows, h, device=dev, dtype=torch.float32)
        v2 = torch.empty(rows, h, device=dev, dtype=torch.float32)
        scratch = torch.empty(int(_abi.load().gr_lcp_scratch_floats(rows, h)), device=dev, dtype=torch.float32)
        pen = torch.empty(1, device=dev, dtype=torch.float32)
        _abi.call("gr_lcp_forward", mu.data_ptr(), _ld(mu), act.data_ptr(), _ld(act), std.data_ptr(), h1.data_ptr(),
                  z2.data_ptr(), w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), rows, h, d, k, float(slope),
                  g.data_ptr(), v1.data_ptr(), v2.data_ptr(), scratch.data_ptr(), pen.data_ptr(),
                  _abi.raw_stream(dev))
        ctx.save_for_backward(mu, std, w1, w2, w3, act, h1, z2, g, v1, v2)
        ctx.slope = float(slope)
        CALLS += 1
        return pen.view(())

    @staticmethod
    def backward(ctx, g_pen):
        mu, std, w1, w2, w3, act, h1, z2, g, v1, v2 = ctx.saved_tensors
        rows, k = mu.shape
        h, d = w1.shape
        dev = mu.device
        g_pen = g_pen.float().reshape(1).contiguous()
        s1 = torch.empty(rows, h, device=dev, dtype=torch.float32)
        scratch = torch.empty(int(_abi.load().gr_lcp_scratch_floats(rows, h)), device=dev, dtype=torch.float32)
        dmu = torch.empty(rows, k, device=dev, dtype=torch.float32)
        dstd = torch.empty(k, device=dev, dtype=torch.float32)
        grads = torch.empty(h * d + h * h + k * h, device=dev, dtype=torch.float32)
        _abi.call("gr_lcp_backward", mu.data_ptr(), _ld(mu), act.data_ptr(), _ld(act), std.data_ptr(), h1.data_ptr(),
                  z2.data_ptr(), w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), rows, h, d, k, ctx.slope, g.data_ptr(),
                  v1.data_ptr(), v2.data_ptr(), g_pen.data_ptr(), s1.data_ptr(), scratch.data_ptr(), dmu.data_ptr(),
                  dstd.data_ptr(), grads.data_ptr(), _abi.raw_stream(dev))
        gw1 = grads[:h * d].view(h, d)
        gw2 = grads[h * d:h * d + h * h].view(h, h)
        gw3 = grads[h * d + h * h:].view(k, h)
        return dmu, dstd, gw1, gw2, gw3, None, None, None, None


def lcp_penalty(actor, mu, std, act, h1, z2):
    """The gradient penalty of `actor` (a Linear -> LeakyReLU -> Linear -> LeakyReLU -> Linear stack that
    linear.networks_fusable covers) on a mini-batch: mu [rows, k] its output, h1 / z2 [rows, H] the forward's saved
    activations (linear.fused_mlps(..., extras=True)), std [k] the policy's std, act [rows, k] the stored actions
    (row-strided).  A differentiable 0-dim tensor."""
    from .linear import _mlp_layers

    l1, l2, l3, slope = _mlp_layers(actor)
    return _LCPPenaltyFn.apply(mu, std, l1.weight, l2.weight, l3.weight, act, h1, z2, slope)
