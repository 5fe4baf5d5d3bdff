"""recurrent_ref.masked_gru extended with the input gradient, for the wide GRU family (gr_gru_wide_*): torch.nn.GRU on
the CPU in `dtype`, one step at a time, the carried state times 1 - dones[t-1].  The same definition, with x a leaf:
d/dx of sum(out * gout) comes back with the four parameter gradients."""
import torch
import torch.nn as nn


def masked_gru_dx(x, h0, dones, w_ih, w_hh, b_ih, b_hh, gout, dtype=torch.float64):
    """-> out [T, B, R], [gW_ih, gW_hh, gb_ih, gb_hh], gx [T, B, D], all detached, on the CPU in `dtype`."""
    T, B, D = x.shape
    R = w_hh.shape[1]
    rnn = nn.GRU(D, R, num_layers=1).to(dtype)
    with torch.no_grad():
        for p, v in zip((rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v.detach().cpu().to(dtype))
    xs = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    keep = 1.0 - dones.detach().cpu().reshape(T, B).to(dtype)
    h = h0.detach().cpu().to(dtype).reshape(1, B, R)
    outs = []
    for t in range(T):
        if t > 0:
            h = h * keep[t - 1].view(1, B, 1)
        o, h = rnn(xs[t:t + 1], h)
        outs.append(o[0])
    out = torch.stack(outs)
    grads = torch.autograd.grad((out * gout.detach().cpu().to(dtype)).sum(), list(rnn.parameters()) + [xs])
    return out.detach(), [g.detach() for g in grads[:4]], grads[4].detach()
