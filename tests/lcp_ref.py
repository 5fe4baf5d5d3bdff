"""Float64 restatement of PPOLCP's gradient penalty and its gradient, without second-order autograd.

Actor x -> z1 = W1 x + b1 -> h1 = lrelu(z1) -> z2 = W2 h1 + b2 -> h2 = lrelu(z2) -> mu = W3 h2 + b3, Gaussian with a
state-independent std.  D = (z > 0 ? 1 : slope) is torch's leaky_relu backward; the sign of h1 is the sign of z1.

    penalty : delta = (a - mu) / std^2;  v2 = D2 (W3^T delta);  v1 = D1 (W2^T v2);  g = W1^T v1;
              P = (1 / rows) sum |g|^2
    gradient: (c = dloss/dP)  gb = (2 c / rows) g;  s1 = D1 (W1 gb);  s2 = D2 (W2 s1);  dbar = W3 s2;
              gW1 = sum v1 gb^T;  gW2 = sum v2 s1^T;  gW3 = sum delta s2^T;  dmu = -dbar / std^2;
              dstd = sum -2 delta dbar / std   (no direct bias term)
dmu then goes through the ordinary backward of the network (total_grads).  The masks come from this module's own
float64 forward (forward) or are given (the fused op's fp32 signs).  Everything is torch float64 on the CPU.
"""
import torch


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def forward(x, w1, b1, w2, b2, w3, b3, slope):
    """(mu, D1, D2, h1, h2) of the float64 forward."""
    x, w1, b1, w2, b2, w3, b3 = (_f64(t) for t in (x, w1, b1, w2, b2, w3, b3))
    z1 = x @ w1.t() + b1
    h1 = torch.where(z1 > 0, z1, z1 * slope)
    z2 = h1 @ w2.t() + b2
    h2 = torch.where(z2 > 0, z2, z2 * slope)
    mu = h2 @ w3.t() + b3
    return mu, masks_of(z1, slope), masks_of(z2, slope), h1, h2


def masks_of(z, slope):
    """D = (z > 0 ? 1 : slope) as float64 (z: a pre-activation, or h1, whose sign is z1's)."""
    z = _f64(z)
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))


def penalty(mu, act, std, d1, d2, w1, w2, w3):
    """The penalty pass from the op's own inputs: dict(P, g, delta, v1, v2)."""
    mu, act, std, d1, d2, w1, w2, w3 = (_f64(t) for t in (mu, act, std, d1, d2, w1, w2, w3))
    delta = (act - mu) / std ** 2
    v2 = d2 * (delta @ w3)
    v1 = d1 * (v2 @ w2)
    g = v1 @ w1
    return dict(P=(g ** 2).sum() / mu.shape[0], g=g, delta=delta, v1=v1, v2=v2)


def gradient(mu, act, std, d1, d2, w1, w2, w3, c=1.0):
    """The gradient pass for upstream c = dloss/dP: dict(P, g, dmu, dstd, gW1, gW2, gW3) (the direct terms)."""
    p = penalty(mu, act, std, d1, d2, w1, w2, w3)
    std, d1, d2, w1, w2, w3 = (_f64(t) for t in (std, d1, d2, w1, w2, w3))
    gb = (2.0 * float(c) / p["g"].shape[0]) * p["g"]
    s1 = d1 * (gb @ w1.t())
    s2 = d2 * (s1 @ w2.t())
    dbar = s2 @ w3.t()
    return dict(P=p["P"], g=p["g"], dmu=-dbar / std ** 2, dstd=(-2.0 * p["delta"] * dbar / std).sum(0),
                gW1=p["v1"].t() @ gb, gW2=p["v2"].t() @ s1, gW3=p["delta"].t() @ s2)


def total_grads(x, act, std, w1, b1, w2, b2, w3, b3, slope, c=1.0, masks=None):
    """d(c P)/d(W1, b1, W2, b2, W3, b3, std) and P: the direct terms plus dmu through the network's ordinary
    backward.  masks (D1, D2): given (e.g. the fused forward's fp32 signs), else this forward's own."""
    mu, d1, d2, h1, h2 = forward(x, w1, b1, w2, b2, w3, b3, slope)
    if masks is not None:
        d1, d2 = (_f64(m) for m in masks)
    r = gradient(mu, act, std, d1, d2, w1, w2, w3, c)
    x, w2_, w3_ = _f64(x), _f64(w2), _f64(w3)
    gy = r["dmu"]
    gz2 = d2 * (gy @ w3_)
    gz1 = d1 * (gz2 @ w2_)
    return dict(P=r["P"], W1=r["gW1"] + gz1.t() @ x, b1=gz1.sum(0), W2=r["gW2"] + gz2.t() @ h1, b2=gz2.sum(0),
                W3=r["gW3"] + gy.t() @ h2, b3=gy.sum(0), std=r["dstd"])
