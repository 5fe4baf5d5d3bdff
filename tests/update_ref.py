"""Float64 restatement of the PPO update's scalar kernels (csrc/gr_update.hip: gr_ppo_loss_*, gr_adaptive_lr,
gr_adam_*), their test inputs and their error bounds.  Written from the formulas of include/gr.h and rsl_rl/ppo.py
(PPO._ppo_losses, PPO._kl_mean, PPO._adapt_learning_rate) and torch's foreach Adam, not from the kernels.

The loss reference is torch's own expressions (Normal.log_prob, torch.max of two tensors, torch.clamp,
torch.log(sigma / sigma_old + 1e-5)) in float64 on the CPU, differentiated by autograd: a tie of torch.max splits the
gradient, clamp passes it on its closed interval and both keep a NaN, so what the kernels promise is the reference's
by construction.  Its inputs are the fp32 inputs converted to double; `clip` is the fp32-rounded value.

Bounds (error_bounds, adam_bounds, clip_grad_bound) are first-order, assembled in float64 from the reference's
intermediates: u = 2^-24 per fp32 rounding on the path to an output, times the magnitude at that rounding, plus the
propagated error of the log prob through exp.  logf, expf and sqrtf are counted at 2 ulp (= 4 u relative): no ROCm
document stating the device library's ulp bounds is at hand, so this figure is assumed, not measured.  Every rounding
also gets an absolute floor of 2^-126 (the smallest normal fp32: an underflowing result is off by no more).  No
multiplier here was fitted to a result: tests/test_update_ref_cpu.py shows the bounds fair (torch's fp32 evaluation of
the same expressions passes) and sharp (ten subtle mutations of it fail).
"""
import json
import math
import os

import numpy as np
import torch

U = 2.0 ** -24  # fp32 unit roundoff: one correctly rounded operation
LIBM = 2.0 * 2.0 ** -23  # logf / expf / sqrtf at 2 ulp, relative (assumed)
TINY = 2.0 ** -126
LOG_SQRT_2PI = math.log(math.sqrt(2.0 * math.pi))
LOSS_FIELDS = ("mu", "std", "value", "act", "logp_old", "adv", "value_old", "ret", "mu_old", "sig_old")
SUM_REL = 1.0e-6  # the fixed-order fp32 reductions' bound, 1e-6 (sum |term| + 1), as tests/test_gpu_units.py test_column_sum
EXEMPT_CAP = 0.005  # at most this share of a case's rows may be left out of the per-row comparison

# ------------------------------------------------------------------------------------------------ the loss cases
ROWS = (1, 63, 64, 65, 255, 256, 257, 1031, 4099)
KS = (1, 2, 3, 4, 5, 8)


def loss_cases():
    """24 (rows, k, clipped_value, clip, seed): every value of each axis at least twice, no full product."""
    out = []
    for i in range(24):
        out.append((ROWS[i % 9], KS[(i + i // 9) % 6], i % 2, 0.2 if (i // 2) % 2 == 0 else 0.1, 1000 + i))
    return out


def f32(x):
    return float(np.float32(x))


def loss_inputs(rows, k, clip, seed):
    """fp32 CPU inputs of one case (LOSS_FIELDS; value / logp_old / adv / value_old / ret are [rows]) and `edge`, the
    mask of the constructed rows.  Row i's class is i % 8:
      0-3 generic; 4 advantage exactly 0; 5 value_old = 0 and value = +-clip exactly (the value clamp's closed
      boundary, and an exact tie of the two value terms); 6 |value - value_old| of 3-5 clips, the return on either
      side; 7 value_old = -+2 clip, value = +-clip, return 0: an exact tie of the two value terms beyond the clip
      (value_clipped = -+clip exactly, so both terms are clip^2 in fp32 and in float64), where the tie's half weight
      shows because the clipped branch passes no gradient.
    Old log probs put the ratio inside (|log ratio| < 0.8 clip), above (1.2-3 clips) and below (-3 to -1.3 clips) the
    clip range by i % 3, for either sign of the (random) advantage."""
    g = torch.Generator().manual_seed(seed)
    c32 = torch.tensor(clip, dtype=torch.float32)
    c = float(c32)
    i = torch.arange(rows)
    cls = i % 8
    std = (0.3 + 0.9 * torch.rand(k, generator=g)).float()
    mu = torch.randn(rows, k, generator=g)
    act = mu + std * torch.randn(rows, k, generator=g)
    logp = torch.distributions.Normal(mu.double(), std.double()).log_prob(act.double()).sum(-1)
    r = torch.rand(rows, generator=g).double()
    z = torch.where(i % 3 == 0, (1.6 * r - 0.8) * c, torch.where(i % 3 == 1, (1.2 + 1.8 * r) * c, -(1.3 + 1.7 * r) * c))
    logp_old = (logp - z).float()
    adv = torch.randn(rows, generator=g)
    value_old = torch.randn(rows, generator=g)
    value = value_old + c * (5.0 * torch.rand(rows, generator=g) - 2.5)
    sign = torch.where((i // 8) % 2 == 0, 1.0, -1.0).float()
    far = value_old + sign * (3.0 + 2.0 * torch.rand(rows, generator=g)) * c
    ret = value + 0.5 * torch.randn(rows, generator=g)
    ret_far = far + torch.randn(rows, generator=g)
    adv = torch.where(cls == 4, torch.zeros(()), adv)
    value_old = torch.where(cls == 5, torch.zeros(()), value_old)
    value = torch.where(cls == 5, sign * c32, value)
    value = torch.where(cls == 6, far, value)
    ret = torch.where(cls == 6, ret_far, ret)
    value_old = torch.where(cls == 7, -2.0 * sign * c32, value_old)
    value = torch.where(cls == 7, sign * c32, value)
    ret = torch.where(cls == 7, torch.zeros(()), ret)
    mu_old = mu + 0.1 * torch.randn(rows, k, generator=g)
    sig_old = (std * (0.9 + 0.2 * torch.rand(rows, k, generator=g))).float()
    out = dict(mu=mu, std=std, value=value, act=act, logp_old=logp_old, adv=adv, value_old=value_old, ret=ret,
               mu_old=mu_old, sig_old=sig_old)
    out = {n: t.float().contiguous() for n, t in out.items()}
    out["edge"] = cls >= 4
    return out


NONFINITE_ROWS = (5, 9, 200, 257)


def nonfinite_inputs():
    """(inputs with the four non-finite rows, the same inputs with ordinary values there): 300 rows, k = 4."""
    plain = loss_inputs(300, 4, 0.2, 77)
    bad = {n: t.clone() for n, t in plain.items()}
    bad["logp_old"][5] = -1.0e30  # ratio inf ...
    bad["adv"][5] = 0.0  # ... times a zero advantage: NaN
    bad["ret"][9] = float("nan")
    bad["adv"][200] = float("nan")
    bad["logp_old"][257] = 1.0e30  # ratio 0
    return bad, plain


# ------------------------------------------------------------------------------------------- the loss reference
class _ClampOpenGrad(torch.autograd.Function):
    """(mutation) clamp whose gradient passes on the open interval only"""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.save_for_backward((x > lo) & (x < hi))
        return x.clamp(lo, hi)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None, None


MUTATIONS = ("clamp_open", "tie_one_side", "kl_no_eps", "var_not_2var", "no_inv_sigma", "rows_minus_1",
             "surr_clamp_passes")


def ppo_loss_ref(inp, clip, clipped_value, value_coef, g, dtype=torch.float64, mutate=None):
    """The losses of one mini-batch and their gradients in `dtype` (float64: the reference; float32: torch's own fp32
    evaluation, the CPU stand-in for the kernel; mutate: one of MUTATIONS, a subtly wrong variant of it).
    g = (g_surrogate, g_value): the upstream gradients of the two means.  Returns detached tensors: per row logp,
    ratio, s1, s2, surr, l1, l2, vterm, vdiff, vc, kl (and logp_terms / kl_terms per action), sums [3], means [3],
    loss, dmu [rows, k], dvalue [rows], dlogp [rows], ds [rows, k] (the rows of dstd), dstd [k]."""
    c = f32(clip)
    t = {n: inp[n].to(dtype) for n in LOSS_FIELDS}
    rows, k = t["mu"].shape
    mu, value, std = t["mu"].requires_grad_(), t["value"].requires_grad_(), t["std"].requires_grad_()
    sig = std.expand(rows, k)  # (non-leaf: its gradient is the rows of dstd)
    if mutate == "var_not_2var":
        logp_terms = -((t["act"] - mu) ** 2) / (sig ** 2) - sig.log() - LOG_SQRT_2PI
    elif mutate == "no_inv_sigma":
        logp_terms = -((t["act"] - mu) ** 2) / (2 * sig ** 2) - sig.detach().log() - LOG_SQRT_2PI
    else:
        logp_terms = torch.distributions.Normal(mu, sig, validate_args=False).log_prob(t["act"])
    logp = logp_terms.sum(-1)
    # PPO._ppo_losses
    ratio = torch.exp(logp - t["logp_old"])
    s1 = -t["adv"] * ratio
    rc = torch.clamp(ratio, 1.0 - c, 1.0 + c)
    if mutate == "surr_clamp_passes":
        rc = ratio + (rc - ratio).detach()
    s2 = -t["adv"] * rc
    surr = torch.max(s1, s2)
    vdiff = value - t["value_old"]
    cl = _ClampOpenGrad.apply(vdiff, -c, c) if mutate == "clamp_open" else vdiff.clamp(-c, c)
    vc = t["value_old"] + cl
    l1 = (value - t["ret"]).pow(2)
    l2 = (vc - t["ret"]).pow(2)
    if clipped_value:
        vterm = torch.where(l1 >= l2, l1, l2) if mutate == "tie_one_side" else torch.max(l1, l2)
    else:
        vterm = (t["ret"] - value).pow(2)
    # PPO._kl_mean
    eps = 0.0 if mutate == "kl_no_eps" else 1.0e-5
    kl_terms = (torch.log(sig / t["sig_old"] + eps)
                + (torch.square(t["sig_old"]) + torch.square(t["mu_old"] - mu)) / (2.0 * torch.square(sig)) - 0.5)
    kl = torch.sum(kl_terms, axis=-1)
    sums = torch.stack([surr.sum(), vterm.sum(), kl.sum()])
    means = sums / ((rows - 1) if mutate == "rows_minus_1" else rows)
    loss = means[0] + value_coef * means[1]
    total = g[0] * means[0] + g[1] * means[1]
    dmu, dvalue, ds, dlogp = torch.autograd.grad(total, [mu, value, sig, logp], allow_unused=True)
    out = dict(logp_terms=logp_terms, logp=logp, ratio=ratio, s1=s1, s2=s2, surr=surr, l1=l1, l2=l2, vterm=vterm,
               vdiff=vdiff, vc=vc, kl_terms=kl_terms, kl=kl, sums=sums, means=means, loss=loss, dmu=dmu, dvalue=dvalue,
               dlogp=dlogp, ds=ds, dstd=ds.sum(0))
    return {n: v.detach() for n, v in out.items()}


def error_bounds(ref, inp, clip, clipped_value, value_coef, g):
    """Bounds on |fp32 evaluation - float64 reference| from the reference's intermediates (all float64 tensors):
    per row `dmu` [rows, k], `dvalue` [rows]; `exempt` [rows] (bool: rows the per-row comparison may leave out);
    `sums` [3], `means` [3], `loss`, `dstd` [k].  The counts of fp32 roundings are written beside each line; u = U,
    L = LIBM."""
    u, L = U, LIBM
    c = f32(clip)
    f = {n: inp[n].double() for n in LOSS_FIELDS}
    rows, k = f["mu"].shape
    sd, var = f["std"], f["std"] ** 2
    d = f["act"] - f["mu"]
    # log prob, per action: q = d^2 / (2 var): d (1, twice: it is squared), the square (1), var (1), the quotient (1)
    # = 5 u q; log sigma at L; the two subtractions (1 each); the constant's own rounding (1)
    q = d * d / (2 * var)
    ls = sd.log()
    tj = ref["logp_terms"].abs()
    e_t = 5 * u * q + L * ls.abs() + u * (q + ls).abs() + u * LOG_SQRT_2PI + u * tj
    # the sum over the actions: k - 1 additions, each of a partial sum of at most sum |t_j|
    e_logp = e_t.sum(-1) + (k - 1) * u * tj.sum(-1)
    # ratio = exp(z), z = logp - logp_old (1); exp at L, and the propagated error of z
    z = ref["logp"] - f["logp_old"]
    ratio = ref["ratio"]
    rel_ratio = e_logp + u * z.abs() + L
    e_ratio = ratio * rel_ratio
    lo, hi = 1.0 - c, 1.0 + c
    inclip = (ratio >= lo) & (ratio <= hi)
    A = f["adv"]
    # s1 = -A ratio (1); s2 = -A clamp(ratio) (1), the clamped value's error the ratio's inside, else the rounding
    # of 1 -+ clip (1)
    e_rc = torch.where(inclip, e_ratio, u * ref["ratio"].clamp(lo, hi))
    e_s1 = A.abs() * e_ratio + u * ref["s1"].abs()
    e_s2 = A.abs() * e_rc + u * ref["s2"].abs()
    s1, s2 = ref["s1"], ref["s2"]
    e_surr = torch.where(s1 > s2, e_s1, torch.where(s2 > s1, e_s2, torch.maximum(e_s1, e_s2)))
    # rows whose ratio lies within its bound of 1 -+ clip may fall on the other side in fp32 (no matter at A = 0)
    near = ((ratio - lo).abs() <= e_ratio + u * lo) | ((ratio - hi).abs() <= e_ratio + u * hi)
    exempt = near & (A != 0)
    # value terms: a = v - ret (1), l1 = a^2 (1): 3 u a^2
    a = f["value"] - f["ret"]
    e_a = u * a.abs()
    e_l1 = 2 * a.abs() * e_a + u * a * a
    if clipped_value:
        # vdiff = v - v_old (1); the clamp keeps it inside, and is exact outside (-+clip are inputs); v_c = v_old +
        # clamp (1); b = v_c - ret (1); l2 = b^2 (1)
        vdiff = ref["vdiff"]
        e_vd = u * vdiff.abs()
        vin = vdiff.abs() <= c
        e_vc = torch.where(vin, e_vd, torch.zeros_like(e_vd)) + u * ref["vc"].abs()
        b = ref["vc"] - f["ret"]
        e_b = e_vc + u * b.abs()
        e_l2 = 2 * b.abs() * e_b + u * b * b
        l1, l2 = ref["l1"], ref["l2"]
        e_vterm = torch.where(l1 > l2, e_l1, torch.where(l2 > l1, e_l2, torch.maximum(e_l1, e_l2)))
        # the two terms closer than their bounds, or vdiff within its rounding of -+clip, but not exactly there: fp32
        # may take the other branch (an exact tie or an exact boundary is the same in fp32: symmetric roundings)
        gap, edge = (l1 - l2).abs(), (vdiff.abs() - c).abs()
        exempt = exempt | ((gap > 0) & (gap <= e_l1 + e_l2)) | ((edge > 0) & (edge <= e_vd))
    else:
        e_vterm = e_l1
    # KL per action: r = sigma / sigma_old (1); + 1e-5 (the constant 1, the addition 1); log at L; sigma_old^2 (1),
    # dm = mu_old - mu (1, squared: twice) and its square (1), their sum (1); 2 sigma^2 (1) and the quotient (1); the
    # addition (1); - 0.5 (1); then k - 1 additions
    so, dm = f["sig_old"], f["mu_old"] - f["mu"]
    r = sd / so
    arg = r + 1.0e-5
    e_arg = u * r + u * 1.0e-5 + u * arg
    lg = arg.log()
    e_lg = e_arg / arg + L * lg.abs()
    num = so * so + dm * dm
    e_num = u * so * so + 3 * u * dm * dm + u * num
    fr = num / (2 * var)
    e_fr = e_num / (2 * var) + 2 * u * fr
    w = lg + fr
    e_term = e_lg + e_fr + u * w.abs() + u * ref["kl_terms"].abs()
    e_kl = e_term.sum(-1) + (k - 1) * u * ref["kl_terms"].abs().sum(-1)
    # dmu = dlogp (d / var), dlogp = ((g0 (1 / rows)) coefficient) ratio: 1 / rows (1), g0 times it (1), times the
    # coefficient (1), times the ratio (1), d (1), var (1), d / var (1), the product (1) = 8 u, and the ratio's
    # relative error (torch's autograd chain has 7)
    e_dmu = ref["dmu"].abs() * (8 * u + rel_ratio)[:, None] + 8 * TINY
    # rows of dstd: dlogp (d^2 / (var sigma) - 1 / sigma): dlogp (4), d^2 (3), var sigma (2), the quotient (1), 1 /
    # sigma (1), the subtraction (1), the product (1) = 13 u at the magnitude |dlogp| (d^2 / sigma^3 + 1 / sigma)
    mag = d * d / (var * sd) + 1.0 / sd
    e_ds = ref["dlogp"].abs()[:, None] * mag * (13 * u + rel_ratio)[:, None] + 13 * TINY
    full_ds = (abs(g[0]) / rows * A.abs() * ratio)[:, None] * mag  # an exempt row's term, were it on the other side
    # dvalue = gv inner, gv = (coef g) (1 / rows): 3 roundings, the product 1
    gv = abs(g[1]) / rows
    if clipped_value:
        tie = l1 == l2
        one = torch.where(l1 > l2, 2 * e_a, 2 * e_b * vin)
        # a float64 tie inside the clip (v_c = v): fp32 may take either branch whole; beyond it (exact in fp32 too) the
        # half weights stand: a (1) and the addition (1)
        both = torch.where(vin, 2 * torch.maximum(e_a, e_b), e_a) + u * (ref["dvalue"].abs() / max(gv, TINY))
        e_inner = torch.where(tie, both, one)
        e_dvalue = gv * e_inner + 4 * u * ref["dvalue"].abs() + 5 * TINY
    else:
        e_dvalue = 5 * u * ref["dvalue"].abs() + 5 * TINY  # a = v - ret (1) more
    # the sums: the rows' bounds, the reduction's, and for an exempt row both branches' bounds (forward) or its whole
    # term (dstd, whose gradient jumps at the clip)
    ex = exempt.double()
    e_sum0 = e_surr.sum() + SUM_REL * (ref["surr"].abs().sum() + 1.0) + (ex * (e_s1 + e_s2)).sum()
    e_sum1 = e_vterm.sum() + SUM_REL * (ref["vterm"].abs().sum() + 1.0)
    if clipped_value:
        e_sum1 = e_sum1 + (ex * (e_l1 + e_l2)).sum()
    e_sum2 = e_kl.sum() + SUM_REL * (ref["kl"].abs().sum() + 1.0)
    e_sums = torch.stack([e_sum0, e_sum1, e_sum2])
    # means: 1 / rows (1) and the product (1); loss: value_coef times the mean (1) and the addition (1)
    e_means = e_sums / rows + 2 * u * ref["means"].abs()
    e_loss = (e_means[0] + abs(value_coef) * e_means[1] + u * abs(value_coef) * ref["means"][1].abs()
              + u * ref["loss"].abs())
    e_dstd = e_ds.sum(0) + SUM_REL * (ref["ds"].abs().sum(0) + 1.0) + (ex[:, None] * full_ds).sum(0)
    return dict(dmu=e_dmu, dvalue=e_dvalue, exempt=exempt, sums=e_sums, means=e_means, loss=e_loss, dstd=e_dstd)


def loss_ratios(got, ref, bnd):
    """The largest |got - ref| / bound per family: `rows` (dmu and dvalue, the exempt rows left out) and `sums` (the
    sums, the means, the loss and dstd).  got: dict of dmu, dvalue, sums, means, loss, dstd."""
    keep = ~bnd["exempt"]
    per_row = [((got["dmu"].double() - ref["dmu"]).abs() / bnd["dmu"])[keep],
               ((got["dvalue"].double() - ref["dvalue"]).abs() / bnd["dvalue"])[keep]]
    rows = max([float(x.max()) for x in per_row if x.numel()] + [0.0])
    sums = max(float(((got[n].double() - ref[n]).abs() / bnd[n]).max()) for n in ("sums", "means", "loss", "dstd"))
    nan = any(bool(torch.isnan(x).any()) for x in per_row) or any(
        bool(torch.isnan(got[n].double()).any()) for n in ("sums", "means", "loss", "dstd"))
    return dict(rows=float("inf") if nan else rows, sums=float("inf") if nan else sums)


# --------------------------------------------------------------------------------------------------- Adam, clip
T_STEPS = (1, 2, 10, 1000, 100000, 5000000)
LAYOUT_A = (1, 255, 256, 1023, 1024, 1025, 4097, 3072)


def adam_layout(name):
    """Segment sizes of layout `a`, `a_rev`, `b` (64 segments, the maximum: sizes cycling 1..7, one of 5000) or `c`."""
    if name == "a":
        return list(LAYOUT_A)
    if name == "a_rev":
        return list(reversed(LAYOUT_A))
    if name == "b":
        return [5000 if s == 40 else 1 + s % 7 for s in range(64)]
    return [1]


def adam_state(n, seed):
    """A random fp32 state of n elements (p, g, m, v >= 0), with the cases a wrong denominator shows on: every 16th
    element has v = 0, g = 0 and a moment of 1e-9 (the denominator is eps alone), every 16th + 1 a second moment near
    1e-14 (sqrt(v) of eps's size)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.1
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01
    i = torch.arange(n)
    z = i % 16 == 3
    g = torch.where(z, torch.zeros(()), g)
    v = torch.where(z, torch.zeros(()), v)
    m = torch.where(z, torch.full((), 1.0e-9), m)
    s = i % 16 == 4
    v = torch.where(s, torch.full((), 1.0e-14) * (1.0 + i % 5), v)
    g = torch.where(s, g * 1.0e-6, g)
    return p.float(), g.float(), m.float(), v.float()


def adam_ref(p, g, m, v, t, lr, betas, eps):
    """One step of torch's Adam in float64 from the fp32 state (p, g, m, v) at step count t (the count after this
    step): m + (1 - b1) (g - m); v b2 + (1 - b2) g g; p - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    Returns (p, m, v) and the intermediates the bounds need."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2 = betas
    eps = f32(eps)  # (the kernel's eps is a float)
    m2 = m + (1.0 - b1) * (g - m)
    v2 = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    bc2s = math.sqrt(1.0 - b2 ** t)
    den = v2.sqrt() / bc2s + eps
    upd = -step_size * (m2 / den)
    return p + upd, m2, v2, dict(den=den, upd=upd, step_size=step_size, bc2s=bc2s, p=p, g=g, m=m, v=v, eps=eps,
                                 b1=b1, b2=b2)


def adam_bounds(p2, m2, v2, x):
    """Bounds (e_p, e_m, e_v) on one fp32 Adam step against adam_ref, from its intermediates x."""
    u, L = U, LIBM
    b1, b2, g, m, v = x["b1"], x["b2"], x["g"], x["m"], x["v"]
    # m: g - m (1), the weight 1 - b1 rounded (1), their product (1), the addition (1)
    e_m = 3 * u * ((1.0 - b1) * (g - m)).abs() + u * m2.abs() + 4 * TINY
    # v: b2 rounded (1) and v b2 (1); 1 - b2 rounded (1), times g (1), times g (1); the addition (1)
    e_v = 2 * u * v * b2 + 3 * u * (1.0 - b2) * g * g + u * v2 + 6 * TINY
    # denominator: sqrt at L with v's error through it (|sqrt a - sqrt b| <= min(|a - b| / (2 sqrt a), sqrt |a - b|));
    # sqrt(1 - b2^t) rounded (1) and the quotient (1); eps rounded (1); the addition (1)
    s = v2.sqrt()
    e_s = torch.minimum(e_v / (2 * s).clamp_min(TINY), e_v.sqrt()) + L * s
    den = x["den"]
    e_den = e_s / x["bc2s"] + 2 * u * s / x["bc2s"] + u * x["eps"] + u * den
    # update: m / den (1) with both errors; lr / (1 - b1^t) rounded (1) and the product (1); p + update (1)
    step = abs(x["step_size"])
    e_p = step * (e_m / den + m2.abs() * e_den / (den * den)) + 3 * u * x["upd"].abs() + u * p2.abs() + 4 * TINY
    return e_p, e_m, e_v


def clip_ref(grads, max_norm):
    """(norm, coefficient) of clip_grad_norm_ in float64: min(1, max_norm / (norm + 1e-6))."""
    total = sum(float((x.double() ** 2).sum()) for x in grads)
    norm = math.sqrt(total)
    return norm, min(1.0, max_norm / (norm + 1.0e-6))


def clip_grad_bound(g, coef):
    """Bound on a clipped gradient g coef: the norm's square root at L, + 1e-6 (the constant 1, the addition 1), the
    quotient (1) and the product (1)."""
    return (LIBM + 4 * U) * (g.double() * coef).abs() + 4 * TINY


def norm_within_2ulp(got, norm):
    """got (fp32) within 2 ulp of the fp32-rounded float64 norm."""
    want = np.float32(norm)
    return abs(float(got) - float(want)) <= 2.0 * float(np.spacing(want)) if want > 0 else float(got) == 0.0


# ---------------------------------------------------------------------------------------------- the rate rule
def adaptive_lr_ref(kl, lr, desired_kl, lr_min, lr_max):
    """PPO._adapt_learning_rate's ordering in numpy fp32, the thresholds the Python doubles desired_kl * 2.0 and
    desired_kl / 2.0 rounded to fp32."""
    kl, lr = np.float32(kl), np.float32(lr)
    hi, lo = np.float32(desired_kl * 2.0), np.float32(desired_kl / 2.0)
    lr_min, lr_max = np.float32(lr_min), np.float32(lr_max)
    with np.errstate(all="ignore"):
        if kl > hi:
            return max(lr_min, np.float32(lr / np.float32(1.5)))
        if lo > kl and kl > np.float32(0.0):
            return min(lr_max, np.float32(lr * np.float32(1.5)))
    return lr


def adaptive_lr_table(desired_kl, lr_min=1.0e-5, lr_max=1.0e-2):
    """(kl, lr) pairs: kl either side of, and at, fp32(2 desired) and fp32(desired / 2), 0, -1e-3, NaN, +inf; rates
    at lr_min, at lr_max, within a factor 1.5 of each, and mid-range."""
    hi, lo = np.float32(desired_kl * 2.0), np.float32(desired_kl / 2.0)
    inf = np.float32(np.inf)
    kls = [np.nextafter(hi, -inf), hi, np.nextafter(hi, inf), np.nextafter(lo, -inf), lo, np.nextafter(lo, inf),
           np.float32(0.0), np.float32(-1.0e-3), np.float32(np.nan), inf]
    lrs = [np.float32(x) for x in (lr_min, lr_max, lr_min * 1.2, lr_max / 1.2, 1.0e-3)]
    return [(k, r) for k in kls for r in lrs]


# ------------------------------------------------------------------------------------------------- recording
_RATIOS = {}


def record(who, family, ratio):
    """Keep the largest error / bound ratio seen per family for `who` (cpu_fp32_stand_in or gpu); written to the file
    GR_UPDATE_ERROR_BUDGET names, when set (profiles/update_kernels_error_budget.json is made that way)."""
    key = (who, family)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), float(ratio))
    path = os.environ.get("GR_UPDATE_ERROR_BUDGET")
    if path:
        data = {}
        if os.path.exists(path):
            with open(path) as fh:
                data = json.load(fh)
        cur = data.setdefault(who, {})
        cur[family] = max(cur.get(family, 0.0), float(ratio))
        with open(path, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
