"""Float64 restatement of the differentiable window (torch autograd over explicit per-component formulas).

What the reference's diff_rl workflow computes per env over a window t = 0..T-1 (ManagerBasedDiffRLEnv.step:
manager_based_diff_rl_env.py:205-257; CTBRController.compute: controller_diff.py:120-138; DroneDynamics.step / align:
droneDynamics.py:119-135, 156-180; the losses: mdp/losses.py:72-117; BPTT's mean: algorithms/bptt.py:38-45), fed the
window's per-step fields ("tape"): the pre-step state is the linearisation point, the nominal model's gradient is
grafted onto it with the decay gamma (align), a reset cuts what comes back from the step after.

    window(tape, consts) -> {"losses" [T, N], "terms" [T, N, 3], "grad" [T, N, 4]}

tape: dict of [T, N, k] tensors (any float dtype; computed in `dtype`):
    p 3, q 4 (w, x, y, z), v 3 (world), w 3 (body), al 3, T 1, tau 3 (pre-step), u 4 (the squashed action applied),
    thr 1, k2 3, k1 3, Kp 3, cT 1, Kd 3, mp 1, ct 3, mc 1, J 3, xp 13 (post-step p, q, v, w values), goal 3, done 1
consts: dt, gravity, thrust_ratio, rate_bound, thrust_lo, thrust_hi, inertia (3, nominal), dr_plant, lag, gamma,
    weights (3), scale
a (optional, [T, N, 4] raw actions): u_t = tanh(a_{t - lag}) for t >= lag (an action from before the window is the
    tape's constant u); without it the tape's u is the leaf and grad = dL/du * (1 - u^2), shifted by the lag.
"grad" is scale * d(sum of losses)/d(raw action); with lag 1 step t's contribution lands on row t - 1, row T - 1 is 0.
"""
from __future__ import annotations

import torch


def _rot(q, v, sign):
    """Isaac Lab quat_rotate (sign +1) / quat_rotate_inverse (sign -1): the explicit, un-normalised formula."""
    qw, qx, qy, qz = q
    s = 2.0 * qw * qw - 1.0
    cx = qy * v[2] - qz * v[1]
    cy = qz * v[0] - qx * v[2]
    cz = qx * v[1] - qy * v[0]
    d = qx * v[0] + qy * v[1] + qz * v[2]
    return [v[0] * s + sign * cx * qw * 2.0 + qx * d * 2.0,
            v[1] * s + sign * cy * qw * 2.0 + qy * d * 2.0,
            v[2] * s + sign * cz * qw * 2.0 + qz * d * 2.0]


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
            w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _cols(x):
    return [x[:, i] for i in range(x.shape[1])]


def _graft(nominal, value, gamma):
    """align: the value of `value`, the gradient of `nominal` decayed by gamma."""
    return gamma * (nominal - nominal.detach()) + value


def window(tape: dict, consts: dict, a: torch.Tensor | None = None, dtype=torch.float64) -> dict:
    tp = {k: v.to(dtype) for k, v in tape.items()}
    T, N = tp["p"].shape[:2]
    lag, gamma = int(consts["lag"]), float(consts["gamma"])
    dt, gz = float(consts["dt"]), float(consts["gravity"])
    lo, hi, rb = float(consts["thrust_lo"]), float(consts["thrust_hi"]), float(consts["rate_bound"])
    Jn = [float(x) for x in consts["inertia"]]
    w_t, w_v, w_f = [float(x) for x in consts["weights"]]
    if a is not None:
        leaf = a.detach().to(dtype).clone().requires_grad_(True)
    else:
        leaf = tp["u"].detach().clone().requires_grad_(True)
    losses, terms = [], []
    nom = None     # the nominal x+ of the step before, columns p q v w (with gradient)
    nomf = None    # the nominal (T+, tau+) of the step before
    cut = torch.ones(N, dtype=torch.bool)  # the step before reset the env (or there is none)
    total = 0.0
    for t in range(T):
        x_val = torch.cat([tp["p"][t], tp["q"][t], tp["v"][t], tp["w"][t]], dim=1)
        f_val = torch.cat([tp["T"][t], tp["tau"][t]], dim=1)
        if nom is None:
            x, f = x_val, f_val
        else:
            keep = (~cut).to(dtype)[:, None]
            x = x_val + keep * gamma * (nom - nom.detach())
            f = f_val + keep * (nomf - nomf.detach())   # the filter state is not decayed
        p, q, v, w = _cols(x[:, 0:3]), _cols(x[:, 3:7]), _cols(x[:, 7:10]), _cols(x[:, 10:13])
        # the action applied
        if a is not None:
            u = torch.tanh(leaf[t - lag]) if t >= lag else tp["u"][t]
        else:
            u = leaf[t]
        u = _cols(u)
        mc, thr = tp["mc"][t][:, 0], tp["thr"][t][:, 0]
        s0 = mc * gz * float(consts["thrust_ratio"]) / 2.0
        cmd = [(u[0] * s0 + s0) * thr, u[1] * rb, u[2] * rb, u[3] * rb]
        # controller (no motor model); w_b and alpha_b enter detached
        wd = [c.detach() for c in w]
        al = _cols(tp["al"][t])
        cT, ct = tp["cT"][t][:, 0], _cols(tp["ct"][t])
        Kp, Kd = _cols(tp["Kp"][t]), _cols(tp["Kd"][t])
        Tn = (1.0 - cT) * torch.clamp(cmd[0], lo, hi) + cT * f[:, 0]
        cr = _cross(wd, [Jn[i] * wd[i] for i in range(3)])
        taun = []
        for i in range(3):
            tdes = Jn[i] * (Kp[i] * (torch.clamp(cmd[i + 1], -rb, rb) - wd[i])) + cr[i] - Kd[i] * al[i]
            taun.append((1.0 - ct[i]) * tdes + ct[i] * f[:, i + 1])
        # dynamics (DroneDynamics.step) at the pre-step state
        if consts["dr_plant"]:
            m, J = tp["mp"][t][:, 0], _cols(tp["J"][t])
        else:
            m, J = mc, [torch.full_like(mc, Jn[i]) for i in range(3)]
        k2, k1 = _cols(tp["k2"][t]), _cols(tp["k1"][t])
        vb = _rot(q, v, -1.0)
        fb = [-(k2[i] * vb[i]) * vb[i].abs() - k1[i] * vb[i] for i in range(3)]
        fb[2] = fb[2] + Tn
        tw = _rot(q, fb, 1.0)
        acc = [tw[0] / m, tw[1] / m, tw[2] / m - gz]
        crp = _cross(w, [J[i] * w[i] for i in range(3)])
        alp = [(taun[i] - crp[i]) / J[i] for i in range(3)]
        pn = [p[i] + v[i] * dt + 0.5 * acc[i] * dt * dt for i in range(3)]
        qd = _qmul(q, [torch.zeros_like(w[0]), w[0], w[1], w[2]])
        qn = [q[i] + 0.5 * qd[i] * dt for i in range(4)]
        nq = torch.sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3])
        qn = [c / nq for c in qn]
        vn = [v[i] + acc[i] * dt for i in range(3)]
        wn = [w[i] + alp[i] * dt for i in range(3)]
        nom = torch.stack(pn + qn + vn + wn, dim=1)
        nomf = torch.stack([Tn] + taun, dim=1)
        # the loss on the aligned post-step state (values: the step's own x+)
        xa = _graft(nom, tp["xp"][t], gamma)
        g = tp["goal"][t]
        d2 = ((g - xa[:, 0:3]) ** 2).sum(dim=1)
        safe = torch.where(d2 > 0, d2, torch.ones_like(d2))
        dist = torch.where(d2 > 0, torch.sqrt(safe), torch.zeros_like(d2))  # gradient 0 at 0
        z = xa[:, 2]
        tr = torch.stack([w_t * dist, w_v * (xa[:, 7:10] ** 2).mean(dim=1), w_f / (1.0 + z + 10.0 * z * z)], dim=1)
        terms.append(tr.detach())
        losses.append(tr.detach().sum(dim=1))
        total = total + tr.sum()
        cut = tp["done"][t][:, 0] != 0
    (gl,) = torch.autograd.grad(total * float(consts["scale"]), leaf)
    if a is None:
        gu = gl * (1.0 - tp["u"] ** 2)
        grad = torch.zeros_like(gu)
        if lag:
            grad[:T - lag] = gu[lag:]
        else:
            grad = gu
    else:
        grad = gl
    return {"losses": torch.stack(losses), "terms": torch.stack(terms), "grad": grad}


TAPE_FIELDS = ("p", "q", "v", "w", "al", "T", "tau", "u", "thr", "k2", "k1", "Kp", "cT", "Kd", "mp", "ct", "mc", "J",
               "xp", "goal", "done")


def tape_fields(tape: torch.Tensor) -> dict:
    """[T, GR_DIFF_PLANES, N, 4] tape rows (include/gr.h GR_DT_*) -> the named fields, [T, N, k]."""
    (POSQ, QV, VW, WA, CTRL, U, RST0, RST1, PAR0, PAR1, PAR2, PAR3, TT, XP0, XP1, XP2, XP3, GOAL) = range(18)
    c = torch.cat
    P = lambda i: tape[:, i]  # noqa: E731
    return {
        "p": P(POSQ)[..., 0:3], "q": c([P(POSQ)[..., 3:4], P(QV)[..., 0:3]], -1),
        "v": c([P(QV)[..., 3:4], P(VW)[..., 0:2]], -1), "w": c([P(VW)[..., 2:4], P(WA)[..., 0:1]], -1),
        "al": P(WA)[..., 1:4], "T": P(CTRL)[..., 0:1], "tau": P(CTRL)[..., 1:4], "u": P(U),
        "thr": P(RST0)[..., 0:1], "k2": c([P(RST0)[..., 2:4], P(RST1)[..., 0:1]], -1), "k1": P(RST1)[..., 1:4],
        "Kp": P(PAR0)[..., 0:3], "cT": P(PAR0)[..., 3:4], "Kd": P(PAR1)[..., 0:3], "mp": P(PAR1)[..., 3:4],
        "ct": P(PAR2)[..., 0:3], "mc": P(PAR2)[..., 3:4], "J": P(PAR3)[..., 0:3],
        "xp": c([P(XP0), P(XP1), P(XP2), P(XP3)[..., 0:1]], -1), "tt": P(TT),
        "goal": P(GOAL)[..., 0:3], "done": P(GOAL)[..., 3:4],
    }
