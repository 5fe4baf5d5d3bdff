"""The differentiable window's tape and its three calls (include/gr.h, ABI 14: gr_diff_record, gr_diff_loss,
gr_diff_backward), and a torch path that computes the same window by autograd from the same planes.

The reference keeps a torch graph over `env.step` for the whole window (ManagerBasedDiffRLEnv.step,
manager_based_diff_rl_env.py:205-257; algorithms/bptt.py:38-45).  Here no graph crosses the step: per step two small
launches write a tape row ([GR_DIFF_PLANES, N, 4] float planes, layout in include/gr.h), per window one reverse-time
launch returns d(mean loss)/d(raw action) [T, N, 4].  `fused=False` runs the same three stages in torch (the adjoint by
autograd over the window, the reference's structure); it also runs on the CPU and in float64.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _abi

LOSS_TERMS = ("racing_target", "racing_vel", "racing_falling")


def window_consts(gcfg, weights=(1.0, 0.05, 0.5), gamma=0.92) -> dict:
    """What the window needs of a gr_config (the values gr_diff.hip's launches take from the context)."""
    k2, k1, k0 = (float(x) for x in gcfg.thrustmap)
    w0, w1 = (float(x) for x in gcfg.motor_omega)
    return {
        "dt": float(gcfg.step_dt), "gravity": float(gcfg.gravity), "thrust_ratio": float(gcfg.max_thrust_weight_ratio),
        "rate_bound": float(gcfg.body_rate_bound),
        "thrust_lo": float(np.float32((k2 * w0 * w0 + k1 * w0 + k0) * 4.0)),
        "thrust_hi": float(np.float32((k2 * w1 * w1 + k1 * w1 + k0) * 4.0)),
        "inertia": [float(x) for x in gcfg.inertia], "dr_plant": int(gcfg.dr_plant), "lag": int(gcfg.action_lag),
        "gamma": float(gamma), "weights": [float(w) for w in weights],
        "num_levels": int(gcfg.num_levels), "max_gates": int(gcfg.max_gates), "num_types": int(gcfg.num_types),
    }


def lean_error(gcfg) -> str | None:
    """Why a configuration cannot be differentiated (None: it can): the window restates the explicit integrator
    without the motor model and without per-env rotor constants."""
    bad = []
    if int(gcfg.integrator) != _abi.GR_INTEGRATOR_DD_EXPLICIT:
        bad.append("integrator must be 'dd_explicit'")
    if int(gcfg.use_motor_model):
        bad.append("use_motor_model must be 0")
    if int(gcfg.dr_rotor):
        bad.append("dr_rotor must be 0")
    if int(gcfg.action_lag) not in (0, 1):
        bad.append("action_lag must be 0 or 1")
    return "; ".join(bad) if bad else None


# ------------------------------------------------------------------ torch path
def _rot(q, v, sign):
    """Isaac Lab quat_rotate (+1) / quat_rotate_inverse (-1), the explicit formula (not normalising q)."""
    qw, qv = q[:, 0:1], q[:, 1:4]
    a = v * (2.0 * qw * qw - 1.0)
    b = torch.linalg.cross(qv, v, dim=1) * qw * 2.0
    c = qv * (qv * v).sum(dim=1, keepdim=True) * 2.0
    return a + sign * b + c


def _qmul(a, b):
    aw, av, bw, bv = a[:, 0:1], a[:, 1:4], b[:, 0:1], b[:, 1:4]
    return torch.cat([aw * bw - (av * bv).sum(dim=1, keepdim=True),
                      aw * bv + bw * av + torch.linalg.cross(av, bv, dim=1)], dim=1)


def _fields(row):
    """[GR_DIFF_PLANES or more, N, 4] planes in the GR_DT_* order -> the pre-step fields."""
    a = _abi
    cat = torch.cat
    return {
        "p": row[a.DT_POSQ][:, 0:3], "q": cat([row[a.DT_POSQ][:, 3:4], row[a.DT_QV][:, 0:3]], 1),
        "v": cat([row[a.DT_QV][:, 3:4], row[a.DT_VW][:, 0:2]], 1), "w": cat([row[a.DT_VW][:, 2:4], row[a.DT_WA][:, 0:1]], 1),
        "al": row[a.DT_WA][:, 1:4], "T": row[a.DT_CTRL][:, 0:1], "tau": row[a.DT_CTRL][:, 1:4], "u": row[a.DT_U],
        "thr": row[a.DT_RST0][:, 0:1], "k2": cat([row[a.DT_RST0][:, 2:4], row[a.DT_RST1][:, 0:1]], 1),
        "k1": row[a.DT_RST1][:, 1:4], "Kp": row[a.DT_PAR0][:, 0:3], "cT": row[a.DT_PAR0][:, 3:4],
        "Kd": row[a.DT_PAR1][:, 0:3], "mp": row[a.DT_PAR1][:, 3:4], "ct": row[a.DT_PAR2][:, 0:3],
        "mc": row[a.DT_PAR2][:, 3:4], "J": row[a.DT_PAR3][:, 0:3],
    }


def _step(f, x, filt, u, k):
    """Controller + integrator of one step: state x [N, 13] (p q v w), filters [N, 4], squashed action u -> (x+, filt+).
    w_b and alpha_b enter the controller detached (controller_diff.py:123)."""
    p, q, v, w = x[:, 0:3], x[:, 3:7], x[:, 7:10], x[:, 10:13]
    Jn = torch.tensor(k["inertia"], dtype=x.dtype, device=x.device)
    s0 = f["mc"] * k["gravity"] * k["thrust_ratio"] / 2.0
    cmd0 = (u[:, 0:1] * s0 + s0) * f["thr"]
    rates = torch.clamp(u[:, 1:4] * k["rate_bound"], -k["rate_bound"], k["rate_bound"])
    Tn = (1.0 - f["cT"]) * torch.clamp(cmd0, k["thrust_lo"], k["thrust_hi"]) + f["cT"] * filt[:, 0:1]
    wd = w.detach()
    tdes = Jn * (f["Kp"] * (rates - wd)) + torch.linalg.cross(wd, Jn * wd, dim=1) - f["Kd"] * f["al"]
    taun = (1.0 - f["ct"]) * tdes + f["ct"] * filt[:, 1:4]
    m, J = (f["mp"], f["J"]) if k["dr_plant"] else (f["mc"], Jn.expand_as(w))
    vb = _rot(q, v, -1.0)
    fb = -(f["k2"] * vb) * vb.abs() - f["k1"] * vb
    fb = fb + torch.cat([torch.zeros_like(Tn), torch.zeros_like(Tn), Tn], dim=1)
    acc = _rot(q, fb, 1.0) / m
    acc = acc - torch.tensor([0.0, 0.0, k["gravity"]], dtype=x.dtype, device=x.device)
    alp = (taun - torch.linalg.cross(w, J * w, dim=1)) / J
    dt = k["dt"]
    pn = p + v * dt + 0.5 * acc * dt * dt
    qn = q + 0.5 * _qmul(q, torch.cat([torch.zeros_like(Tn), w], dim=1)) * dt
    qn = qn / qn.norm(dim=1, keepdim=True)
    return torch.cat([pn, qn, v + acc * dt, w + alp * dt], dim=1), torch.cat([Tn, taun], dim=1)


def _terms(xp, goal, k):
    d2 = ((goal - xp[:, 0:3]) ** 2).sum(dim=1)
    pos = d2 > 0
    dist = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    z = xp[:, 2]
    w = k["weights"]
    return torch.stack([w[0] * dist, w[1] * (xp[:, 7:10] ** 2).mean(dim=1), w[2] / (1.0 + z + 10.0 * z * z)], dim=1)


def torch_record(state: torch.Tensor, actions: torch.Tensor | None, k: dict, u: torch.Tensor | None = None) -> torch.Tensor:
    """gr_diff_record in torch: the tape row [GR_DIFF_PLANES, N, 4] of the step about to be taken from the pre-step
    state planes [GR_NUM_PLANES, N, 4] (values only).  u: the squashed action the step applies, if the caller keeps
    it in a wider type than the lag plane's float32."""
    a = _abi
    with torch.no_grad():
        row = state.new_zeros(a.GR_DIFF_PLANES, state.shape[1], 4)
        for dst, src in ((a.DT_POSQ, a.P_POSQ), (a.DT_QV, a.P_QV), (a.DT_VW, a.P_VW), (a.DT_WA, a.P_WA),
                         (a.DT_CTRL, a.P_CTRL), (a.DT_RST0, a.P_RST0), (a.DT_RST1, a.P_RST1), (a.DT_PAR0, a.P_PAR0),
                         (a.DT_PAR1, a.P_PAR1), (a.DT_PAR2, a.P_PAR2), (a.DT_PAR3, a.P_PAR3)):
            row[dst] = state[src]
        if u is not None:
            row[a.DT_U] = u
        else:
            row[a.DT_U] = state[a.P_LAG] if k["lag"] else torch.tanh(actions.to(state.dtype))
        f = _fields(row)
        xp, fp = _step(f, torch.cat([f["p"], f["q"], f["v"], f["w"]], 1), torch.cat([f["T"], f["tau"]], 1), f["u"], k)
        row[a.DT_TT] = fp
        row[a.DT_XP0], row[a.DT_XP1], row[a.DT_XP2] = xp[:, 0:4], xp[:, 4:8], xp[:, 8:12]
        row[a.DT_XP3][:, 0] = xp[:, 12]
    return row


def torch_loss(row: torch.Tensor, gates: torch.Tensor, packed: torch.Tensor, dones: torch.Tensor, k: dict):
    """gr_diff_loss in torch: fills the row's GR_DT_GOAL plane (gate centre after the step, done flag) and returns
    (loss [N], terms [N, 3]).  gates [T*L, max_gates, GR_GATE_FLOATS]; packed: the post-step GR_I_PACKED words."""
    a = _abi
    with torch.no_grad():
        packed = packed.to(torch.int64)
        gate = (packed & 0xFF).clamp(max=k["max_gates"] - 1)
        lvl = ((packed >> 8) & 0xFF).clamp(max=k["num_levels"] - 1)
        typ = ((packed >> 24) & 0xFF).clamp(max=k["num_types"] - 1)
        goal = gates.to(row.device)[typ * k["num_levels"] + lvl, gate, 0:3].to(row.dtype)
        row[a.DT_GOAL][:, 0:3] = goal
        row[a.DT_GOAL][:, 3] = (dones != 0).to(row.dtype)
        xp = torch.cat([row[a.DT_XP0], row[a.DT_XP1], row[a.DT_XP2], row[a.DT_XP3][:, 0:1]], dim=1)
        terms = _terms(xp, goal, k)
    return terms.sum(dim=1), terms


def torch_backward(tape: torch.Tensor, k: dict, scale: float) -> torch.Tensor:
    """gr_diff_backward by autograd over the window's torch graph, linearised at the tape's pre-step planes: the
    nominal model's gradient is grafted onto each step's state with the decay gamma (DroneDynamics.align), the filter
    state's undecayed, both cut where the step before reset the env.  tape [T, GR_DIFF_PLANES, N, 4] ->
    scale * d(sum of losses)/d(raw action) [T, N, 4]."""
    a = _abi
    T = tape.shape[0]
    lag, gamma = k["lag"], k["gamma"]
    with torch.enable_grad():
        leaf = tape[:, a.DT_U].detach().clone().requires_grad_(True)
        nom = nomf = keep = None
        total = 0.0
        for t in range(T):
            row = tape[t]
            f = _fields(row)
            x = torch.cat([f["p"], f["q"], f["v"], f["w"]], dim=1)
            filt = torch.cat([f["T"], f["tau"]], dim=1)
            if nom is not None:
                x = x + keep * gamma * (nom - nom.detach())
                filt = filt + keep * (nomf - nomf.detach())
            nom, nomf = _step(f, x, filt, leaf[t], k)
            xp = torch.cat([row[a.DT_XP0], row[a.DT_XP1], row[a.DT_XP2], row[a.DT_XP3][:, 0:1]], dim=1)
            xa = gamma * (nom - nom.detach()) + xp
            total = total + _terms(xa, row[a.DT_GOAL][:, 0:3], k).sum()
            keep = (row[a.DT_GOAL][:, 3:4] == 0).to(tape.dtype)
        (gu,) = torch.autograd.grad(total * scale, leaf)
    gu = gu * (1.0 - tape[:, a.DT_U] ** 2)
    if not lag:
        return gu
    out = torch.zeros_like(gu)
    out[:T - 1] = gu[1:]
    return out


# ------------------------------------------------------------------ the tape
class DiffTape:
    """The tape of one env: `t_max` rows, the per-step losses, and the three stages (fused HIP or torch)."""

    def __init__(self, ctx, gcfg, t_max: int, device, fused: bool = True, weights=(1.0, 0.05, 0.5), gamma=0.92,
                 dtype=torch.float32):
        why = lean_error(gcfg)
        if why is not None:
            raise ValueError(f"the configuration cannot be differentiated: {why}")
        self.ctx, self.fused, self.t_max = ctx, bool(fused), int(t_max)
        self.device = torch.device(device)
        self.k = window_consts(gcfg, weights, gamma)
        n = self.num_envs = int(gcfg.num_envs)
        if self.t_max < 1:
            raise ValueError("t_max must be at least 1")
        if self.t_max * _abi.GR_DIFF_PLANES * n >= 2 ** 31:
            raise ValueError(f"a tape of {self.t_max} rows of {n} envs exceeds the adjoint kernel's 32-bit offsets")
        if self.fused and (self.device.type != "cuda" or dtype != torch.float32):
            raise ValueError("the fused path runs in float32 on the GPU")
        self.tape = torch.zeros(self.t_max, _abi.GR_DIFF_PLANES, n, 4, dtype=dtype, device=self.device)
        self.losses = torch.zeros(self.t_max, n, dtype=dtype, device=self.device)
        self.terms = torch.zeros(self.t_max, n, 3, dtype=dtype, device=self.device)
        self.grad = torch.zeros(self.t_max, n, 4, dtype=dtype, device=self.device)
        self.cursor = 0
        if self.fused:
            rf = _abi.load().gr_diff_row_floats(ctx)
            if rf != _abi.GR_DIFF_PLANES * n * 4:
                raise RuntimeError(f"gr_diff_row_floats reports {rf} floats per tape row, expected "
                                   f"{_abi.GR_DIFF_PLANES * n * 4}")
            w = (C.c_float * 3)(*[float(x) for x in weights])
            _abi.call("gr_diff_config", w, C.c_float(gamma), ctx=ctx)

    def rewind(self):
        self.cursor = 0

    def check_room(self):
        if self.cursor >= self.t_max:
            raise RuntimeError(f"the tape holds {self.t_max} steps: call detach() before stepping further")

    def record(self, state: torch.Tensor, actions: torch.Tensor, u: torch.Tensor | None = None):
        """Before the step: write row `cursor` from the pre-step planes (u: torch_record's, torch path only)."""
        self.check_room()
        if self.fused:
            _abi.call("gr_diff_record", actions.data_ptr(), self.tape[self.cursor].data_ptr(),
                      _abi.raw_stream(self.device), ctx=self.ctx)
        else:
            self.tape[self.cursor] = torch_record(state.to(self.tape.dtype), actions, self.k, u)

    def loss(self, gates: torch.Tensor, packed: torch.Tensor, dones: torch.Tensor):
        """After the step: the row's losses; advances the cursor.  Returns (loss [N], terms [N, 3]) views."""
        t = self.cursor
        if self.fused:
            _abi.call("gr_diff_loss", gates.data_ptr(), self.tape[t].data_ptr(), self.losses[t].data_ptr(),
                      self.terms[t].data_ptr(), _abi.raw_stream(self.device), ctx=self.ctx)
        else:
            self.losses[t], self.terms[t] = torch_loss(self.tape[t], gates, packed, dones, self.k)
        self.cursor = t + 1
        return self.losses[t], self.terms[t]

    def backward(self, scale: float) -> torch.Tensor:
        """d(scale * sum of the recorded losses)/d(raw action) over the rows since the last rewind, [T, N, 4]."""
        T = self.cursor
        if T < 1:
            raise RuntimeError("no step recorded since detach()")
        if self.fused:
            _abi.call("gr_diff_backward", self.tape.data_ptr(), T, C.c_float(scale), self.grad.data_ptr(),
                      _abi.raw_stream(self.device), ctx=self.ctx)
            return self.grad[:T]
        return torch_backward(self.tape[:T], self.k, float(scale))
