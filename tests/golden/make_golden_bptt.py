"""Generate tests/golden/golden_bptt.npz from the reference's own classes in float64 (data only).

Driven: DroneDynamics.step / align / reset_idx / reset_state / detach, CTBRController.compute / reset_idx / detach, the
three racing loss functions (mdp/losses.py) with LossesCfg's weights summed as LossManager.compute does, and the mean of
BPTT.update.  Composition in the order of ManagerBasedDiffRLEnv.step, the plant state taken as nominal.detach().
Cases: T = 6, N = 48, action lag 0 and 1; per-env gains, delays, mass, inertia and drag; resets injected at steps 0, 3
and 5; gate centres given per step.  Needs the reference checkout that
il_shim.py locates:

    python tests/golden/make_golden_bptt.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import il_shim  # noqa: E402
from make_golden import CTBRCfg, DT, INERTIA, MASS, load_reference  # noqa: E402

T, N, GAMMA = 6, 48, 0.92
WEIGHTS = (1.0, 0.05, 0.5)
RESETS = {0: [0], 3: [20, 21], 5: [47]}


def main():
    torch.set_default_dtype(torch.float64)
    DroneDynamics, CTBRController, _ = load_reference()
    envs = types.ModuleType("diff.lab.envs")  # (losses.py imports the env class for its annotations only)
    envs.ManagerBasedDiffRLEnv = object
    sys.modules["diff.lab.envs"] = envs
    losses = il_shim.load("grref_mdp_losses", os.path.join(il_shim.MDP_DIR, "losses.py"))
    g = torch.Generator().manual_seed(20251021)
    R = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    Nn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = {"T": T, "N": N, "gamma": GAMMA, "weights": np.array(WEIGHTS), "dt": DT, "inertia_nominal": np.array(INERTIA)}
    for lag in (0, 1):
        mass_c = torch.full((N,), MASS)
        mass_p = MASS + 0.2 * R(N)
        J_p = torch.tensor(INERTIA) * (0.8 + 0.4 * R(N, 3))
        # (random_drag off: reset_idx would redraw the drag in place under the window's graph; per-env drag set here)
        dd = DroneDynamics(N, mass_p, torch.diag_embed(J_p), DT, 3, random_drag=False, device="cpu")
        dd.drag_coeffs = dd.drag_coeffs * (0.5 + R(N, 3)) + 0.05 * R(N, 3)
        dd.h_force_drag_coeffs = dd.h_force_drag_coeffs * (0.5 + R(N, 3)) + 0.1 * R(N, 3)
        dd.decay_factor = GAMMA
        ctl = CTBRController(CTBRCfg(), N, "cpu", mass_c, torch.tensor(INERTIA).diag().unsqueeze(0).repeat(N, 1, 1), DT)
        ctl.rate_gain_p = ctl.rate_gain_p * (0.9 + 0.2 * R(N, 3))
        ctl.rate_gain_d = ctl.rate_gain_d * (0.9 + 0.2 * R(N, 3))
        ctl.thrust_ctrl_delay = ctl.thrust_ctrl_delay * (0.8 + 0.5 * R(N, 1))
        ctl.torque_ctrl_delay = ctl.torque_ctrl_delay * (0.8 + 0.5 * R(N, 3))
        idx = torch.arange(N)
        torch.manual_seed(17 + lag)
        dd.reset_idx(idx)

        def fresh(n):
            q = Nn(n, 4)
            q = q / q.norm(dim=1, keepdim=True)
            return torch.cat([Nn(n, 3) * 0.5 + torch.tensor([0.0, 0.0, 1.0]), q, Nn(n, 3) * 2.0, Nn(n, 3) * 2.0], 1)

        dd.reset_state(fresh(N), idx)
        ctl.gross_thrust = 3.0 + 6.0 * R(N, 1)
        ctl.torque = Nn(N, 3) * 0.01
        dd.detach()
        ctl.detach()
        thr = 1.0 + Nn(N) * 0.05
        weight = mass_c * CTBRCfg.g
        sc = torch.hstack([(weight * 3.0 / 2)[:, None], torch.ones(N, 3) * 6])
        of = torch.hstack([(weight * 3.0 / 2)[:, None], torch.zeros(N, 3)])
        a = (Nn(T, N, 4) * 1.5).requires_grad_(True)
        u_before = torch.tanh(Nn(N, 4))  # the lag buffer at the head of the window: a constant
        goals = Nn(T, N, 3) * 2.0
        alpha_b = Nn(T, N, 3) * 5.0
        rec = {k: [] for k in ("p", "q", "v", "w", "al", "T", "tau", "u", "thr", "k2", "k1", "Kp", "cT", "Kd", "mp", "ct",
                               "mc", "J", "xp", "goal", "done")}
        per_step, per_terms = [], []
        for t in range(T):
            u = torch.tanh(a[t - lag]) if t >= lag else u_before
            cmd = u * sc + of
            cmd = torch.cat([cmd[:, :1] * thr[:, None], cmd[:, 1:]], 1)
            pre = {"p": dd.pos, "q": dd.quat, "v": dd.lin_vel_w, "w": dd.ang_vel_b, "al": alpha_b[t], "T": ctl.gross_thrust,
                   "tau": ctl.torque, "u": u, "thr": thr[:, None], "k2": dd.drag_coeffs, "k1": dd.h_force_drag_coeffs,
                   "Kp": ctl.rate_gain_p, "cT": torch.exp(-DT / ctl.thrust_ctrl_delay), "Kd": ctl.rate_gain_d,
                   "mp": mass_p[:, None], "ct": torch.exp(-DT / ctl.torque_ctrl_delay), "mc": mass_c[:, None], "J": J_p}
            for k, v in pre.items():
                rec[k].append(v.detach().clone())
            z3 = torch.zeros(N, 3)
            st = {"pos": dd.pos.detach(), "quat": dd.quat.detach(), "lin_vel_w": dd.lin_vel_w.detach(),
                  "ang_vel_w": dd.ang_vel_w.detach(), "lin_vel_b": dd.lin_vel_b.detach(),
                  "ang_vel_b": dd.ang_vel_b.detach(), "lin_acc_w": z3, "ang_acc_w": z3, "lin_acc_b": z3,
                  "ang_acc_b": alpha_b[t]}
            _, tt = ctl.compute(st, cmd)
            nominal, _ = dd.step(tt)
            w_b_plus = dd.ang_vel_b.detach().clone()
            aligned = dd.align(nominal.detach(), nominal)
            env = types.SimpleNamespace(
                command_manager=types.SimpleNamespace(get_term=lambda name, t=t: types.SimpleNamespace(gate_pose_gt_w=goals[t])),
                scene=types.SimpleNamespace(env_origins=torch.zeros(N, 3)))
            terms = torch.stack([WEIGHTS[0] * losses.racing_target_diff(env, aligned, "next_gate_pose"),
                                 WEIGHTS[1] * losses.racing_vel_diff(env, aligned),
                                 WEIGHTS[2] * losses.racing_falling_diff(env, aligned)], dim=1)
            per_terms.append(terms)
            per_step.append(terms.sum(dim=1))
            rec["xp"].append(torch.cat([nominal[:, 0:10], w_b_plus], 1).detach().clone())
            rec["goal"].append(goals[t].clone())
            done = torch.zeros(N, 1)
            if t in RESETS:
                ids = torch.tensor(RESETS[t])
                done[ids] = 1.0
                dd.reset_idx(ids)
                dd.reset_state(fresh(N), ids)
                ctl.reset_idx(ids)
            rec["done"].append(done)
        stacked = torch.stack(per_step)
        total = (stacked + torch.zeros_like(stacked)).mean()  # BPTT.update: (losses + losses_detached).mean()
        total.backward()
        tag = f"lag{lag}_"
        for k, v in rec.items():
            out[tag + k] = torch.stack(v).numpy()
        out[tag + "losses"] = stacked.detach().numpy()
        out[tag + "terms"] = torch.stack(per_terms).detach().numpy()
        out[tag + "grad"] = a.grad.numpy()
        out[tag + "a"] = a.detach().numpy()
        out[tag + "total"] = float(total.detach())
    np.savez_compressed(os.path.join(HERE, "golden_bptt.npz"), **out)
    print("wrote golden_bptt.npz", {k: np.shape(v) for k, v in out.items() if k.startswith("lag1_")})


if __name__ == "__main__":
    main()
