"""Golden vectors for the recurrent PPO update, produced by the REFERENCE's own storage and algorithm code.

Run where the reference tree is available (il_shim.REF; the fixture, not the reference, is what the tests read):

    python tests/golden/make_golden_recurrent.py

Loads standalone/rsl_rl/ext/storage/rollout_storage.py (reccurent_mini_batch_generator, :193-254) and
algorithms/ppo.py (the is_recurrent branches, :72-73,106-127) from the reference tree as make_golden_ppo.py does.
rsl_rl is not installed: `rsl_rl.utils.split_and_pad_trajectories` / `unpad_trajectories` and the upstream-style
`Memory` / ActorCriticRecurrent are the restatements of rsl-rl-lib 2.2 in tests/recurrent_ref.py.  Everything runs in
float64 on the CPU.

One T = 6, N = 8 rollout, 2 mini-batches.  The dones pattern has an env with no done, one done at t = 0, one at
t = T-1, one env done twice, two consecutive dones (and an env done at both ends).  Recorded: the inputs and the
stored rollout, the reference generator's batches (padded trajectories, masks, hidden batches), the action mean and
value per [t, env] after unpad_trajectories, one PPO.update()'s losses, learning rate and resulting parameters.  Only
arrays: no program text.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import il_shim  # noqa: E402
import recurrent_ref  # noqa: E402

OUT = os.path.join(HERE, "golden_recurrent.npz")
EXT = os.path.join(il_shim.REF, "standalone/rsl_rl/ext")
T, N, OBS, R, K = 6, 8, 16, 16, 4
HEADS = [16, 16]
HP = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
          entropy_coef=0.005, learning_rate=5e-4, max_grad_norm=1.0, use_clipped_value_loss=True,
          schedule="adaptive", desired_kl=0.01)
# (t, env) of every done
DONES = [(0, 1), (T - 1, 2), (1, 3), (4, 3), (2, 4), (3, 4), (3, 6), (0, 7), (T - 1, 7)]


def load_reference():
    from generalizableracing_amd.rsl_rl import ActorCritic

    for n in ("rsl_rl", "rsl_rl.modules", "rsl_rl.utils", "standalone", "standalone.rsl_rl", "standalone.rsl_rl.ext"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["rsl_rl.modules"].ActorCritic = ActorCritic
    sys.modules["rsl_rl.utils"].split_and_pad_trajectories = recurrent_ref.split_and_pad_trajectories
    sys.modules["rsl_rl.utils"].unpad_trajectories = recurrent_ref.unpad_trajectories
    st = il_shim.synthetic_package("standalone.rsl_rl.ext.storage", os.path.join(EXT, "storage"))
    rs = il_shim.load("standalone.rsl_rl.ext.storage.rollout_storage", os.path.join(EXT, "storage/rollout_storage.py"))
    st.RolloutStorage = rs.RolloutStorage
    return il_shim.load("grref_ppo_recurrent", os.path.join(EXT, "algorithms/ppo.py")).PPO


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(T, N, OBS, generator=g, dtype=torch.float64)
    cobs = torch.randn(T, N, OBS, generator=g, dtype=torch.float64)
    rew = torch.randn(T, N, generator=g, dtype=torch.float64) * 0.1
    dones = torch.zeros(T, N, dtype=torch.long)
    for t, e in DONES:
        dones[t, e] = 1
    tout = (torch.rand(T, N, generator=g) < 0.5) & dones.bool()
    last = torch.randn(N, OBS, generator=g, dtype=torch.float64)
    return obs, cobs, rew, dones, tout, last


def flat_params(policy):
    return torch.cat([p.detach().reshape(-1) for p in policy.parameters()])


def main():
    torch.set_default_dtype(torch.float64)
    RefPPO = load_reference()
    Policy = recurrent_ref.ref_policy_class()
    torch.manual_seed(0)
    pol = Policy(OBS, OBS, K, HEADS, HEADS, "lrelu", rnn_hidden_size=R)
    rec = {"dones_pattern": torch.tensor(DONES), "param_names": None}
    names = [n for n, _ in pol.named_parameters()]
    obs, cobs, rew, dones, tout, last = inputs(11)
    for k, v in (("obs", obs), ("cobs", cobs), ("rew", rew), ("dones", dones), ("tout", tout), ("last", last)):
        rec[f"in_{k}"] = v
    rec["init_params"] = flat_params(pol)
    alg = RefPPO(pol, None, device="cpu", **HP)
    alg.init_storage("rl", N, T, [OBS], [OBS], [K])
    # a warm-up step so that the rollout starts from a non-zero state (the state a previous rollout left)
    torch.manual_seed(50)
    with torch.inference_mode():
        pol.act(torch.randn(N, OBS))
        pol.evaluate(torch.randn(N, OBS))
        torch.manual_seed(100)
        for t in range(T):
            alg.act(obs[t], cobs[t])
            alg.process_env_step(rew[t], dones[t], {"time_outs": tout[t]})
        alg.compute_returns(last)
    st = alg.storage
    for k in ("actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "returns", "advantages"):
        rec[f"st_{k}"] = getattr(st, k).clone()
    rec["st_h0_a"] = st.saved_hidden_states_a[0][0, 0].clone()  # [N, R]: the states saved at rollout step 0
    rec["st_h0_c"] = st.saved_hidden_states_c[0][0, 0].clone()
    # the reference generator's batches and the per-[t, env] outputs before the update
    mean = torch.zeros(T, N, K)
    value = torch.zeros(T, N, 1)
    size = N // HP["num_mini_batches"]
    with torch.no_grad():
        for i, b in enumerate(st.reccurent_mini_batch_generator(HP["num_mini_batches"], 1)):
            rec[f"gen{i}_obs"], rec[f"gen{i}_cobs"], rec[f"gen{i}_masks"] = b[0].clone(), b[1].clone(), b[10].clone()
            rec[f"gen{i}_hid_a"], rec[f"gen{i}_hid_c"] = b[9][0].clone(), b[9][1].clone()
            pol.act(b[0], masks=b[10], hidden_states=b[9][0])
            mean[:, i * size:(i + 1) * size] = pol.action_mean
            value[:, i * size:(i + 1) * size] = pol.evaluate(b[1], masks=b[10], hidden_states=b[9][1])
    rec["ref_mean"], rec["ref_value"] = mean, value
    torch.manual_seed(200)
    losses = alg.update()
    for k, v in losses.items():
        rec[f"loss_{k}"] = torch.tensor(float(v), dtype=torch.float64)
    rec["lr"] = torch.tensor(float(alg.learning_rate), dtype=torch.float64)
    rec["params"] = flat_params(pol)
    out = {}
    for k, v in rec.items():
        if v is None:
            continue
        a = v.detach().cpu().numpy()
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        out[k] = np.ascontiguousarray(a)
    out["param_names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB, {len(out)} arrays; lr {float(rec['lr']):.3e} losses "
          f"{ {k: float(v) for k, v in losses.items()} }")


if __name__ == "__main__":
    main()
