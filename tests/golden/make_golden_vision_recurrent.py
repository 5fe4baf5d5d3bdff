"""Golden vectors for VisionActorCriticRecurrent, produced by the REFERENCE's own module, storage and algorithm code.

Run where the reference tree is available (il_shim.REF; the fixture, not the reference, is what the tests read):

    python tests/golden/make_golden_vision_recurrent.py

Loads standalone/rsl_rl/ext/modules/vision_actor_critic.py (VisionActorCriticRecurrent, :150-278) as
make_golden_vision.py loads its sibling, with tests/recurrent_ref.py's restatements of rsl-rl-lib 2.2 (`Memory`, the
upstream ActorCriticRecurrent over this project's ActorCritic, `unpad_trajectories`) bound where the file imports
rsl_rl; and the reference's RolloutStorage (reccurent_mini_batch_generator) and PPO (the is_recurrent branches) as
make_golden_recurrent.py loads them.  Everything runs in float64 on the CPU.

Shapes: T = 6, N = 8, images 72 x 96 (the class asserts it), dim_hidden_input 16, GRU 16, heads [16, 16], 2
mini-batches.  The observation rows come from a seeded CPU generator (tests/vision_recurrent_golden.py) that the test
re-runs: the fixture stores the seed and a checksum, not the images.  Two recordings:
  (a) eval mode, the full DONES pattern: the action mean and the value per [t, env] after unpad_trajectories;
  (b) train mode, no done inside the rollout (the reference's stem then sees no padding image): the same outputs per
      mini-batch (the two forwards update the BatchNorm running statistics), then one PPO.update()'s losses, learning
      rate, resulting parameters and BatchNorm running statistics.
Only arrays: no program text.
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
import vision_recurrent_golden as vg  # noqa: E402

OUT = os.path.join(HERE, "golden_vision_recurrent.npz")
EXT = os.path.join(il_shim.REF, "standalone/rsl_rl/ext")
STORED = ("actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "returns", "advantages")


def load_reference():
    from generalizableracing_amd.rsl_rl import ActorCritic

    for n in ("rsl_rl", "rsl_rl.modules", "rsl_rl.modules.actor_critic_recurrent", "rsl_rl.utils", "standalone",
              "standalone.rsl_rl", "standalone.rsl_rl.ext"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["rsl_rl.modules"].ActorCritic = ActorCritic
    acr = sys.modules["rsl_rl.modules.actor_critic_recurrent"]
    acr.ActorCritic = ActorCritic
    acr.ActorCriticRecurrent = recurrent_ref.ref_policy_class()
    acr.Memory = recurrent_ref.Memory
    sys.modules["rsl_rl.utils"].split_and_pad_trajectories = recurrent_ref.split_and_pad_trajectories
    sys.modules["rsl_rl.utils"].unpad_trajectories = recurrent_ref.unpad_trajectories
    policy = il_shim.load("grref_vision_actor_critic_recurrent",
                          os.path.join(EXT, "modules/vision_actor_critic.py")).VisionActorCriticRecurrent
    st = il_shim.synthetic_package("standalone.rsl_rl.ext.storage", os.path.join(EXT, "storage"))
    rs = il_shim.load("standalone.rsl_rl.ext.storage.rollout_storage", os.path.join(EXT, "storage/rollout_storage.py"))
    st.RolloutStorage = rs.RolloutStorage
    return policy, il_shim.load("grref_ppo_vision_recurrent", os.path.join(EXT, "algorithms/ppo.py")).PPO


def rollout(alg, pol, seed, dones_list, sample_seed):
    obs, cobs, rew, dones, tout, last, warm = vg.inputs(seed, dones_list)
    alg.init_storage("rl", vg.N, vg.T, [vg.OBS], [vg.OBS], [vg.K])
    with torch.inference_mode():
        pol.act(warm[0])  # a warm-up step: the rollout starts from a non-zero state
        pol.evaluate(warm[1])
        torch.manual_seed(sample_seed)
        for t in range(vg.T):
            alg.act(obs[t], cobs[t])
            alg.process_env_step(rew[t], dones[t], {"time_outs": tout[t]})
        alg.compute_returns(last)
    return obs, cobs, dones


def batch_outputs(pol, st):
    mean, value = torch.zeros(vg.T, vg.N, vg.K), torch.zeros(vg.T, vg.N, 1)
    size = vg.N // vg.HP["num_mini_batches"]
    with torch.no_grad():
        for i, b in enumerate(st.reccurent_mini_batch_generator(vg.HP["num_mini_batches"], 1)):
            pol.act(b[0], masks=b[10], hidden_states=b[9][0])
            mean[:, i * size:(i + 1) * size] = pol.action_mean
            value[:, i * size:(i + 1) * size] = pol.evaluate(b[1], masks=b[10], hidden_states=b[9][1])
    return mean, value


def record(rec, tag, pol, alg, obs, cobs, dones):
    st = alg.storage
    rec[f"{tag}_checksum"] = vg.checksum(obs, cobs)
    rec[f"{tag}_dones"] = dones
    for k in STORED:
        rec[f"{tag}_st_{k}"] = getattr(st, k).clone()
    rec[f"{tag}_h0_a"] = st.saved_hidden_states_a[0][0, 0].clone()  # [N, R]: the states saved at rollout step 0
    rec[f"{tag}_h0_c"] = st.saved_hidden_states_c[0][0, 0].clone()


def state(pol, prefix, rec, buffers_only=False):
    """The state dict under `prefix`; buffers_only: the BatchNorm statistics alone (the parameters have not moved)."""
    names = {n for n, _ in pol.named_buffers()}
    for k, v in pol.state_dict().items():
        if not buffers_only or k in names:
            rec[f"{prefix}:{k}"] = v.detach().clone()


def main():
    torch.set_default_dtype(torch.float64)
    Policy, RefPPO = load_reference()
    rec = {"seeds": torch.tensor([vg.SEED_A, vg.SEED_B]), "dones_pattern": torch.tensor(vg.DONES)}
    torch.manual_seed(0)
    pol = Policy(vg.OBS, vg.OBS, vg.K, **vg.policy_kwargs())
    vg.randomise_batchnorms(pol, torch.Generator().manual_seed(5))
    state(pol, "sd0", rec)
    init = {k: v.clone() for k, v in pol.state_dict().items()}
    # ---- (a) eval mode, the full dones pattern
    alg = RefPPO(pol, None, device="cpu", **vg.HP)
    pol.eval()
    obs, cobs, dones = rollout(alg, pol, vg.SEED_A, vg.DONES, 100)
    record(rec, "a", pol, alg, obs, cobs, dones)
    rec["a_mean"], rec["a_value"] = batch_outputs(pol, alg.storage)
    # ---- (b) train mode, no done inside the rollout
    torch.manual_seed(1)
    pol = Policy(vg.OBS, vg.OBS, vg.K, **vg.policy_kwargs())
    pol.load_state_dict(init)
    alg = RefPPO(pol, None, device="cpu", **vg.HP)
    pol.train()
    obs, cobs, dones = rollout(alg, pol, vg.SEED_B, [], 101)
    record(rec, "b", pol, alg, obs, cobs, dones)
    state(pol, "sdb_rollout", rec, buffers_only=True)  # after the rollout's training-mode forwards
    rec["b_mean"], rec["b_value"] = batch_outputs(pol, alg.storage)
    state(pol, "sdb_batch", rec, buffers_only=True)  # after the two batch-mode forwards per mini-batch
    torch.manual_seed(200)
    losses = alg.update()
    for k, v in losses.items():
        rec[f"b_loss_{k}"] = torch.tensor(float(v), dtype=torch.float64)
    rec["b_lr"] = torch.tensor(float(alg.learning_rate), dtype=torch.float64)
    state(pol, "sdb_update", rec)
    out = {}
    for k, v in rec.items():
        a = v.detach().cpu().numpy()
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        out[k] = np.ascontiguousarray(a)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB, {len(out)} arrays; lr {float(rec['b_lr']):.3e} losses "
          f"{ {k: float(v) for k, v in losses.items()} }")


if __name__ == "__main__":
    main()
