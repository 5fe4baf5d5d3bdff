"""PPOL2C2 — PPO with the L2C2 smoothness regulariser
(standalone/rsl_rl/ext/algorithms/ppo_l2c2.py:8-212), the algorithm the vision racing
recipe registers (quadcopter_diff/agents/rsl_rl_ppo_cfg.py:87-101, class_name="PPOL2C2").

Same act / process_env_step / compute_returns / PPO losses as PPO, plus, per
minibatch (ppo_l2c2.py:176-190):
    eps   = lb / (ub - lb);   c_pi = ub * eps;   c_v = value_smoothness_coef * c_pi
    w     = cont * U(-1, 1)                           (one scalar per sample; 0 across a reset)
    o_mix = o + w * (o_next - o)
    L_s   = c_pi * mean(|mu(o) - mu(o_mix)|^2) + c_v * mean(|V(o) - V(o_mix)|^2)
added to the PPO loss.  Multi-GPU as in PPO: KL mean averaged across ranks
before the learning-rate decision, gradients averaged in one flat all-reduce.

Deviations (documented):
  * `act_inference` of the reference's VisionActorCritic returns (mean, feat) and
    ppo_l2c2.py:184,189 take `[0]`; on a plain ActorCritic `[0]` would pick the first
    ROW of the mean and broadcast it.  Here `_mean_of` takes [0] only of a tuple.
  * the transition is stored unless the whole observation batch is ~0
    (ppo_l2c2.py:98), as in the reference; that test costs one host sync per step.  With the
    observation sink (the camera kernel writes the rows into the storage slot) the test runs in act(),
    on the same rows, and a skipped transition's successor rows move down into its slot
    (RolloutStorage.sink_skipped).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _abi
from . import fused_loss as _floss
from .ppo import PPO, _GraphedStep
from .rollout_storage_l2c2 import RolloutStorageL2C2


def _mean_of(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def _mix(obs, next_obs, w):
    """obs + w * (next_obs - obs) (ppo_l2c2.py:179-180), w [rows, 1]: on the GPU one pass of gr_l2c2_mix (the same
    three fp32 roundings as the torch expression), else the expression."""
    fused = (obs.is_cuda and obs.dim() == 2 and obs.dtype == torch.float32 and next_obs.dtype == torch.float32
             and obs.shape == next_obs.shape and obs.shape[1] % 4 == 0 and w.numel() == obs.shape[0]
             and obs.is_contiguous() and next_obs.is_contiguous()
             and not (obs.requires_grad or next_obs.requires_grad or w.requires_grad))
    if fused:
        w = w.reshape(-1).float().contiguous()
        out = torch.empty_like(obs)
        _abi.call("gr_l2c2_mix", obs.data_ptr(), next_obs.data_ptr(), w.data_ptr(), obs.shape[0], obs.shape[1],
                  out.data_ptr(), _abi.raw_stream(obs.device))
        return out
    return obs + w * (next_obs - obs)


def _mix_rows(src, rows_obs, rows_next, w):
    """_mix(src[rows_obs], src[rows_next], w) in one pass over the storage rows (gr_l2c2_mix_rows): no gathered copies
    of the pair."""
    w = w.reshape(-1).float().contiguous()
    out = torch.empty(rows_obs.numel(), src.shape[1], device=src.device, dtype=torch.float32)
    _abi.call("gr_l2c2_mix_rows", src.data_ptr(), src.data_ptr(), src.stride(0), rows_obs.data_ptr(),
              rows_next.data_ptr(), w.data_ptr(), out.shape[0], out.shape[1], out.data_ptr(),
              _abi.raw_stream(src.device))
    return out


class PPOL2C2(PPO):
    storage_cls = RolloutStorageL2C2
    loss_terms = PPO.loss_terms + ("smooth_loss",)

    def __init__(self, policy, env=None, value_smoothness_coef=0.1, smoothness_upper_bound=1.0,
                 smoothness_lower_bound=0.1, share_mix_features=True, rows_update=True, **kwargs):
        kwargs.pop("normalize_advantage", None)
        # one stem evaluation of the mixed batch for the actor and the critic (policies with shared_features)
        self.share_mix_features = bool(share_mix_features)
        # the graphed update reads the mini-batch's image rows through its permutation (no gathered copies)
        self.rows_update = bool(rows_update)
        super().__init__(policy, env=env, normalize_advantage=True, **kwargs)
        self._mix_uniform = torch.rand_like  # the smoothness loss's uniform draw (tests substitute a fixed one)
        self.value_smoothness_coef = value_smoothness_coef
        self.smoothness_upper_bound = smoothness_upper_bound
        self.smoothness_lower_bound = smoothness_lower_bound

    def smooth_coefs(self):
        """ppo_l2c2.py:176-178."""
        eps = self.smoothness_lower_bound / (self.smoothness_upper_bound - self.smoothness_lower_bound)
        policy_coef = self.smoothness_upper_bound * eps
        return policy_coef, self.value_smoothness_coef * policy_coef

    def _store_test(self, obs):
        """ppo_l2c2.py:98's zero-observation test on these rows, issued before the policy forward and the env step
        (stream order: the step cannot have touched them yet).  On the GPU its result is copied to pinned host
        memory behind an event and read in process_env_step: the host never waits for the policy forward or the env
        step, only for this reduction, long finished by then (the same decision, no per-step drain of the queue)."""
        flag = torch.norm(obs).mean() > 1e-4
        if not flag.is_cuda:
            self._store_flag = bool(flag)
            return
        if getattr(self, "_flag_host", None) is None:
            with torch.inference_mode(False):
                self._flag_host = torch.zeros((), dtype=torch.bool, pin_memory=True)
            self._flag_event = torch.cuda.Event()
        self._flag_host.copy_(flag, non_blocking=True)
        self._flag_event.record()
        self._store_flag = None

    def _stored(self) -> bool:
        if not hasattr(self, "_store_flag"):  # (a transition stored without act: test its rows now)
            self._store_test(self.transition.observations)
        if self._store_flag is None:
            self._flag_event.synchronize()
            self._store_flag = bool(self._flag_host)
        return self._store_flag

    def act(self, obs, critic_obs):
        # (with the observation sink the rows of a skipped transition are moved down a slot and the env's next step
        # writes the slot `obs` views: the test is on these rows as they are now)
        self._store_test(obs)
        return super().act(obs, critic_obs)

    def process_env_step(self, rewards, dones, infos):
        self._stage_rewards(rewards, dones, infos)  # ppo_l2c2.py:91-95
        sink = getattr(self.storage, "sink", False)
        store = self._stored()  # ppo_l2c2.py:98
        del self._store_flag
        if store:
            self.storage.add_transitions(self.transition)
        elif sink:
            self.storage.sink_skipped()
        self.transition.clear()
        self.policy.reset(dones)

    def smooth_loss(self, obs_batch, next_obs_batch, cont_batch, mu_batch, value_batch, rows=None,
                    want_smoothness=True):
        """ppo_l2c2.py:176-188; returns (smooth_loss, action_smoothness).  rows (src, idx, next_idx): the pair is
        src[idx], src[next_idx] (the rollout storage's rows, read through the indices; obs_batch / next_obs_batch
        unused).  want_smoothness False (the update, which never reads it, ppo_l2c2.py:188-191): action_smoothness is
        None and the successor forward runs only for its side effects, the BatchNorm statistics of a training-mode
        forward (policies with record_batch_statistics; none for the others)."""
        policy_coef, value_coef = self.smooth_coefs()
        mix_weights = cont_batch * (self._mix_uniform(cont_batch) - 0.5) * 2.0
        if rows is not None:
            mix_obs_batch = _mix_rows(rows[0], rows[1], rows[2], mix_weights)
        else:
            mix_obs_batch = _mix(obs_batch, next_obs_batch, mix_weights)
        shared = getattr(self.policy, "shared_features", None)
        if shared is not None and self.share_mix_features:
            # the actor's and the critic's forward of the mixed batch share one stem evaluation (VisionActorCritic:
            # the same features, BatchNorm running statistics updated as by the reference's two forwards)
            feat = shared(mix_obs_batch, 2)
            mix_mean, mix_value = self.policy.actor(feat), self.policy.critic(feat)
        else:
            mix_mean = _mean_of(self.policy.act_inference(mix_obs_batch))
            mix_value = self.policy.evaluate(mix_obs_batch)
        policy_smooth = torch.square(torch.norm(mu_batch - mix_mean, dim=-1)).mean()
        value_smooth = torch.square(torch.norm(value_batch - mix_value, dim=-1)).mean()
        loss = policy_coef * policy_smooth + value_coef * value_smooth
        with torch.inference_mode():
            if not want_smoothness:
                record = getattr(self.policy, "record_batch_statistics", None)
                if record is not None:
                    record(*((rows[0], rows[2]) if rows is not None else (next_obs_batch,)))
                return loss, None
            if rows is not None:
                next_mean = self.policy.actor(self.policy.features_rows(rows[0], rows[2]))
            else:
                next_mean = _mean_of(self.policy.act_inference(next_obs_batch))
            action_smoothness = torch.norm(mu_batch - next_mean, dim=-1).mean()
        return loss, action_smoothness

    def _use_fused_losses(self, obs) -> bool:
        """The graphed step's PPO losses as one device op each way (fused_loss.combined_loss): a policy with actor /
        critic heads and a state-independent std over <= 8 actions, fp32 outside autocast."""
        pol = self.policy
        return (self.fused_losses and obs.is_cuda and obs.dtype == torch.float32 and hasattr(pol, "features")
                and isinstance(pol.actor, nn.Sequential) and pol.actor[-1].out_features <= 8
                and getattr(pol, "noise_std_type", None) in ("scalar", "log")
                and not torch.is_autocast_enabled("cuda"))

    def _minibatch_loss(self, batch, acc=None, kl_out=None, seed=None):
        """PPO._minibatch_loss plus the smoothness loss (ppo_l2c2.py:127-191).  The eager loop takes the torch ops,
        without autocast.  The graphed step may hand obs, critic obs and next obs each as a (storage rows, indices)
        pair, read through the indices (_GraphedStepL2C2._gather).  seed is unused: the loss is never the root."""
        obs, crit, nxt, cont = batch[:4]
        pol = self.policy
        rows = (obs[0], obs[1], nxt[1]) if isinstance(obs, tuple) else None
        if rows is not None or (acc is not None and self._use_fused_losses(obs)):
            # the log prob, KL, surrogate and value losses in one launch each way, into the sinks
            feat = (lambda x: pol.features_rows(*x)) if rows is not None else pol.features
            mu_b, value_b = pol.actor(feat(obs)), pol.critic(feat(crit))
            loss, _ = _floss.combined_loss(self, mu_b, value_b, *batch[4:11], acc=acc[:2], kl_out=kl_out)
            smooth_loss, _ = self.smooth_loss(obs, nxt, cont, mu_b, value_b, rows=rows, want_smoothness=False)
            acc[2:].add_(smooth_loss.detach())
            return loss + smooth_loss, (), None
        loss, terms, kl, mu_b, value_b = self._torch_ppo_loss(obs, crit, *batch[4:11], kl_out, draw=acc is None)
        smooth_loss, _ = self.smooth_loss(obs, nxt, cont, mu_b, value_b, want_smoothness=False)
        return loss + smooth_loss, terms + (smooth_loss.detach(),), kl


class _GraphedStepL2C2(_GraphedStep):
    """PPOL2C2.update's mini-batch step as hipGraph replays (ppo.py _GraphedStep: one graph per epoch on one rank,
    two segments around the eager all-reduce on several): the vision recipe's update is ~590 launches per
    mini-batch, most of them small, and the eager loop reads the KL back to the host once per mini-batch.

    Segment A is ppo_l2c2.py:127-191 on the mini-batch gathered by a static index buffer from the (T-1) N samples
    (rollout_storage_l2c2.py:131-167; the continuation flags in a persistent buffer refreshed per update): the
    distribution and values, the KL mean into the flat buffer's extra slot, the PPO losses, the smoothness loss
    (its own uniform draw per replay: torch's graph-safe generator), and the backward into the flat gradient
    views.  Segment B is the base class's: the rate rule on the device, the clip and Adam.  As in _GraphedStep the
    learning rate is an fp32 device tensor and the eager loop's unused action draw is not made; the BatchNorm
    running statistics of the warm-up and captured steps are restored after the capture."""

    _PACK = False  # (the pairs are gathered field by field, _gather: no packed copy of the samples)

    def __init__(self, alg: "PPOL2C2"):
        super().__init__(alg)
        st, dev = alg.storage, alg.device
        if self.T < 2:
            raise ValueError("L2C2 needs at least 2 transitions per env (pairs obs[t] with obs[t+1])")
        self.mb = (self.T - 1) * self.N // self.nmb
        self.perm = torch.zeros(self.nmb * self.mb, dtype=torch.long, device=dev)
        self.idx = self.perm[:self.mb]
        self.cont = torch.zeros((self.T - 1) * self.N, 1, device=dev)

    def _refresh_sources(self):
        st = self.alg.storage
        with torch.no_grad():
            torch.sub(1.0, st.dones[:self.T - 1].float().flatten(0, 1), out=self.cont)

    def _sources(self):
        st, T = self.alg.storage, self.T
        obs = st.observations[:T - 1].flatten(0, 1)
        crit = st.privileged_observations[:T - 1].flatten(0, 1) if st.privileged_observations is not None else obs
        return (obs, crit, st.observations[1:T].flatten(0, 1), self.cont) + tuple(
            x[:T - 1].flatten(0, 1) for x in (st.actions, st.values, st.advantages, st.returns, st.actions_log_prob,
                                               st.mu, st.sigma))

    def _gather(self, idx):
        """The generator's fields by a static index buffer; the three image fields as (storage rows, indices) pairs
        instead when the rows can be read through the permutation (_rows_ok: the same values, no gathered copies)."""
        srcs = self._sources()
        if not self._rows_ok():
            g = tuple(x.index_select(0, idx) for x in srcs)
            return tuple(x.float() for x in g[:3]) + g[3:]
        st = self.alg.storage
        src = st.observations.flatten(0, 1)  # row j + N is the successor of row j
        csrc = st.privileged_observations.flatten(0, 1) if st.privileged_observations is not None else src
        nidx = idx + self.N
        return ((src, idx), (csrc, idx), (src, nidx)) + tuple(x.index_select(0, idx) for x in srcs[3:])

    def _rows_ok(self) -> bool:
        """The mini-batch's image rows read through the permutation (VisionActorCritic.features_rows, the fused
        first block's row indices, gr_l2c2_mix_rows) instead of gathered: fp32 storage rows, a policy with
        features_rows, the fused losses."""
        st, pol = self.alg.storage, self.alg.policy
        srcs = [st.observations] + ([st.privileged_observations] if st.privileged_observations is not None else [])
        return (self.alg.rows_update and hasattr(pol, "features_rows") and st.observations.is_cuda
                and all(x.dtype == torch.float32 and x.is_contiguous() for x in srcs)
                and st.observations.shape[-1] % 4 == 0 and self.alg._use_fused_losses(st.observations[0]))


PPOL2C2.graphed_step_cls = _GraphedStepL2C2
