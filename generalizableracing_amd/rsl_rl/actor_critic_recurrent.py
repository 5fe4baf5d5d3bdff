"""ActorCriticRecurrent — the rsl_rl policy with a GRU memory in front of the actor and of the critic
(rsl_rl.modules.ActorCriticRecurrent; the reference's config for it: agents/rsl_rl_ppo_cfg.py:64-76, its
`is_recurrent` branches: standalone/rsl_rl/ext/algorithms/ppo.py:72-73,106-127).  rsl_rl is not vendored in the
reference: this restates rsl-rl-lib 2.2's class, so it is parity unpinned like ActorCritic.  The default `rnn_type`
is "gru" where upstream's is "lstm": only the one-layer GRU is built here.

Batch mode differs from upstream in form, not in value.  Upstream splits the rollout at every done, pads the
trajectories and starts each from a saved hidden state (rollout_storage.py:193-254).  Every such state is either the
state at rollout step 0 or zero (`reset(dones)` zeroes finished envs, and the state is saved before `act`), so the
same values come from running the memory over the whole [T, B] block with the carried state multiplied by
1 - dones[t-1] before step t, from the state the envs held at step 0.  `masks` in batch mode is therefore the
rollout's `dones` of the same block, not a padding mask, and nothing is unpadded: fixed shapes, no host read, one
launch per direction (fused_gru.py; csrc/gr_gru.hip), h0 [N, R] per memory in the storage.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.distributions import Normal

from . import fused_gru
from .actor_critic import ActorCritic


class Memory(nn.Module):
    """One GRU layer with upstream's parameter names (`rnn.weight_ih_l0`, `weight_hh_l0`, `bias_ih_l0`, `bias_hh_l0`,
    gate order r, z, n) and the carried rollout state `hidden_states` [1, N, R] (zeros on first use).

    The eager path (CPU, other sizes, fused=False) is the definition: a loop over T calling `self.rnn` on one step
    with the masked state.  The fused path (fp32 CUDA tensors, fused_gru.gru_fusable, no autocast) is gr_gru_step per
    rollout step and the gr_gru_seq_* op per mini-batch."""

    def __init__(self, input_size, hidden_size=256, fused=True):
        super().__init__()
        self.rnn = nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=1)
        self.hidden_states = None
        self.fused = bool(fused)
        self.h0_sink = None  # [N, R]: the next fused rollout step copies its pre-step state here (stage_h0), once

    def _fusable(self, x, steps=1) -> bool:
        return self.fused and fused_gru.gru_fusable(self.rnn, x, steps)

    def _fused_step(self, x) -> bool:
        """The rollout step on x goes through gr_gru_step: it records no graph, so only with grad mode off (a caller
        that differentiates act() in rollout mode gets torch's GRU and its gradient)."""
        return not torch.is_grad_enabled() and self._fusable(x)

    def _state(self, x):
        """The carried state, zeros on first use.  Never an inference tensor, though the rollout runs in inference
        mode: reset() may be called outside it."""
        if self.hidden_states is None:
            with torch.inference_mode(False):
                self.hidden_states = torch.zeros(1, x.shape[0], self.rnn.hidden_size, device=x.device,
                                                 dtype=self.rnn.weight_hh_l0.dtype)
        return self.hidden_states

    def stage_h0(self, x, sink):
        """Before the rollout step on x at rollout step 0 (ppo.py:72-73): the state for the transition to carry to
        the storage, which copies it into `sink` (its h0) after the step; torch's step leaves that tensor intact.
        gr_gru_step updates the state in place, so on the fused path the step itself copies the pre-step state into
        `sink` (its second pointer) and the transition carries None."""
        if self._fused_step(x):
            self.h0_sink = sink
            return None
        return self._state(x)

    def forward(self, x, masks=None, hidden_states=None):
        if masks is not None:  # batch mode: x [T, B, D], masks = dones [T, B], hidden_states = h0 [1, B, R]
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            return self.sequence(x, masks, hidden_states)
        # rollout mode: x [N, D]
        state = self._state(x)
        if self._fused_step(x):
            sink, self.h0_sink = self.h0_sink, None
            fused_gru.gru_step(self.rnn, x, state[0], h_prev_out=sink)
            return state[0]
        out, h = self.rnn(x.unsqueeze(0), state)
        h = h.detach()  # (the rollout carries no graph from step to step)
        if torch.is_inference_mode_enabled():
            with torch.inference_mode(False):
                h = h.clone()
        self.hidden_states = h
        return out[0]

    def sequence(self, x, dones, h0):
        """The masked sequence: out [T * B, R], time-major."""
        T, B = x.shape[0], x.shape[1]
        r = self.rnn.hidden_size
        if self._fusable(x, T):
            return fused_gru.gru_sequence(self.rnn, x, h0, dones).reshape(T * B, r)
        keep = (dones.reshape(T, B) == 0).to(x.dtype)
        h = h0.reshape(1, B, r)
        outs = []
        for t in range(T):
            if t > 0:
                h = h * keep[t - 1].view(1, B, 1)
            o, h = self.rnn(x[t:t + 1], h)
            outs.append(o[0])
        return torch.stack(outs).reshape(T * B, r)

    def reset(self, dones=None):
        """Zero the state of finished envs (all of them for dones None).  A masked fill on the device: no host read.
        gr_gru_step takes no dones: the reset stays this separate masked zero."""
        if self.hidden_states is None:
            return
        if dones is None:
            self.hidden_states.zero_()
            return
        self.hidden_states.masked_fill_((dones.reshape(1, -1, 1) != 0).to(self.hidden_states.device), 0.0)


class RecurrentHeads:
    """What a policy with a memory in front of the actor and of the critic adds to its feed-forward base, shared by
    ActorCriticRecurrent and VisionActorCriticRecurrent (mixed in ahead of the base).  `encode` maps observations
    to the memories' inputs: the observations themselves here, the vision feature there."""
    is_recurrent = True

    def init_memories(self, input_a, input_c, hidden_size, fused):
        self.memory_a = Memory(input_a, hidden_size=hidden_size, fused=fused)
        self.memory_c = Memory(input_c, hidden_size=hidden_size, fused=fused)

    @staticmethod
    def check_rnn(name, rnn_type, rnn_num_layers):
        if str(rnn_type).lower() != "gru" or int(rnn_num_layers) != 1:
            raise NotImplementedError(f"{name}: rnn_type={rnn_type!r} with {rnn_num_layers} layer(s) is "
                                      "not built; supported: rnn_type='gru' with rnn_num_layers=1")

    @property
    def fused_gru(self) -> bool:
        return self.memory_a.fused

    @fused_gru.setter
    def fused_gru(self, on):
        self.memory_a.fused = self.memory_c.fused = bool(on)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def stage_hidden_states(self, observations, critic_observations, h0_a, h0_c):
        """(h_a, h_c) for the transition at rollout step 0, before acting on these observations; None for a memory
        whose fused step writes h0_a / h0_c itself (Memory.stage_h0)."""
        return (self.memory_a.stage_h0(observations, h0_a), self.memory_c.stage_h0(critic_observations, h0_c))

    def get_hidden_sizes(self):
        return self.memory_a.rnn.hidden_size, self.memory_c.rnn.hidden_size

    def encode(self, observations):
        """The memory's input for these observations ([N, .] in rollout mode, [T, B, .] in batch mode)."""
        return observations

    def memory_inputs(self, observations, critic_observations):
        """(memory_a's, memory_c's) inputs for a mini-batch's [T, B, .] observation blocks (PPO._recurrent_loss)."""
        return self.encode(observations), self.encode(critic_observations)

    def set_distribution(self, mean, draw=False):
        """The action distribution from the actor's output on the memory's rows; draw: sample once, as `act` does."""
        self.distribution = Normal(mean, self._std(mean))
        return self._sample() if draw else None

    def update_distribution(self, observations, masks=None, hidden_states=None):
        self.set_distribution(self.actor(self.memory_a(self.encode(observations), masks, hidden_states)))

    def act(self, observations, masks=None, hidden_states=None):
        self.update_distribution(observations, masks, hidden_states)
        return self._sample()

    def _sample(self):
        d = self.distribution
        if d.loc.is_cuda:  # (as ActorCritic.act: Normal.sample's bits without its host read)
            with torch.no_grad():
                return torch.randn(d.loc.shape, dtype=d.loc.dtype, device=d.loc.device).mul_(d.scale).add_(d.loc)
        return d.sample()

    def act_inference(self, observations):
        return self.actor(self.memory_a(self.encode(observations)))

    def evaluate(self, critic_observations, masks=None, hidden_states=None):
        return self.critic(self.memory_c(self.encode(critic_observations), masks, hidden_states))


class ActorCriticRecurrent(RecurrentHeads, ActorCritic):
    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", rnn_type="gru", rnn_hidden_size=256,
                 rnn_num_layers=1, init_noise_std=1.0, noise_std_type: str = "scalar", fused_gru=True, **kwargs):
        self.check_rnn("ActorCriticRecurrent", rnn_type, rnn_num_layers)
        super().__init__(rnn_hidden_size, rnn_hidden_size, num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std,
                         noise_std_type=noise_std_type, **kwargs)
        self.init_memories(num_actor_obs, num_critic_obs, rnn_hidden_size, fused_gru)
