"""VisionActorCriticRecurrent — the vision policy with a GRU memory in front of the actor and of the critic
(standalone/rsl_rl/ext/modules/vision_actor_critic.py:150-278; its config: agents/rsl_rl_ppo_cfg.py:64-76).

feature = act(stem(depth image) + state_enc(state)), VisionActorCritic's, feeds memory_a -> actor and memory_c ->
critic.  The feature path is VisionActorCritic's code (features, features_rows, the fused stem switches) and the
memories are actor_critic_recurrent.Memory through RecurrentHeads: nothing is restated here.  State-dict keys are the
reference's: stem.*, state_enc.*, memory_a.rnn.*, memory_c.rnn.*, actor.*, critic.*, std / log_std.

Rollout mode (observations [N, .]) steps the memories' carried state; batch mode follows the project's masked-sequence
convention (actor_critic_recurrent.py): observations [T, B, .], masks = the block's dones, hidden_states = h0.  The
features train through the memories: fused_gru's wide family returns dL/dx (gr_gru_wide_seq_backward).

One deviation from the reference.  In batch mode the reference runs the stem over the PADDED trajectories
(vision_actor_critic.py:236-244), so in training mode its BatchNorm batch statistics include the all-zero padding
images whenever an env finished inside the rollout.  Here the statistics are over the T * B real rows only.  With no
done inside the rollout, or in eval mode, the two agree exactly; the padding is not reproduced.
"""
from __future__ import annotations

import torch

from .actor_critic_recurrent import RecurrentHeads
from .vision_actor_critic import VisionActorCritic


class VisionActorCriticRecurrent(RecurrentHeads, VisionActorCritic):
    def __init__(self, num_actor_obs: int, num_critic_obs: int, num_actions: int, img_res=(72, 96),
                 dim_hidden_input: int = 192, actor_hidden_dims=(256, 256, 256), critic_hidden_dims=(256, 256, 256),
                 activation="elu", rnn_type="gru", rnn_hidden_size=256, rnn_num_layers=1, init_noise_std=1.0,
                 noise_std_type: str = "scalar", fused_gru=True, **kwargs):
        self.check_rnn("VisionActorCriticRecurrent", rnn_type, rnn_num_layers)
        kwargs.pop("use_auxiliary_loss", None)  # (the reference's recurrent class has no auxiliary decoder)
        super().__init__(num_actor_obs, num_critic_obs, num_actions, img_res=img_res,
                         dim_hidden_input=dim_hidden_input, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std,
                         noise_std_type=noise_std_type, head_input_dim=rnn_hidden_size, **kwargs)
        self.init_memories(dim_hidden_input, dim_hidden_input, rnn_hidden_size, fused_gru)
        self._rows = None  # (key, row indices) of the last storage block (_block_rows)

    def _block_rows(self, obs: torch.Tensor):
        """A [T, B, D] block of a [T, N, D] rollout buffer as (flat [rows, D] view of the buffer from the block's first
        row, the block's row indices t N + b in time-major order), so that features_rows reads the images in place: a
        gathered [T * B, 6928] copy is 680 MB at the recipe's mini-batch.  (obs.reshape(T * B, D), None) when the
        block is contiguous or not such a view."""
        T, B, D = obs.shape
        if obs.is_contiguous() or obs.requires_grad or obs.stride(2) != 1 or obs.stride(1) != D \
                or (T > 1 and (obs.stride(0) % D != 0 or obs.stride(0) < B * D)):
            return obs.reshape(T * B, D), None
        N = obs.stride(0) // D if T > 1 else B
        key = (T, B, N, obs.device)
        if self._rows is None or self._rows[0] != key:
            with torch.inference_mode(False):
                t = torch.arange(T, device=obs.device).view(T, 1) * N
                self._rows = (key, (t + torch.arange(B, device=obs.device).view(1, B)).reshape(-1))
        flat = obs.as_strided(((T - 1) * N + B, D), (D, 1), obs.storage_offset())
        return flat, self._rows[1]

    def encode(self, observations):
        """The memories' input: the feature of [N, .] rows, or of a [T, B, .] block as [T, B, dim_hidden_input] (one
        stem evaluation over the T * B rows)."""
        if observations.dim() == 2:
            return self.features(observations)
        if observations.dim() != 3:
            raise ValueError("Invalid input shape")
        T, B = observations.shape[:2]
        flat, rows = self._block_rows(observations)
        feat = self.features(flat) if rows is None else self.features_rows(flat, rows)
        return feat.view(T, B, -1)

    def memory_inputs(self, observations, critic_observations):
        """The reference evaluates the stem on the actor's observations, then on the critic's (`act`, then `evaluate`:
        ppo.py:123-127).  Where the two blocks are the same memory (the storage keeps one buffer when the critic has
        no observations of its own) one evaluation stands for both, as shared_features: the same values, the summed
        feature gradient through one stem backward, every BatchNorm's running statistics updated twice."""
        o, c = observations, critic_observations
        if o.data_ptr() == c.data_ptr() and o.shape == c.shape and o.stride() == c.stride() and o.dtype == c.dtype:
            self._bn_uses = 2
            try:
                feat = self.encode(o)
            finally:
                self._bn_uses = 1
            return feat, feat
        return self.encode(o), self.encode(c)
