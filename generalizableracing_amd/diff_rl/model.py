"""BaseModel (standalone/diff_rl/algorithms/model.py:63-99): the rsl_rl ActorCritic whose `act` is a reparametrised
sample, so the action carries the policy's gradient."""
from __future__ import annotations

import torch

from ..rsl_rl.actor_critic import ActorCritic


class BaseModel(ActorCritic):
    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", init_noise_std=1.0,
                 noise_std_type: str = "scalar", **kwargs):
        super().__init__(num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std,
                         noise_std_type=noise_std_type, **kwargs)

    def noise_std(self) -> torch.Tensor:
        """The policy's std [num_actions] (with its gradient)."""
        return self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std)

    def act(self, observations, **kwargs):
        self.update_distribution(observations)
        return self.distribution.rsample()

    def act_with_noise(self, observations):
        """rsample() with the noise returned: a = mu + std * eps, eps ~ N(0, 1) -> (a, eps)."""
        mean = self.actor(observations)
        eps = torch.randn_like(mean)
        return mean + self.noise_std().expand_as(mean) * eps, eps
