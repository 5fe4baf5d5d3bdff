"""BPTT (standalone/diff_rl/algorithms/bptt.py, algo.py): one AdamW step per window on the mean differentiable loss.

The reference keeps T policy forwards and the env's torch graph alive and calls total.backward().  Here the rollout
runs under no_grad and stores obs_t and the noise eps_t; `update` takes G = d(mean loss)/d(action) [T, N, 4] from the
env (RacingEnv.loss_action_grad: one reverse-time HIP launch over the tape), recomputes a = mu(obs) + std * eps over
the T * N rows in one forward and calls a.backward(G): the same parameter gradients, because the observations carry
no gradient (tests/test_bptt_cpu.py).
"""
from __future__ import annotations

import torch
from torch.optim import SGD, Adam, Adamax, AdamW, RMSprop  # noqa: F401
from torch.optim.lr_scheduler import CosineAnnealingLR, ExponentialLR, StepLR  # noqa: F401

from ..rsl_rl import linear
from .model import BaseModel

_OPTIMIZERS = {"Adam": Adam, "AdamW": AdamW, "SGD": SGD, "Adamax": Adamax, "RMSprop": RMSprop}
_SCHEDULES = {"CosineAnnealingLR": CosineAnnealingLR}


class BPTT:
    def __init__(self, actor_critic: BaseModel, max_iterations=1000, learning_rate=1e-3, schedule="CosineAnnealingLR",
                 device="cpu", optimizer="Adam", **kwargs):
        if kwargs:
            print(f"{self.__class__}.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        if optimizer not in _OPTIMIZERS:
            raise ValueError(f"unknown optimizer {optimizer!r}; one of {sorted(_OPTIMIZERS)}")
        if schedule not in _SCHEDULES:
            raise ValueError(f"unknown schedule {schedule!r}; one of {sorted(_SCHEDULES)}")
        self.device = device
        self.learning_rate = learning_rate
        self.actor_critic = actor_critic.to(device)
        self.optimizer = _OPTIMIZERS[optimizer](self.actor_critic.parameters(), lr=learning_rate)
        self.schedule = _SCHEDULES[schedule](self.optimizer, max_iterations, learning_rate * 0.01)
        self.env = None  # set by the runner: the env whose loss_action_grad() closes the window
        self.obs, self.eps, self.losses, self.losses_detached = [], [], [], []

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def act(self, obs, critic_obs=None):
        with torch.no_grad():
            a, eps = self.actor_critic.act_with_noise(obs)
        self.obs.append(obs.clone())  # (the env's observation tensors alternate between two sets)
        self.eps.append(eps)
        return a

    def process_env_step(self, losses, losses_detached, dones, rewards=None, infos=None):
        self.losses.append(losses)
        self.losses_detached.append(losses_detached)
        self.actor_critic.reset(dones)

    def policy_actions(self, obs: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
        """a = mu(obs) + std * eps over [rows, obs] in one forward (the fused MLP where linear.networks_fusable)."""
        ac = self.actor_critic
        if linear.networks_fusable([ac.actor], [obs]):
            mean = linear.fused_mlps([ac.actor], [obs])[0]
        else:
            mean = ac.actor(obs)
        return mean + ac.noise_std().expand_as(mean) * eps

    def update(self, grad_actions: torch.Tensor | None = None):
        """One optimiser step on mean(losses + losses_detached) over the window.  grad_actions: d(mean)/d(action)
        [T, N, 4] (default: the env's loss_action_grad())."""
        T = len(self.obs)
        G = self.env.loss_action_grad() if grad_actions is None else grad_actions
        total = (torch.stack(self.losses) + torch.stack(self.losses_detached)).mean()
        obs = torch.stack(self.obs).flatten(0, 1)
        eps = torch.stack(self.eps).flatten(0, 1)
        self.optimizer.zero_grad()
        a = self.policy_actions(obs, eps)
        a.backward(G[:T].reshape(a.shape).to(a.dtype))
        self.optimizer.step()
        self.schedule.step()
        self.learning_rate = self.optimizer.param_groups[0]["lr"]
        self.obs, self.eps, self.losses, self.losses_detached = [], [], [], []
        return 0.0, total  # (0.0: the runner's value-loss slot)
