"""PPOLCP — PPO with the Lipschitz-constrained-policy gradient penalty
(standalone/rsl_rl/ext/algorithms/ppo_lcp.py:13-210; the knob the racing recipe leaves commented out,
quadcopter_diff/agents/rsl_rl_ppo_cfg.py:102, grad_penalty_coef_schedule = [0.1, 0.1, 700, 1000]).

Same act / process_env_step / compute_returns / PPO losses as PPO, plus, per mini-batch (ppo_lcp.py:105-108,134-137):
    P     = mean_rows | d sum(log pi(a | x)) / dx |^2            (the actor's input gradient of the log prob)
    stage = min(max(counter - s[2], 0) / s[3], 1);   coef = s[0] + stage * (s[1] - s[0])      (s = the schedule)
    loss  = surrogate + value_loss_coef * value - entropy_coef * entropy + coef * P
`counter` starts at 0 and counts update() calls; as in the reference it is not part of a checkpoint, so a resumed
run restarts the schedule.  Multi-GPU, FlatAdam, the observation sink and the fused rollout inference as in PPO.

Two paths for P:
  * fused: on the update's tall fp32 CUDA mini-batches of a LeakyReLU ActorCritic that the whole-network MLP kernels
    cover (linear.networks_fusable), P and its gradient are two more first-order passes over the actor
    (fused_lcp.py, gr_lcp_forward / gr_lcp_backward); the observations need no gradient;
  * torch: everywhere else (CPU, ELU, short batches) the reference's idiom, `obs.clone().requires_grad_()` and
    `autograd.grad(..., create_graph=True)`, with the actor evaluated layer by layer through F.linear and its
    activation modules: never through linear.MLP's fused ops, whose backward records nothing for a second
    differentiation (the penalty would silently lose its dependence on the parameters).
Rejected: policies other than the MLP ActorCritic (the vision stem's fused ops have no double backward) and
update_autocast_bf16.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Normal

from . import fused_lcp as _flcp
from . import fused_loss as _floss
from . import linear as _lin
from .actor_critic import ActorCritic
from .ppo import PPO, _GraphedStep
from .vision_actor_critic import VisionActorCritic


def penalty_coef(schedule, counter: int) -> float:
    """ppo_lcp.py:136-137: the coefficient moves linearly from schedule[0] to schedule[1] over schedule[3] updates,
    starting at update schedule[2]."""
    stage = min(max((counter - schedule[2]), 0) / schedule[3], 1)
    return stage * (schedule[1] - schedule[0]) + schedule[0]


def actor_plain(actor: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The actor on x module by module, every Linear as F.linear: plain differentiable torch ops on every device and
    batch size, so its input gradient can be differentiated again."""
    for m in actor:
        x = F.linear(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
    return x


class PPOLCP(PPO):
    loss_terms = PPO.loss_terms + ("grad_penalty",)

    def __init__(self, policy, env=None, grad_penalty_coef_schedule=None, **kwargs):
        # (required, and asserted, as in ppo_lcp.py:59)
        assert grad_penalty_coef_schedule is not None, "PPOLCP: grad_penalty_coef_schedule is required"
        if not isinstance(policy, ActorCritic) or isinstance(policy, VisionActorCritic):
            raise TypeError(f"PPOLCP needs the MLP ActorCritic (got {type(policy).__name__}): the penalty differentiates "
                            "the actor's input gradient, and the vision stem's fused ops have no double backward")
        if kwargs.get("update_autocast_bf16"):
            raise ValueError("PPOLCP does not support update_autocast_bf16: the gradient penalty is an fp32 second-order "
                             "term")
        super().__init__(policy, env=env, **kwargs)
        self.gradient_penalty_coef_schedule = list(grad_penalty_coef_schedule)
        self.counter = 0
        # mini-batch steps whose penalty ran through the fused HIP op (gr_lcp_*), for tests and logs
        self.fused_penalty_steps = 0

    def gradient_penalty_coef(self) -> float:
        return penalty_coef(self.gradient_penalty_coef_schedule, self.counter)

    def update_counter(self):
        self.counter += 1

    # ---------------------------------------------------------------------------------------------- the two paths
    def _use_fused_penalty(self, obs, critic_obs) -> bool:
        pol = self.policy
        return (self._use_fused_losses(obs) and self.fused_mlp
                and _lin.networks_fusable([pol.actor, pol.critic], [obs, critic_obs]))

    def _fused_lcp_loss(self, obs, critic_obs, act, val, adv, ret, logp_old, mu_old, sig_old, coef, acc=None,
                        kl_out=None):
        """(loss, [surrogate, value, KL] means, P): the PPO losses as fused_loss.ppo_loss computes them, with the
        actor's saved activations handed to the fused penalty (fused_lcp.py).  coef: a float or a device scalar."""
        pol = self.policy
        mu, value, h1, z2 = _lin.fused_mlps([pol.actor, pol.critic], [obs, critic_obs], extras=True)
        std = _floss._policy_std(pol)
        loss, stats = _floss.combined_loss(self, mu, value, act, val, adv, ret, logp_old, mu_old, sig_old, acc=acc,
                                           kl_out=kl_out, std=std)
        pen = _flcp.lcp_penalty(pol.actor, mu, std, act.float(), h1, z2)
        self.fused_penalty_steps += 1
        return loss + coef * pen, stats, pen

    def _torch_lcp_loss(self, obs, critic_obs, act, val, adv, ret, logp_old, coef):
        """(loss, surrogate, value loss, P, mu, sigma) in the reference's order of operations (ppo_lcp.py:122-181)."""
        pol = self.policy
        obs_est = obs.clone()
        obs_est.requires_grad_()
        mean = actor_plain(pol.actor, obs_est)
        pol.distribution = Normal(mean, pol._std(mean))
        logp = pol.get_actions_log_prob(act)
        value = pol.evaluate(critic_obs)
        mu_b, sigma_b, entropy_b = pol.action_mean, pol.action_std, pol.entropy
        grad_log_prob = torch.autograd.grad(logp.sum(), obs_est, create_graph=True)[0]
        pen = torch.sum(torch.square(grad_log_prob), dim=-1).mean()
        surrogate_loss, value_loss = self._ppo_losses(logp, logp_old, adv, value, val, ret)
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_b.mean() + coef * pen
        return loss, surrogate_loss, value_loss, pen, mu_b, sigma_b

    def _minibatch_loss(self, batch, acc=None, kl_out=None, seed=None):
        """PPO._minibatch_loss plus coef * P.  The graphed step's coefficient is its device scalar; seed is unused:
        the loss is never the root."""
        coef = self._graphed.coef if acc is not None else self.gradient_penalty_coef()
        if self._use_fused_penalty(batch[0], batch[1]):
            loss, stats, pen = self._fused_lcp_loss(*batch[:9], coef, acc=None if acc is None else acc[:2],
                                                    kl_out=kl_out)
            if acc is not None:
                acc[2:].add_(pen.detach())
                return loss, (), None
            return loss, (stats[0], stats[1], pen.detach()), stats[2]
        loss, surrogate_loss, value_loss, pen, mu, sigma = self._torch_lcp_loss(*batch[:7], coef)
        return (loss, (surrogate_loss.detach(), value_loss.detach(), pen.detach()),
                self._kl_mean(mu, sigma, *batch[7:9], kl_out))

    def update(self):
        coef = self.gradient_penalty_coef()
        out = super().update()
        self.update_counter()
        out["gradient_penalty_coef"] = coef
        return out


class _GraphedStepLCP(_GraphedStep):
    """PPOLCP.update's mini-batch step as hipGraph replays (ppo.py _GraphedStep).  Segment A adds coef * P to the PPO
    loss, with the coefficient in a device scalar (`coef`) filled before each update's replays, so the schedule
    moves without a re-capture."""

    def __init__(self, alg: "PPOLCP"):
        super().__init__(alg)
        self.coef = torch.zeros((), device=alg.device)

    def update(self):
        self.coef.fill_(self.alg.gradient_penalty_coef())
        return super().update()


PPOLCP.graphed_step_cls = _GraphedStepLCP
