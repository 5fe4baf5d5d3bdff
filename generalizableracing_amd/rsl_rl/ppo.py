"""PPO (standalone/rsl_rl/ext/algorithms/ppo.py:14-190) + data parallelism.

Same act / process_env_step (time-out bootstrap) / compute_returns / update
as the reference: clipped surrogate, clipped value loss, adaptive-KL learning
rate, grad-norm clipping, Adam.  Added for the multi-GPU path:
the KL mean is averaged across ranks before the learning-rate decision and
gradients are averaged in one flat all-reduce before clipping, so every rank
applies the identical update.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn
import torch.optim as optim
import torch.distributed as dist

from .. import _abi
from . import distributed as gdist
from . import flat_adam as _fadam
from . import fused_loss as _floss
from . import linear as _lin
from . import rollout_ops as _rops
from .rollout_storage import RolloutStorage


class PPO:
    """One update for the family: `update` below drives every mini-batch step (eager loop or graphed replays);
    a subclass supplies its storage and graphed-step classes, the names of its loss terms and `_minibatch_loss`."""

    storage_cls = RolloutStorage
    graphed_step_cls = None  # _GraphedStep (set below it)
    # the mini-batch means update() averages, in the order _minibatch_loss returns them (an extra term goes last)
    loss_terms = ("surrogate", "value_function")

    def __init__(self, policy, env=None, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998,
                 lam=0.95, value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu",
                 normalize_advantage=True, storage_obs_dtype=torch.float32, fused_rollout_inference=False,
                 fused_rollout_precision="bf16", graph_update=False, update_autocast_bf16=False,
                 graph_update_segmented=False, fused_losses=True, fused_adam=True, fused_mlp=True,
                 graph_update_per_step=False, **kwargs):
        self.env = env
        self.device = device
        self.desired_kl = desired_kl
        self.schedule = schedule
        self.learning_rate = learning_rate
        self.policy = policy
        self.policy.to(self.device)
        gdist.broadcast_params(self.policy)
        self.storage: RolloutStorage | None = None
        # Adam (ppo.py:39) and the grad-norm clip as four device launches over the parameter table on CUDA
        # (flat_adam.py); torch.optim.Adam + nn.utils.clip_grad_norm_ on CPU or with fused_adam=False
        self.optimizer = _fadam.make_adam(self.policy.parameters(), learning_rate, fused=fused_adam)
        self.transition = self.storage_cls.Transition()
        self.clip_param = clip_param
        self.num_learning_epochs = num_learning_epochs
        self.num_mini_batches = num_mini_batches
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.gamma = gamma
        self.lam = lam
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.normalize_advantage = normalize_advantage
        # "float32" / "bfloat16" from a cfg dict, or a torch dtype (BASELINE C5: bf16 rollout obs buffers)
        self.storage_obs_dtype = getattr(torch, storage_obs_dtype) if isinstance(storage_obs_dtype, str) \
            else storage_obs_dtype
        # rollout inference on MFMA (rsl_rl/fused_inference.py, BASELINE config C5): bf16 operands, fp32
        # accumulation, one launch for actor + sampling + log prob + critic; the update stays fp32 PyTorch
        self.fused_rollout_inference = bool(fused_rollout_inference)
        self.fused_rollout_precision = str(fused_rollout_precision)
        self.fused = None
        # the update's mini-batch step (gather, forward, adaptive learning rate, losses, backward, clip,
        # Adam) captured once in a hipGraph and replayed per mini-batch (single rank, GPU): see _GraphedStep
        self.graph_update = bool(graph_update)
        # two graph segments with the collectives run eagerly between them: always at world size > 1; this
        # switch forces it on one rank (tests: the segmented step must equal the single graph)
        self.graph_update_segmented = bool(graph_update_segmented)
        # one graph per mini-batch step instead of one per epoch (the state between steps can be inspected: tests)
        self.graph_update_per_step = bool(graph_update_per_step)
        self._graphed = None
        self._grads_checked = False  # which parameters the loss reaches (see _check_all_grads)
        self._unused: set = set()
        # not in the reference (fp32 update): forward/backward of the update under torch.autocast(bf16);
        # the losses' exp / log / sums stay fp32 (autocast's fp32 list), parameters and Adam stay fp32
        self.update_autocast_bf16 = bool(update_autocast_bf16)
        self._flat = None  # gdist.FlatGrads: the parameters' gradients as views of one buffer
        # the mini-batch losses (log prob, KL, surrogate, value loss) as one device op each way on CUDA
        # (fused_loss.py); False: the torch ops
        self.fused_losses = bool(fused_losses)
        # with the fused losses: the actor and critic MLPs as whole-network fp32-MFMA kernels (linear.fused_mlps)
        self.fused_mlp = bool(fused_mlp)
        # a policy with memories (ActorCriticRecurrent): the update runs them over each mini-batch's [T, B] block
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        self._refuse_recurrent()

    # what a recurrent policy (ActorCriticRecurrent) cannot be combined with yet, by constructor argument
    _RECURRENT_REFUSALS = ("graph_update", "fused_rollout_inference", "update_autocast_bf16")

    def _refuse_recurrent(self):
        if not self.recurrent:
            return
        if type(self) is not PPO:
            raise ValueError(f"{type(self).__name__} does not support a recurrent policy: its extra loss term reads "
                             "single observations, not sequences; use PPO.")
        for name in self._RECURRENT_REFUSALS:
            if getattr(self, name):
                raise ValueError(f"PPO: {name}=True is not supported with a recurrent policy (the recurrent update "
                                 "runs eagerly in fp32 and the rollout steps the policy's own memories).")

    def flat_grads(self) -> gdist.FlatGrads:
        """The flat gradient buffer over the parameters the loss reaches (all of them until the first mini-batch
        has been checked, see _check_all_grads)."""
        used = [p for p in self.policy.parameters() if id(p) not in self._unused]
        if self._flat is None or len(self._flat.params) != len(used) or \
                any(a is not b for a, b in zip(self._flat.params, used)):
            self._flat = gdist.FlatGrads(used)
        return self._flat

    def init_storage(self, training_type, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape,
                     action_shape):
        self.storage = self.storage_cls(training_type, num_envs, num_transitions_per_env, actor_obs_shape,
                                        critic_obs_shape, action_shape, self.device, obs_dtype=self.storage_obs_dtype)
        self._init_fused(num_envs)

    def _init_fused(self, num_envs):
        if not self.fused_rollout_inference:
            return
        from .fused_inference import FusedPolicyInference

        ucfg = getattr(getattr(self.env, "unwrapped", None), "cfg", None)
        seed = getattr(ucfg, "seed", None)
        self.fused = FusedPolicyInference(self.policy, num_envs, self.device, seed=42 if seed is None else int(seed),
                                          env_id_offset=int(getattr(ucfg, "env_id_offset", 0) or 0),
                                          precision=self.fused_rollout_precision)

    def test_mode(self):
        self.policy.eval()

    def train_mode(self):
        self.policy.train()

    def act(self, obs, critic_obs):
        if self.fused is not None:
            a, v, lp, mu, sd = self.fused.act(obs, critic_obs)
            self.transition.actions, self.transition.values, self.transition.actions_log_prob = a, v, lp
            self.transition.action_mean, self.transition.action_sigma = mu, sd
            self.transition.observations = obs
            self.transition.privileged_observations = critic_obs
            return a
        if self.recurrent and self.storage.step == 0:
            # ppo.py:72-73 saves the hidden states before acting at every step; the masked sequence needs those of
            # rollout step 0 only.  The transition carries them to the storage; a memory on the fused step writes
            # the storage's h0 itself (gr_gru_step's second pointer) and hands None
            self.transition.hidden_states = self.policy.stage_hidden_states(
                obs, critic_obs, *self.storage.h0_buffers(*self.policy.get_hidden_sizes()))
        self.transition.actions = self.policy.act(obs).detach()
        self.transition.values = self.policy.evaluate(critic_obs).detach()
        self.transition.actions_log_prob = self.policy.get_actions_log_prob(self.transition.actions).detach()
        self.transition.action_mean = self.policy.action_mean.detach()
        self.transition.action_sigma = self.policy.action_std.detach()
        self.transition.observations = obs
        self.transition.privileged_observations = critic_obs
        return self.transition.actions

    def process_env_step(self, rewards, dones, infos):
        tos = infos.get("time_outs")
        tos = tos.to(self.device) if tos is not None else None
        if _rops.store_ok(self.storage, self.transition, rewards, dones, tos):
            # the bootstrap below and add_transitions as one launch (rollout_ops.py), the same bits
            _rops.store_transition(self.storage, self.transition, rewards, dones, tos, self.gamma)
            self.transition.clear()
            self.policy.reset(dones)
            return
        self._stage_rewards(rewards, dones, infos)
        self.storage.add_transitions(self.transition)
        self.transition.clear()
        self.policy.reset(dones)

    def _stage_rewards(self, rewards, dones, infos):
        """The step's rewards and dones into the transition, bootstrapping on time outs (ppo.py:88-92)."""
        self.transition.rewards = rewards.clone()
        self.transition.dones = dones
        if "time_outs" in infos:
            self.transition.rewards += self.gamma * torch.squeeze(
                self.transition.values * infos["time_outs"].unsqueeze(1).to(self.device), 1)

    def compute_returns(self, last_critic_obs):
        last_values = self.policy.evaluate(last_critic_obs).detach()
        self.storage.compute_returns(last_values, self.gamma, self.lam, self.normalize_advantage)

    def _adaptive(self) -> bool:
        return self.desired_kl is not None and self.schedule == "adaptive"

    def _kl_mean(self, mu, sigma, mu_old, sig_old, out=None):
        """The mini-batch's mean KL between the old and the new Gaussians (ppo.py:133-141), None off the adaptive
        schedule; written to out [1] when given (the graphed step's device sink)."""
        if not self._adaptive():
            return None
        with torch.no_grad():
            kl = torch.sum(torch.log(sigma / sig_old + 1.0e-5)
                           + (torch.square(sig_old) + torch.square(mu_old - mu)) / (2.0 * torch.square(sigma)) - 0.5,
                           axis=-1)
            kl = torch.mean(kl)
            if out is not None:
                out[0].copy_(kl)
        return kl

    def _adapt_learning_rate(self, kl_mean):
        """Adaptive KL learning rate (ppo.py:142-150) on the host; the KL mean is averaged over ranks first."""
        if not self._adaptive():
            return
        kl_val = float(gdist.allreduce_mean(kl_mean.detach()))  # host decision, as in the reference
        if kl_val > self.desired_kl * 2.0:
            self.learning_rate = max(1e-5, self.learning_rate / 1.5)
        elif self.desired_kl / 2.0 > kl_val > 0.0:
            self.learning_rate = min(1e-2, self.learning_rate * 1.5)
        for g in self.optimizer.param_groups:
            g["lr"] = self.learning_rate

    def _ppo_losses(self, actions_log_prob_batch, old_actions_log_prob_batch, advantages_batch, value_batch,
                    target_values_batch, returns_batch):
        """Clipped surrogate (ppo.py:152-158) and (clipped) value loss (ppo.py:160-169)."""
        ratio = torch.exp(actions_log_prob_batch - torch.squeeze(old_actions_log_prob_batch))
        surrogate = -torch.squeeze(advantages_batch) * ratio
        surrogate_clipped = -torch.squeeze(advantages_batch) * torch.clamp(ratio, 1.0 - self.clip_param,
                                                                           1.0 + self.clip_param)
        surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
        if self.use_clipped_value_loss:
            value_clipped = target_values_batch + (value_batch - target_values_batch).clamp(-self.clip_param,
                                                                                            self.clip_param)
            value_losses = (value_batch - returns_batch).pow(2)
            value_losses_clipped = (value_clipped - returns_batch).pow(2)
            value_loss = torch.max(value_losses, value_losses_clipped).mean()
        else:
            value_loss = (returns_batch - value_batch).pow(2).mean()
        return surrogate_loss, value_loss

    def _check_all_grads(self, loss, params, grads=None):
        """Find the parameters the loss does not reach (e.g. VisionActorCritic's aux_decoder) and take them out of
        the flat gradient buffer, with `.grad` None: the reference's `zero_grad()` leaves their `.grad` None and
        Adam skips them (ppo.py:178-181), where a bound zero `.grad` would count an Adam step for them (and step
        them by their moments if they ever had any).  Checked once, on the first mini-batch: the set of parameters
        the loss reaches must not change afterwards.  The eager update raises if a dropped parameter later receives a
        gradient (PPO.update); the graphed update differentiates only the parameters kept here."""
        if grads is None:
            grads = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
        self._unused = {id(p) for p, g in zip(params, grads) if g is None}
        for p in self.policy.parameters():
            if id(p) in self._unused:
                p.grad = None
        self._grads_checked = True
        return self.flat_grads()

    def update(self):
        if self.graph_update and self.storage is not None and str(self.device).startswith("cuda"):
            if self._graphed is None:
                self._graphed = self.graphed_step_cls(self)
            out = self._graphed.update()
            if self.fused is not None:  # graph replays write the parameters without bumping their versions
                self.fused.refresh()
            return out
        sums = [torch.zeros((), device=self.device) for _ in self.loss_terms]
        if self.recurrent:  # ppo.py:106-109
            generator = self.storage.recurrent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        else:
            generator = self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        params = list(self.policy.parameters())
        flat = self.flat_grads()
        flat.bind()
        for batch in generator:
            loss, terms, kl = self._minibatch_loss(batch)
            self.optimizer.zero_grad(set_to_none=False)  # (in place: the views of the flat buffer stay bound)
            if not self._grads_checked:
                flat = self._check_all_grads(loss, params)
                flat.bind()
            loss.backward()
            if self._unused and any(p.grad is not None for p in params if id(p) in self._unused):
                raise RuntimeError("PPO.update: a parameter the loss did not reach on the first mini-batch now has a "
                                   "gradient; the set of parameters the loss reaches must be fixed from the first "
                                   "mini-batch (it is checked once: _check_all_grads)")
            self._adapt_learning_rate(kl)  # (the rate only enters optimizer.step; ahead of the gradients' exchange)
            gdist.allreduce_grads(params, flat)
            _fadam.clip_grad_norm_(self.optimizer, params, self.max_grad_norm)
            self.optimizer.step()
            for s, t in zip(sums, terms):
                s += t
        self.storage.clear()
        return self._stats([float(s) for s in sums])

    def _stats(self, sums):
        """update()'s result from the sums of the mini-batch means (in loss_terms order)."""
        n = self.num_learning_epochs * self.num_mini_batches
        mean = {k: v / n for k, v in zip(self.loss_terms, sums)}
        return {k: mean[k] for k in ("value_function", "surrogate") + self.loss_terms[2:]}

    def _use_fused_losses(self, obs) -> bool:
        return (self.fused_losses and obs.is_cuda and not self.update_autocast_bf16
                and _floss.fused_losses_ok(self.policy, obs))

    def _minibatch_loss(self, batch, acc=None, kl_out=None, seed=None):
        """(loss, terms, KL mean) of one mini-batch, `batch` as the storage's generator yields it (the graphed step
        gathers the same fields).  terms: the detached means named by loss_terms.  The eager loop passes nothing
        else.  The graphed step passes its device sinks, and nothing here may then read back to the host: acc holds
        the update's sums of the terms (a path whose fused op adds to it adds all its terms and returns none), the KL
        mean goes to kl_out [1] too (given on the adaptive schedule only; the return value is not read), and seed is
        the tensor autograd will be seeded with, for a loss that is its root (fused_loss.combined_loss)."""
        if self.recurrent:  # ppo.py:123-127: the memories over the block, then the same losses per row
            return self._recurrent_loss(batch)
        if self._use_fused_losses(batch[0]):  # the same losses as one device op each way (fused_loss.py)
            loss, stats = _floss.ppo_loss(self, *batch[:9], acc=acc, kl_out=kl_out, seed=seed)
            return loss, () if acc is not None else (stats[0], stats[1]), stats[2]
        autocast = self.update_autocast_bf16 and str(self.device).startswith("cuda")
        return self._torch_ppo_loss(*batch[:9], kl_out, draw=acc is None, autocast=autocast)[:3]

    def _recurrent_loss(self, batch):
        """_minibatch_loss for a recurrent policy: `batch` as recurrent_mini_batch_generator yields it.  The memories
        run over the [T, B] block (policy.act / evaluate with masks = the block's dones and hidden_states = its h0) on
        the inputs the policy forms from the observation blocks (memory_inputs: the blocks themselves for
        ActorCriticRecurrent, the stem's features for VisionActorCriticRecurrent); from the [T * B]-row memory outputs
        on, the feed-forward code runs unchanged on the policy's heads."""
        obs, critic_obs = batch[0], batch[1]
        (h0_a, h0_c), dones = batch[9], batch[10]
        pol = self.policy
        x_a, x_c = pol.memory_inputs(obs, critic_obs)
        feat_a = pol.memory_a(x_a, dones, h0_a)
        feat_c = pol.memory_c(x_c, dones, h0_c)
        rest = batch[2:9]
        # (the heads module by module: linear.networks_fusable refuses inputs that need a gradient, as these do)
        if self._use_fused_losses(feat_a):
            loss, stats = _floss.ppo_loss(self, feat_a, feat_c, *rest)
            return loss, (stats[0], stats[1]), stats[2]
        return self._torch_ppo_loss(feat_a, feat_c, *rest, heads_only=True)[:3]

    def _torch_ppo_loss(self, obs, critic_obs, act, val, adv, ret, logp_old, mu_old, sig_old, kl_out=None, draw=True,
                        autocast=False, heads_only=False):
        """ppo.py:103-172 as torch ops (CPU, autocast, other policies): _minibatch_loss's triple, then the action
        mean and the value.  draw: through policy.act, whose sample nobody uses but which advances the generator as
        the reference does (the eager loops); torch.normal's check of the std reads back to the host, which a capture
        forbids, so the graphed steps only set the distribution.  heads_only: obs / critic_obs are the memories'
        outputs of a recurrent policy (_recurrent_loss): the actor and the critic heads on them."""
        pol = self.policy
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if heads_only:
                pol.set_distribution(pol.actor(obs), draw)
            else:
                pol.act(obs) if draw else pol.update_distribution(obs)
            logp = pol.get_actions_log_prob(act)
            value = pol.critic(critic_obs) if heads_only else pol.evaluate(critic_obs)
            mu, sigma, entropy = pol.action_mean, pol.action_std, pol.entropy
        if not heads_only:  # (fp32 from autocast's bf16; the recurrent path has no autocast and keeps a float64
            # policy, which its CPU golden test steps, in float64)
            logp, value, mu, sigma, entropy = (t.float() for t in (logp, value, mu, sigma, entropy))
        kl = self._kl_mean(mu, sigma, mu_old, sig_old, kl_out)
        surrogate_loss, value_loss = self._ppo_losses(logp, logp_old, adv, value, val, ret)
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy.mean()
        return loss, (surrogate_loss.detach(), value_loss.detach()), kl, mu, value


class _GraphedStep:
    """PPO.update's mini-batch step as hipGraph replays (the same operations as the eager loop).

    Per mini-batch the eager loop launches ~150 small kernels and reads the KL back to the host for the
    adaptive learning rate (ppo.py:133-150).  Here the learning-rate rule runs on the device (the same
    comparisons, in fp32), Adam takes the rate as a device tensor (FlatAdam's lr pointer, or torch's
    `capturable=True` with fused_adam off), and the step
    (mini-batch gathers from the storage by a static index buffer, forward, losses, backward, grad
    clipping, Adam) is captured once and replayed per mini-batch.  Capture needs warm-up steps; the
    parameters, the optimizer state and the rate are snapshotted before and restored after, so training
    is unchanged.  `learning_rate` is read back once per update, for the log.

    Gradients: `torch.autograd.grad` into the views of one flat buffer (gdist.FlatGrads, bound as the
    parameters' `.grad` before capture and never rebound), so the captured step does not depend on how
    autograd's gradient accumulation treats an existing `.grad` (an out-of-place accumulation during
    capture rebinds `.grad` and leaves the graph writing a buffer nobody holds).  The mini-batch's local KL
    mean is written into the flat buffer's extra slot.

    Two segments: A = gathers, forward, KL, losses, backward (into the flat buffer); B = learning-rate rule,
    clip, Adam.  The rate only enters Adam, so computing it after the backward changes nothing.  With one
    rank both segments of every mini-batch of an epoch are one graph (each step gathers by its own slice of the
    update's permutation), replayed once per epoch.  With several ranks (any backend) they are two graphs and the exchange
    runs eagerly between them: ONE in-place all-reduce of the flat buffer carries the gradients and the KL
    mean together.  No collective is ever captured."""

    _PACK = True  # gather the mini-batch from the storage's packed sample rows when it has them

    def __init__(self, alg: "PPO"):
        self.alg = alg
        st, dev = alg.storage, alg.device
        self.T, self.N = st.num_transitions_per_env, st.num_envs
        self.mb = self.T * self.N // alg.num_mini_batches
        self.params = list(alg.policy.parameters())
        self.lr = torch.tensor(float(alg.learning_rate), device=dev, dtype=torch.float32)
        old = alg.optimizer
        if isinstance(old, _fadam.FlatAdam):  # the same launches eager or captured: the rate as a device tensor
            self.opt = old
            self.opt.param_groups[0]["lr"] = self.lr
        else:
            self.opt = optim.Adam(self.params, lr=self.lr, capturable=True)
            if old.state:  # resumed from a checkpoint: keep Adam's moments and step counts
                self.opt.load_state_dict(old.state_dict())
            for g in self.opt.param_groups:  # (load_state_dict brings the eager groups' settings)
                g["lr"] = self.lr
                g["capturable"] = True
        alg.optimizer = self.opt
        self.flat = alg.flat_grads()
        self.nmb = alg.num_mini_batches
        # the update's permutation (rollout_storage.py:152-191: one draw, the same mini-batch partition every epoch);
        # one rank: ONE graph holds an epoch's mini-batch steps, each gathering by its own slice of this buffer (no
        # per-step index copy or replay launch); several ranks: per-step graphs read `idx`, refilled per step
        self.perm = torch.zeros(self.nmb * self.mb, dtype=torch.long, device=dev)
        self.idx = self.perm[:self.mb]
        # packed sample rows (None: gathered field by field); a subclass gathering its own fields sets _PACK False and
        # never allocates the buffer
        self.cols = st.sample_columns() if self._PACK else None
        # persistent: the graphs read it (the storage's own packed buffer, shared with the eager generator)
        self.pack = st.pack_samples(out=st.packed_buffer()) if self.cols is not None else None
        self.acc = torch.zeros(len(alg.loss_terms), device=dev)  # the update's sums of the loss terms' means
        self.one = torch.ones((), device=dev)
        self.segmented = gdist.is_dist() or alg.graph_update_segmented
        self.per_step = self.segmented or alg.graph_update_per_step
        # epoch graph + packed rows: the samples in the update's permutation order, gathered ONCE per update (every
        # epoch uses the same partition, rollout_storage.py:152-191), so mini-batch i is the contiguous row slice i and
        # the captured steps gather nothing (the per-step gathers were latency-bound launches, one per step)
        self.pack_perm = torch.empty_like(self.pack) if self.pack is not None and not self.per_step else None
        self.graph = None  # one rank: an epoch's steps (per_step: one step)
        self.graph_b = None  # segmented: graph = segment A, graph_b = segment B

    def _gather(self, idx):
        """The mini-batch's fields by a static index buffer: one row gather of the packed samples (refilled
        before every update's replays, RolloutStorage.pack_samples), or one gather per field for wide rows.  idx a
        (lo, hi) pair: rows lo .. hi of the permuted packed samples (pack_perm), views, no gather."""
        st = self.alg.storage
        if isinstance(idx, tuple):
            g = self.pack_perm[idx[0]:idx[1]]
            return tuple(g[:, a:b] for a, b in self.cols)
        if self.cols is not None:
            g = self.pack.index_select(0, idx)
            return tuple(g[:, a:b] for a, b in self.cols)
        g = tuple(x.index_select(0, idx) for x in st.sample_sources())
        return (g[0].float(), g[1].float()) + g[2:]  # (fp32 observations, as the generator yields them)

    @contextlib.contextmanager
    def _grad_sink(self):
        """While set, the fused ops write their gradients into the flat buffer's views directly
        (linear._GRAD_SINK): the step copies only the others."""
        _lin._GRAD_SINK = {id(p): v for p, v in zip(self.flat.params, self.flat.views)}
        try:
            yield
        finally:
            _lin._GRAD_SINK = None

    def _seg_a(self, idx=None):
        """Gather, the algorithm's loss with the device sinks (PPO._minibatch_loss), backward."""
        alg = self.alg
        batch = self._gather(self.idx if idx is None else idx)
        with self._grad_sink():  # (a seeded fused loss has its gradients in its forward already)
            loss, terms, _ = alg._minibatch_loss(batch, acc=self.acc, seed=self.one,
                                                 kl_out=self.flat.extra[:1] if alg._adaptive() else None)
        if terms:  # (the torch ops: no fused op has added them up)
            self.acc.add_(torch.stack(terms))
        self._backward(loss)

    def _backward(self, loss):
        alg = self.alg
        if not alg._grads_checked:  # (first warm-up step, before any capture)
            grads = torch.autograd.grad(loss, self.params, retain_graph=True, allow_unused=True)
            self.flat = alg._check_all_grads(loss, self.params, grads)
            self.flat.bind()
        with self._grad_sink():  # (the seed gradient from a persistent 1: no fill launch in the captured step)
            grads = torch.autograd.grad(loss, self.flat.params, grad_outputs=self.one)
        pairs = [(v, g) for v, g in zip(self.flat.views, grads) if g.data_ptr() != v.data_ptr()]
        if pairs:
            torch._foreach_copy_([v for v, _ in pairs], [g for _, g in pairs])

    def _seg_b(self):
        alg = self.alg
        if isinstance(self.opt, _fadam.FlatAdam):  # the rate rule, the clip and Adam: two launches (gr_adam_clip_step)
            self.opt.clip_and_step(alg.max_grad_norm, kl=self.flat.extra if alg._adaptive() else None,
                                   desired_kl=alg.desired_kl)
            return
        if alg._adaptive():  # on the rank-averaged KL mean once the flat buffer has been all-reduced: the
            # comparisons of ppo.py:133-150 on the device, one launch (gr_adaptive_lr)
            _abi.call("gr_adaptive_lr", self.flat.extra.data_ptr(), self.lr.data_ptr(), alg.desired_kl, 1e-5, 1e-2,
                      _abi.raw_stream(self.lr.device))
        _fadam.clip_grad_norm_(self.opt, self.params, alg.max_grad_norm)
        self.opt.step()

    def _capture(self):
        # snapshot (parameters, optimizer state, rate), warm up on a side stream, capture, restore
        snap_p = [p.detach().clone() for p in self.params]
        # (the module's buffers too: the warm-up and captured steps' BatchNorm running statistics and batch counts)
        bufs = list(self.alg.policy.buffers())
        snap_bufs = [b.detach().clone() for b in bufs]
        snap_lr = self.lr.clone()
        snap_acc = self.acc.clone()
        self.flat.bind()  # Adam and the clip read the gradients from these views (static addresses)
        snap_o = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.opt.state[p].items()}
                  for p in self.params}
        self.perm.copy_(torch.arange(self.perm.numel(), device=self.perm.device))
        self._permute_pack()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        _lin._FORCE_FN = True  # bias gradients by gr_column_sum in the captured step (linear.bias_grad)
        try:
            with torch.cuda.stream(s):
                for _ in range(3):  # (no collective in the warm-up: its results are discarded)
                    self._seg_a()
                    self._seg_b()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            if self.segmented:
                with torch.cuda.graph(self.graph, stream=s):
                    self._seg_a()
                self.graph_b = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_b, stream=s, pool=self.graph.pool()):
                    self._seg_b()
            elif self.per_step:
                with torch.cuda.graph(self.graph, stream=s):
                    self._seg_a()
                    self._seg_b()
            else:  # an epoch: every mini-batch step, each on its slice of the permutation
                with torch.cuda.graph(self.graph, stream=s):
                    for i in range(self.nmb):
                        lo, hi = i * self.mb, (i + 1) * self.mb
                        self._seg_a((lo, hi) if self.pack_perm is not None else self.perm[lo:hi])
                        self._seg_b()
        finally:
            _lin._FORCE_FN = False
        with torch.no_grad():
            for p, v in zip(self.params, snap_p):
                p.copy_(v)
            for p in self.params:
                for k, v in snap_o[id(p)].items():
                    if torch.is_tensor(v):
                        self.opt.state[p][k].copy_(v)
            for b, v in zip(bufs, snap_bufs):
                b.copy_(v)
            self.lr.copy_(snap_lr)
            self.acc.copy_(snap_acc)

    def _permute_pack(self):
        if self.pack_perm is not None:
            torch.index_select(self.pack, 0, self.perm, out=self.pack_perm)

    def _refresh_sources(self):
        """Before an update's replays: this rollout's samples, packed in place (the graphs read the buffer)."""
        if self.pack is not None:
            self.alg.storage.pack_samples(out=self.pack)

    def update(self):
        alg = self.alg
        n = alg.num_mini_batches
        perm = torch.randperm(n * self.mb, device=self.perm.device)  # rollout_storage.py:152-191, drawn first
        self._refresh_sources()
        if self.graph is None:
            had_state = bool(self.opt.state)
            if not had_state:  # Adam's first step creates its state: take it with zero gradients, then undo
                snap_p = [p.detach().clone() for p in self.params]
                self.flat.bind()
                self.flat.flat.zero_()
                self.opt.step()
                with torch.no_grad():
                    for p, v in zip(self.params, snap_p):
                        p.copy_(v)
                    for p in self.params:
                        for k, v in self.opt.state[p].items():
                            if torch.is_tensor(v):
                                v.zero_()
            self._capture()
        self.lr.fill_(float(alg.learning_rate))
        self.acc.zero_()
        if not self.per_step:
            self.perm.copy_(perm)
            self._permute_pack()
        for _ in range(alg.num_learning_epochs):
            if not self.per_step:  # one replay per epoch
                self.graph.replay()
                continue
            for i in range(n):
                self.idx.copy_(perm[i * self.mb:(i + 1) * self.mb])
                self.graph.replay()
                if self.graph_b is not None:
                    self.flat.allreduce_()  # eager, on the current stream's order: gradients + KL mean, one message
                    self.graph_b.replay()
        alg.learning_rate = float(self.lr)
        alg.storage.clear()
        return alg._stats(self.acc.tolist())


PPO.graphed_step_cls = _GraphedStep
