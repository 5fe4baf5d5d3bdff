"""AlgoRunner (standalone/diff_rl/algorithms/runner.py): the diff_rl training loop, its log keys and checkpoints."""
from __future__ import annotations

import os
import statistics
import time
from collections import deque

import torch

from ..rsl_rl.on_policy_runner import _make_writer
from .bptt import BPTT
from .model import BaseModel

ALGORITHMS = {"BPTT": BPTT}
MODELS = {"BaseModel": BaseModel}


class AlgoRunner:
    def __init__(self, env, agent_cfg: dict, log_dir: str | None = None, device="cpu"):
        self.cfg = agent_cfg
        self.alg_cfg = dict(agent_cfg["algorithm"])
        self.policy_cfg = dict(agent_cfg["policy"])
        self.device = device
        self.env = env
        if agent_cfg.get("empirical_normalization"):
            raise NotImplementedError("empirical_normalization is not built for the diff_rl workflow")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("the diff_rl workflow runs on one GPU")
        obs, extras = self.env.get_observations()
        num_obs = obs.shape[1]
        crit = extras["observations"].get("critic")
        num_critic_obs = crit.shape[1] if crit is not None else num_obs
        model = MODELS[self.policy_cfg.pop("class_name")](num_obs, num_critic_obs, self.env.num_actions,
                                                         **self.policy_cfg).to(self.device)
        self.alg = ALGORITHMS[self.alg_cfg.pop("class_name")](actor_critic=model,
                                                             max_iterations=agent_cfg["max_iterations"],
                                                             device=self.device, **self.alg_cfg)
        self.alg.env = self.env.unwrapped
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]
        self.log_dir = log_dir
        self.writer = None
        self.tot_timesteps = 0
        self.tot_time = 0.0
        self.current_learning_iteration = 0
        self.last_log: dict = {}
        self.log_history: list | None = None  # a list: every iteration's scalars are appended to it
        # one switch, the env's: a runner cfg that asks for the other path than the env's tape runs is an error
        tape = getattr(self.env.unwrapped, "_diff", None) or getattr(self.env.unwrapped, "diff", None)
        want = agent_cfg.get("fused")
        if tape is not None and want is not None and bool(want) != bool(tape.fused):  # (no tape: play)
            raise ValueError(f"the runner cfg has fused={bool(want)} but the env's tape was built with "
                             f"fused={bool(tape.fused)} (RacingEnvCfg.diff_fused): make them agree")

    def train_mode(self):
        self.alg.train_mode()

    def eval_mode(self):
        self.alg.test_mode()

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False):
        if self.log_dir is not None and self.writer is None:
            self.writer = _make_writer(self.log_dir, str(self.cfg.get("logger", "tensorboard")).lower())
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf,
                                                             high=int(self.env.max_episode_length))
        obs, extras = self.env.get_observations()
        critic_obs = extras["observations"].get("critic", obs)
        self.train_mode()
        n, dev = self.env.num_envs, self.device
        ep_infos = []
        bufs = {k: deque(maxlen=100) for k in ("reward", "loss", "loss_detached", "loss_total", "length")}
        sums = {k: torch.zeros(n, dtype=torch.float32, device=dev) for k in bufs}
        start_iter = self.current_learning_iteration
        tot_iter = start_iter + num_learning_iterations
        for it in range(start_iter, tot_iter):
            start = time.time()
            self.env.unwrapped.detach()  # the window starts here
            for _ in range(self.num_steps_per_env):
                actions = self.alg.act(obs, critic_obs)
                obs, rewards, dones, extras = self.env.step(actions)
                critic_obs = extras["observations"].get("critic", obs)
                loss, loss_detached = extras["losses"], extras["losses_detached"]
                self.alg.process_env_step(loss, loss_detached, dones, rewards, extras)
                if self.log_dir is not None:
                    if "log" in extras:
                        ep_infos.append(extras["log"])
                    sums["reward"] += rewards
                    sums["loss"] += loss
                    sums["loss_detached"] += loss_detached
                    sums["loss_total"] += loss + loss_detached
                    sums["length"] += 1
                    new_ids = (dones > 0).nonzero(as_tuple=False)[:, 0]
                    if new_ids.numel():
                        for k in bufs:
                            bufs[k].extend(sums[k][new_ids].cpu().numpy().tolist())
                            sums[k][new_ids] = 0
            stop = time.time()
            collection_time = stop - start
            start = stop
            mean_value_loss, mean_policy_loss = self.alg.update()
            mean_policy_loss = float(mean_policy_loss)  # (synchronises: the iteration's work is done)
            learn_time = time.time() - start
            self.current_learning_iteration = it
            if self.log_dir is not None:
                self.log(it, tot_iter, collection_time, learn_time, mean_value_loss, mean_policy_loss, bufs, ep_infos)
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
            ep_infos.clear()
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
        self.current_learning_iteration = tot_iter  # (a further learn() in this process goes on from here)

    def log(self, it, tot_iter, collection_time, learn_time, mean_value_loss, mean_policy_loss, bufs, ep_infos,
            width: int = 80, pad: int = 35):
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
        self.tot_time += collection_time + learn_time
        fps = int(self.num_steps_per_env * self.env.num_envs / (collection_time + learn_time))
        scalars = {}
        if ep_infos:
            for key in ep_infos[0]:
                vals = [torch.as_tensor(e[key], dtype=torch.float32).reshape(-1).to(self.device) for e in ep_infos
                        if key in e]
                scalars[key if "/" in key else "Episode/" + key] = float(torch.cat(vals).mean())
        mean_std = float(self.alg.actor_critic.noise_std().detach().mean())
        scalars.update({"Loss/value_function": mean_value_loss, "Loss/policy": mean_policy_loss,
                        "Loss/learning_rate": self.alg.learning_rate, "Policy/mean_noise_std": mean_std,
                        "Perf/total_fps": fps, "Perf/collection_time": collection_time,
                        "Perf/learning_time": learn_time})
        if len(bufs["reward"]) > 0:
            scalars.update({"Train/mean_reward": statistics.mean(bufs["reward"]),
                            "Train/mean_loss": statistics.mean(bufs["loss"]),
                            "Train/mean_loss_detached": statistics.mean(bufs["loss_detached"]),
                            "Train/mean_loss_total": statistics.mean(bufs["loss_total"]),
                            "Train/mean_episode_length": statistics.mean(bufs["length"])})
        for k, v in scalars.items():
            self.writer.add_scalar(k, v, it)
        self.last_log = dict(scalars)
        if self.log_history is not None:
            self.log_history.append(dict(scalars))
        head = f" Learning iteration {it}/{tot_iter} "
        s = f"{'#' * width}\n{head.center(width, ' ')}\n\n"
        s += (f"{'Computation:':>{pad}} {fps:.0f} steps/s (collection: {collection_time:.3f}s, learning "
              f"{learn_time:.3f}s)\n{'Policy loss:':>{pad}} {mean_policy_loss:.4f}\n"
              f"{'Mean action noise std:':>{pad}} {mean_std:.2f}\n")
        if len(bufs["reward"]) > 0:
            s += (f"{'Mean reward:':>{pad}} {scalars['Train/mean_reward']:.2f}\n"
                  f"{'Mean total loss:':>{pad}} {scalars['Train/mean_loss_total']:.4f}\n"
                  f"{'Mean episode length:':>{pad}} {scalars['Train/mean_episode_length']:.2f}\n")
        s += (f"{'-' * width}\n{'Total timesteps:':>{pad}} {self.tot_timesteps}\n"
              f"{'Total time:':>{pad}} {self.tot_time:.2f}s\n")
        print(s, flush=True)

    def save(self, path, infos=None):
        torch.save({"model_state_dict": self.alg.actor_critic.state_dict(),
                    "optimizer_state_dict": self.alg.optimizer.state_dict(),
                    "iter": self.current_learning_iteration, "infos": infos}, path)

    def load(self, path, load_optimizer=True):
        loaded = torch.load(path, weights_only=True, map_location=self.device)
        self.alg.actor_critic.load_state_dict(loaded["model_state_dict"])
        if load_optimizer:
            self.alg.optimizer.load_state_dict(loaded["optimizer_state_dict"])
        self.current_learning_iteration = loaded["iter"]
        return loaded["infos"]

    def get_inference_policy(self, device=None):
        self.eval_mode()
        if device is not None:
            self.alg.actor_critic.to(device)
        return self.alg.actor_critic.act_inference
