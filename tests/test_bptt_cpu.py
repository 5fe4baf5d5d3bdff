"""The diff_rl workflow on the CPU, over the oracle-backed differentiable env (tests/oracle_diff_vecenv.py).

  * the torch path of diff_ops in float64 equals the float64 restatement tests/bptt_ref.py on the same planes;
  * BPTT.update's batched recompute (one forward over the T * N rows, a.backward(G)) gives the parameter gradients of
    the reference's structure (T forwards kept in the graph, the window's autograd graph through the actions, then
    total.backward()), in float64 to 1e-10 of each gradient's norm;
  * two iterations of AlgoRunner (T = 4, 16 envs) run, change every parameter that has a gradient, log the
    reference's keys, follow the cosine schedule, and the checkpoint round-trips."""
import math

import pytest
import torch

import bptt_ref
import diff_window as dw
from generalizableracing_amd.diff_rl import AlgoRunner, BaseModel, BPTT, QuadcopterDiffRLRunnerCfg
from oracle_diff_vecenv import OracleDiffVecEnv


@pytest.mark.parametrize("lag", [0, 1])
def test_torch_path_equals_restatement(lag):
    T, N = 6, 48
    env = dw.oracle_window(T, N, lag, seed=3, dtype=torch.float64)
    G = env.loss_action_grad()
    k = dict(env.diff.k, scale=1.0 / (T * N))
    ref = bptt_ref.window(bptt_ref.tape_fields(env.diff.tape), k)
    assert int((env.diff.tape[:, 17, :, 3] != 0).sum()) >= 3  # the forced resets are in the window
    assert float(ref["grad"].abs().max()) > 0
    for a, b in ((G, ref["grad"]), (env.diff.losses, ref["losses"]), (env.diff.terms, ref["terms"])):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())


@pytest.mark.parametrize("lag", [0, 1])
def test_batched_recompute_equals_reference_structure(lag):
    T, N = 5, 16
    torch.manual_seed(0)
    env = OracleDiffVecEnv(num_envs=N, lag=lag, t_max=T, dtype=torch.float64)
    model = BaseModel(16, 16, 4, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="lrelu").double()
    alg = BPTT(model, max_iterations=10, learning_rate=1e-3, optimizer="AdamW", device="cpu")
    alg.env = env
    obs, _ = env.get_observations()
    env.detach()
    kept = []  # the reference's structure: each step's action stays in the graph
    for t in range(T):
        dw.force_timeouts(env, t, T, N)
        a = alg.act(obs.double())
        kept.append(model.actor(alg.obs[-1]) + model.noise_std() * alg.eps[-1])
        assert torch.equal(kept[-1].detach(), a)
        obs, _, dones, extras = env.step(a)
        alg.process_env_step(extras["losses"], extras["losses_detached"], dones)
    # total.backward() through the window's autograd graph with the actions as its inputs
    k = dict(env.diff.k, scale=1.0 / (T * N))
    acts = torch.stack(kept)
    G_ref = bptt_ref.window(bptt_ref.tape_fields(env.diff.tape), k, a=acts.detach())["grad"]
    model.zero_grad()
    acts.backward(G_ref)
    want = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    out = alg.policy_actions(torch.stack(alg.obs).flatten(0, 1), torch.stack(alg.eps).flatten(0, 1))
    out.backward(env.loss_action_grad().reshape(out.shape))
    assert want and "std" in want
    for n, p in model.named_parameters():
        if n in want:
            assert float((p.grad - want[n]).norm()) <= 1e-10 * float(want[n].norm()), n


def test_runner_two_iterations(tmp_path):
    torch.manual_seed(1)
    # episodes of 3 steps: every env finishes one inside the first window, so the Train/* keys are written
    env = OracleDiffVecEnv(num_envs=16, lag=1, t_max=4, dtype=torch.float32, episode_length_s=0.09)
    assert env.max_episode_length == 3
    cfg = QuadcopterDiffRLRunnerCfg(num_steps_per_env=4, max_iterations=2, save_interval=1, device="cpu", logger="csv",
                                    fused=False)
    cfg.policy.actor_hidden_dims = [32, 16]
    cfg.policy.critic_hidden_dims = [32, 16]
    runner = AlgoRunner(env, cfg.to_dict(), log_dir=str(tmp_path), device="cpu")
    model = runner.alg.actor_critic
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    lrs = []
    step = runner.alg.optimizer.step
    runner.alg.optimizer.step = lambda *a, **k: (lrs.append(runner.alg.optimizer.param_groups[0]["lr"]), step(*a, **k))[1]
    runner.learn(2, init_at_random_ep_len=True)
    for n, p in model.named_parameters():
        if n.startswith("actor") or n == "std":
            assert not torch.equal(p, before[n]), n
    eta_min, lr0 = 5e-4 * 0.01, 5e-4
    want = [eta_min + (lr0 - eta_min) * (1 + math.cos(math.pi * i / 2)) / 2 for i in range(2)]
    assert lrs == pytest.approx(want, rel=1e-12)
    text = (tmp_path / "scalars.csv").read_text()
    for key in ("Loss/policy", "Loss/learning_rate", "Policy/mean_noise_std", "Perf/total_fps", "Perf/collection_time",
                "Perf/learning_time", "Train/mean_loss,", "Train/mean_loss_detached,", "Train/mean_loss_total,"):
        assert key in text, key
    ck = torch.load(tmp_path / "model_1.pt", weights_only=True)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and ck["iter"] == 1
    other = AlgoRunner(OracleDiffVecEnv(num_envs=16, lag=1, t_max=4, dtype=torch.float32), cfg.to_dict(), None, "cpu")
    other.load(str(tmp_path / "model_1.pt"))
    for (n, p), (_, q) in zip(model.named_parameters(), other.alg.actor_critic.named_parameters()):
        assert torch.equal(p, q), n
    assert other.current_learning_iteration == 1
    assert runner.current_learning_iteration == 2  # a further learn() goes on from here


def test_unbuilt_options_raise(monkeypatch):
    env = OracleDiffVecEnv(num_envs=16, t_max=4, dtype=torch.float32)
    cfg = QuadcopterDiffRLRunnerCfg(device="cpu", empirical_normalization=True, fused=False)
    with pytest.raises(NotImplementedError):
        AlgoRunner(env, cfg.to_dict(), None, "cpu")
    cfg = QuadcopterDiffRLRunnerCfg(device="cpu", fused=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError):
        AlgoRunner(env, cfg.to_dict(), None, "cpu")
    monkeypatch.setenv("WORLD_SIZE", "1")
    AlgoRunner(env, cfg.to_dict(), None, "cpu")
    # one switch for the tape's path: a runner cfg that disagrees with the env's tape is refused
    with pytest.raises(ValueError, match="fused"):
        AlgoRunner(env, QuadcopterDiffRLRunnerCfg(device="cpu", fused=True).to_dict(), None, "cpu")
