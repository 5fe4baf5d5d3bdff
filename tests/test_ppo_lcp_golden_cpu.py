"""The build's PPOLCP (torch path) against the REFERENCE's own algorithm code (tests/golden/make_golden_ppo_lcp.py:
standalone/rsl_rl/ext/algorithms/ppo_lcp.py:105-206 with storage/rollout_storage.py).

Three iterations of rollout -> compute_returns -> update on make_golden_ppo.py's seeded synthetic rollouts with
grad_penalty_coef_schedule = [0.1, 1.0, 0, 2] (coefficients 0.1, 0.55, 1.0), replayed with the same torch generator
seeds.  Tolerances are test_ppo_golden_cpu.py's: the same fp32 torch ops in the same order on both sides, so the
storage and the parameters are held to rtol = atol = 1e-6, the mean losses (summed on the device in fp32 here, as
Python floats there) to 1e-5 relative.  Plain PPO on the same inputs must miss the fixture's parameters by more than
1e-3: the fixture sees the penalty."""
import os

import numpy as np
import pytest
import torch

from generalizableracing_amd.rsl_rl import ActorCritic
from generalizableracing_amd.rsl_rl.ppo import PPO
from generalizableracing_amd.rsl_rl.ppo_lcp import PPOLCP
from test_ppo_golden_cpu import HP, N, OBS, T, make_policy

ITERS = 3


@pytest.fixture(scope="module")
def gp():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ppo_lcp.npz")))


def rollout(alg, gp, it):
    x = {k: torch.from_numpy(gp[f"in_it{it}_{k}"]) for k in ("obs", "cobs", "rew", "dones", "tout", "last")}
    x["tout"] = x["tout"].bool()
    torch.manual_seed(100 + it)
    with torch.inference_mode():
        for t in range(T):
            alg.act(x["obs"][t], x["cobs"][t])
            alg.process_env_step(x["rew"][t], x["dones"][t], {"time_outs": x["tout"][t]})
        alg.compute_returns(x["last"])


def flat_params(alg):
    return torch.cat([p.detach().reshape(-1) for p in alg.policy.parameters()]).numpy()


def test_ppo_lcp_matches_reference(gp):
    pol = make_policy(ActorCritic)
    np.testing.assert_array_equal(torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).numpy(),
                                  gp["init_params"])
    alg = PPOLCP(pol, None, device="cpu", grad_penalty_coef_schedule=[float(v) for v in gp["schedule"]], **HP)
    alg.init_storage("rl", N, T, [OBS], [OBS], [4])
    for it in range(ITERS):
        rollout(alg, gp, it)
        st = alg.storage
        assert st.step == int(gp[f"lcp_it{it}_stored_steps"].item())
        for k in ("actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "returns", "advantages"):
            np.testing.assert_allclose(getattr(st, k).numpy(), gp[f"lcp_it{it}_{k}"], rtol=1e-6, atol=1e-6,
                                       err_msg=f"lcp it{it} {k}")
        torch.manual_seed(200 + it)
        losses = alg.update()
        assert sorted(losses) == ["grad_penalty", "gradient_penalty_coef", "surrogate", "value_function"]
        for k, v in losses.items():
            want = gp[f"lcp_it{it}_loss_{k}"].item()
            assert abs(v - want) <= 1e-5 * max(abs(want), 1e-3), (it, k, v, want)
        assert alg.learning_rate == pytest.approx(gp[f"lcp_it{it}_lr"].item(), rel=1e-12)
        np.testing.assert_allclose(flat_params(alg), gp[f"lcp_it{it}_params"], rtol=1e-6, atol=1e-6,
                                   err_msg=f"lcp it{it} params")
    assert alg.counter == ITERS and alg.fused_penalty_steps == 0
    assert [gp[f"lcp_it{it}_loss_gradient_penalty_coef"].item() for it in range(ITERS)] == pytest.approx([0.1, 0.55, 1.0])


def test_plain_ppo_misses_the_fixture(gp):
    """The same inputs without the penalty: after one update the parameters are more than 1e-3 from the fixture's."""
    alg = PPO(make_policy(ActorCritic), None, device="cpu", **HP)
    alg.init_storage("rl", N, T, [OBS], [OBS], [4])
    rollout(alg, gp, 0)
    torch.manual_seed(200)
    alg.update()
    assert float(np.abs(flat_params(alg) - gp["lcp_it0_params"]).max()) > 1e-3
