"""The masked-sequence form of the recurrent update against the REFERENCE's own recurrent generator and PPO
(tests/golden/golden_recurrent.npz, written by tests/golden/make_golden_recurrent.py from standalone/rsl_rl/ext/
storage/rollout_storage.py:193-254 and algorithms/ppo.py:103-190 over rsl-rl-lib 2.2's restated Memory).

The reference splits the rollout at every done, pads the trajectories and starts each from a saved hidden state; this
project runs the memories over the whole [T, B] block, masks the carried state with 1 - dones[t-1] and starts from the
state at rollout step 0.  Fed the same rollout, h0 and parameters in float64, it must give the same action means,
values and losses within 1e-10 and the same updated parameters within 1e-9: the test of that equivalence."""
import os

import numpy as np
import pytest
import torch

from generalizableracing_amd.rsl_rl import PPO, ActorCriticRecurrent

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_recurrent.npz")
T, N, OBS, R, K = 6, 8, 16, 16, 4
HP = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
          entropy_coef=0.005, learning_rate=5e-4, max_grad_norm=1.0, use_clipped_value_loss=True,
          schedule="adaptive", desired_kl=0.01)


@pytest.fixture(scope="module")
def gold():
    return {k: v for k, v in np.load(GOLD).items()}


@pytest.fixture()
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _setup(gold):
    pol = ActorCriticRecurrent(OBS, OBS, K, [16, 16], [16, 16], "lrelu", rnn_hidden_size=R)
    assert [n for n, _ in pol.named_parameters()] == [str(n) for n in gold["param_names"]]
    torch.nn.utils.vector_to_parameters(_t(gold["init_params"]), pol.parameters())
    alg = PPO(pol, device="cpu", storage_obs_dtype=torch.float64, **HP)
    alg.init_storage("rl", N, T, [OBS], [OBS], [K])
    st = alg.storage
    st.observations.copy_(_t(gold["in_obs"]))
    st.privileged_observations.copy_(_t(gold["in_cobs"]))
    st.dones.copy_(_t(gold["in_dones"]).unsqueeze(-1))
    for k in ("actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "returns", "advantages"):
        getattr(st, k).copy_(_t(gold[f"st_{k}"]))
    h0_a, h0_c = st.h0_buffers(R, R)
    h0_a.copy_(_t(gold["st_h0_a"]))
    h0_c.copy_(_t(gold["st_h0_c"]))
    st.step = T
    return pol, alg


def test_fixture_has_the_dones_pattern_and_only_step0_or_zero_trajectory_starts(gold):
    d = gold["in_dones"]
    per_env = d.sum(0)
    assert d.shape == (T, N) and per_env[0] == 0 and d[0, 1] == 1 and d[T - 1, 2] == 1 and per_env[3] == 2
    assert d[2, 4] == 1 and d[3, 4] == 1  # two consecutive dones
    assert np.abs(gold["st_h0_a"]).min() > 0  # the rollout starts from a non-zero state
    # every hidden state the reference starts a trajectory from is an env's step-0 state or zero
    for i in range(HP["num_mini_batches"]):
        for key, h0 in (("hid_a", gold["st_h0_a"]), ("hid_c", gold["st_h0_c"])):
            for row in gold[f"gen{i}_{key}"][0]:
                assert not row.any() or any(np.array_equal(row, r) for r in h0)
        assert gold[f"gen{i}_masks"].sum() == T * N // HP["num_mini_batches"]


def test_masked_sequence_gives_the_reference_means_and_values(gold, float64_default):
    pol, alg = _setup(gold)
    st = alg.storage
    with torch.no_grad():
        pol.act(st.observations, masks=st.dones[:, :, 0], hidden_states=st.h0_a.unsqueeze(0))
        mean = pol.action_mean.reshape(T, N, K)
        value = pol.evaluate(st.privileged_observations, masks=st.dones[:, :, 0],
                             hidden_states=st.h0_c.unsqueeze(0)).reshape(T, N, 1)
    e_mean = float((mean - _t(gold["ref_mean"])).abs().max())
    e_value = float((value - _t(gold["ref_value"])).abs().max())
    print(f"mean err {e_mean:.3e} value err {e_value:.3e}")
    assert e_mean <= 1e-10 and e_value <= 1e-10
    # the stored rollout's own means are the batch mode's (the parameters have not changed yet)
    assert float((mean - st.mu).abs().max()) <= 1e-10


def test_update_matches_the_reference(gold, float64_default):
    pol, alg = _setup(gold)
    torch.manual_seed(200)
    losses = alg.update()
    for k in ("value_function", "surrogate"):
        err = abs(losses[k] - float(gold[f"loss_{k}"].item()))
        print(f"loss {k}: {losses[k]:.12e} ref {float(gold[f'loss_{k}'].item()):.12e}")
        assert err <= 1e-10, (k, err)
    assert alg.learning_rate == pytest.approx(float(gold["lr"].item()), rel=1e-12)
    params = torch.nn.utils.parameters_to_vector(pol.parameters()).detach()
    err = float((params - _t(gold["params"])).abs().max())
    print(f"params max err {err:.3e}")
    assert err <= 1e-9
    assert alg.storage.step == 0
