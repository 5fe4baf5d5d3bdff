"""VisionActorCriticRecurrent on the CPU in float64: against the REFERENCE's own class, recurrent generator and PPO
(tests/golden/golden_vision_recurrent.npz, written by tests/golden/make_golden_vision_recurrent.py), and against
itself (rollout mode versus batch mode, the feature path, the state dict, the gradients that reach the stem through the
memories, the registry, the TorchScript export).

The reference pads the trajectories and runs the stem over the padded block; this project runs the stem over the
T * B real rows and the memories over the masked block.  In eval mode (recording a, the full dones pattern) and in
train mode with no done inside the rollout (recording b) the two agree: 1e-9 relative."""
import os

import numpy as np
import pytest
import torch

import vision_recurrent_golden as vg
from generalizableracing_amd.registry import load_cfg_from_registry
from generalizableracing_amd.rsl_rl import PPO, PPOL2C2, VisionActorCritic, VisionActorCriticRecurrent, exporter
from generalizableracing_amd.rsl_rl.on_policy_runner import POLICIES

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_vision_recurrent.npz")
T, N, K, R = vg.T, vg.N, vg.K, vg.R
STORED = ("actions", "values", "actions_log_prob", "mu", "sigma", "rewards", "returns", "advantages")


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


def _rel(got, ref):
    got, ref = got.detach(), ref.detach()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def _policy(seed=0, **kw):
    torch.manual_seed(seed)
    pol = VisionActorCriticRecurrent(vg.OBS, vg.OBS, K, **{**vg.policy_kwargs(), **kw})
    vg.randomise_batchnorms(pol, torch.Generator().manual_seed(seed + 1))
    return pol


def _state(gold, prefix):
    return {k[len(prefix) + 1:]: _t(v) for k, v in gold.items() if k.startswith(prefix + ":")}


def _setup(gold, tag, seed, dones_list):
    """The policy with the fixture's initial state and a PPO whose storage holds the fixture's rollout; the
    observation rows are regenerated from the seed and checked against the stored checksum."""
    pol = VisionActorCriticRecurrent(vg.OBS, vg.OBS, K, **vg.policy_kwargs())
    sd0 = _state(gold, "sd0")
    assert set(sd0) == set(pol.state_dict())
    pol.load_state_dict(sd0)
    alg = PPO(pol, device="cpu", storage_obs_dtype=torch.float64, **vg.HP)
    alg.init_storage("rl", N, T, [vg.OBS], [vg.OBS], [K])
    obs, cobs, _, dones, _, _, _ = vg.inputs(seed, dones_list)
    # (sums of ~1e5 float64 terms: their order differs between machines, the terms do not)
    assert _rel(vg.checksum(obs, cobs), _t(gold[f"{tag}_checksum"])) <= 1e-13
    assert torch.equal(dones, _t(gold[f"{tag}_dones"]))
    st = alg.storage
    st.observations.copy_(obs)
    st.privileged_observations.copy_(cobs)
    st.dones.copy_(dones.unsqueeze(-1))
    for k in STORED:
        getattr(st, k).copy_(_t(gold[f"{tag}_st_{k}"]))
    h0_a, h0_c = st.h0_buffers(R, R)
    h0_a.copy_(_t(gold[f"{tag}_h0_a"]))
    h0_c.copy_(_t(gold[f"{tag}_h0_c"]))
    st.step = T
    return pol, alg


def _batch_outputs(pol, st, mini_batches):
    """As the fixture: per mini-batch, act on the block, then evaluate on it."""
    mean, value = torch.zeros(T, N, K), torch.zeros(T, N, 1)
    size = N // mini_batches
    with torch.no_grad():
        for i, b in enumerate(st.recurrent_mini_batch_generator(mini_batches, 1)):
            assert not b[0].is_contiguous()  # a block of the storage: read through row indices
            pol.act(b[0], masks=b[10], hidden_states=b[9][0])
            mean[:, i * size:(i + 1) * size] = pol.action_mean.reshape(T, size, K)
            value[:, i * size:(i + 1) * size] = pol.evaluate(b[1], masks=b[10],
                                                              hidden_states=b[9][1]).reshape(T, size, 1)
    return mean, value


def test_eval_mode_batch_outputs_match_the_reference_over_the_full_dones_pattern(gold, float64_default):
    pol, alg = _setup(gold, "a", vg.SEED_A, vg.DONES)
    pol.eval()
    st = alg.storage
    assert int(st.dones.sum()) == len(vg.DONES)
    # the whole [T, N] block with masks = dones ...
    with torch.no_grad():
        pol.act(st.observations, masks=st.dones[:, :, 0], hidden_states=st.h0_a.unsqueeze(0))
        mean = pol.action_mean.reshape(T, N, K)
        value = pol.evaluate(st.privileged_observations, masks=st.dones[:, :, 0],
                             hidden_states=st.h0_c.unsqueeze(0)).reshape(T, N, 1)
    e_mean, e_value = _rel(mean, _t(gold["a_mean"])), _rel(value, _t(gold["a_value"]))
    print(f"(a) whole block: mean {e_mean:.3e} value {e_value:.3e}")
    assert e_mean <= 1e-9 and e_value <= 1e-9
    # ... and per mini-batch block of the storage
    mean, value = _batch_outputs(pol, st, vg.HP["num_mini_batches"])
    assert _rel(mean, _t(gold["a_mean"])) <= 1e-9 and _rel(value, _t(gold["a_value"])) <= 1e-9
    assert _rel(mean, st.mu) <= 1e-9  # the rollout's own means (the parameters have not changed)


def test_train_mode_outputs_and_update_match_the_reference(gold, float64_default):
    pol, alg = _setup(gold, "b", vg.SEED_B, [])
    pol.load_state_dict({**pol.state_dict(), **_state(gold, "sdb_rollout")})  # the statistics after the rollout
    pol.train()
    mean, value = _batch_outputs(pol, alg.storage, vg.HP["num_mini_batches"])
    e_mean, e_value = _rel(mean, _t(gold["b_mean"])), _rel(value, _t(gold["b_value"]))
    print(f"(b) mean {e_mean:.3e} value {e_value:.3e}")
    assert e_mean <= 1e-9 and e_value <= 1e-9
    sd = pol.state_dict()
    for k, v in _state(gold, "sdb_batch").items():  # two forwards per mini-batch moved the running statistics
        assert _rel(sd[k].double(), v.double()) <= 1e-9, k
    torch.manual_seed(200)
    losses = alg.update()
    for k in ("value_function", "surrogate"):
        ref = float(gold[f"b_loss_{k}"].item())
        print(f"loss {k}: {losses[k]:.12e} ref {ref:.12e}")
        assert abs(losses[k] - ref) <= 1e-9 * max(abs(ref), 1e-3), k
    assert alg.learning_rate == pytest.approx(float(gold["b_lr"].item()), rel=1e-12)
    sd, ref_sd = pol.state_dict(), _state(gold, "sdb_update")
    assert set(sd) == set(ref_sd)
    worst = max((_rel(sd[k].double(), v.double()), k) for k, v in ref_sd.items())
    print(f"parameters and running statistics after the update: worst {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= 1e-9, worst
    assert not torch.equal(sd["stem.0.weight"], _state(gold, "sd0")["stem.0.weight"])  # the stem trained
    assert alg.storage.step == 0


def test_rollout_mode_stepped_with_resets_equals_batch_mode(float64_default):
    """Eval mode: in train mode the BatchNorms normalise a rollout step over its N rows and a block over its T * N
    rows, so the two modes differ there by construction (as in the reference)."""
    pol = _policy(seed=3).eval()
    obs, cobs, _, dones, _, _, warm = vg.inputs(21, vg.DONES)
    with torch.no_grad():
        pol.act(warm[0])
        pol.evaluate(warm[1])
        h0 = [h.clone() for h in pol.get_hidden_states()]
        means, values = [], []
        for t in range(T):
            pol.update_distribution(obs[t])
            means.append(pol.action_mean)
            values.append(pol.evaluate(cobs[t]))
            pol.reset(dones[t])
        pol.update_distribution(obs, masks=dones, hidden_states=h0[0])
        value = pol.evaluate(cobs, masks=dones, hidden_states=h0[1])
    assert _rel(pol.action_mean.reshape(T, N, K), torch.stack(means)) <= 1e-12
    assert _rel(value.reshape(T, N, 1), torch.stack(values)) <= 1e-12


def test_train_mode_block_is_normalised_over_its_real_rows(float64_default):
    """The documented deviation: the batch statistics of a block are those of its T * B rows, no padding image."""
    pol = _policy(seed=3).train()
    obs = vg.inputs(21, vg.DONES)[0]
    with torch.no_grad():
        a = pol.encode(obs)
        b = pol.features(obs.reshape(T * N, -1)).view(T, N, -1)
    assert _rel(a, b) <= 1e-12


def test_feature_path_is_vision_actor_critics(float64_default):
    pol = _policy(seed=4)
    kw = vg.policy_kwargs()
    ff = VisionActorCritic(vg.OBS, vg.OBS, K, img_res=kw["img_res"], dim_hidden_input=vg.DIM,
                           actor_hidden_dims=vg.HEADS, critic_hidden_dims=vg.HEADS, activation="lrelu")
    ff.stem.load_state_dict(pol.stem.state_dict())
    ff.state_enc.load_state_dict(pol.state_enc.state_dict())
    obs = vg.rows(torch.Generator().manual_seed(2), 5)
    for training in (False, True):
        pol.train(training), ff.train(training)
        with torch.no_grad():
            assert torch.equal(pol.features(obs), ff.features(obs))
    # a strided block of a wider buffer goes through row indices and gives the gathered rows' feature
    buf = vg.rows(torch.Generator().manual_seed(3), 3, 6)
    block = buf[:, 1:4]
    flat, rows = pol._block_rows(block)
    assert rows is not None and torch.equal(flat[rows], block.reshape(9, -1))
    pol.eval()
    with torch.no_grad():
        assert _rel(pol.encode(block), pol.features(block.reshape(9, -1)).view(3, 3, -1)) <= 1e-12
    assert VisionActorCriticRecurrent.fused_bn and pol.is_recurrent and not ff.is_recurrent


def test_one_shared_buffer_stands_for_the_actors_and_the_critics_stem_pass(float64_default):
    obs = vg.rows(torch.Generator().manual_seed(6), 3, 4)
    one, two = _policy(seed=5).train(), _policy(seed=5).train()
    a1, c1 = one.memory_inputs(obs, obs)
    a2, c2 = two.memory_inputs(obs, obs.clone())
    assert a1 is c1 and a2 is not c2
    assert _rel(a1, a2) <= 1e-12 and _rel(c1, c2) <= 1e-12
    for (k, v), w in zip(one.state_dict().items(), two.state_dict().values()):
        assert _rel(v.double(), w.double()) <= 1e-12, k  # both updated every running statistic twice
    assert int(one.stem[1].num_batches_tracked) == 2


def test_state_dict_keys_are_the_references():
    pol = _policy()
    gru = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    want = {f"{m}.rnn.{g}" for m in ("memory_a", "memory_c") for g in gru} | {"std"}
    want |= {f"{net}.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4) for p in ("weight", "bias")}
    want |= {"state_enc.weight", "state_enc.bias", "stem.0.weight", "stem.3.weight", "stem.6.weight",
             "stem.10.weight", "stem.10.bias"}
    want |= {f"stem.{i}.{p}" for i in (1, 4, 7)
             for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(pol.state_dict()) == want
    assert "log_std" in _policy(noise_std_type="log").state_dict()
    assert pol.actor[0].in_features == R and pol.memory_a.rnn.input_size == vg.DIM


def test_gradients_reach_the_stem_and_the_state_encoder_and_match_finite_differences(float64_default):
    pol = _policy(seed=7).train()
    g = torch.Generator().manual_seed(8)
    Tn, Bn = 4, 3
    obs, cobs = vg.rows(g, Tn, Bn), vg.rows(g, Tn, Bn)
    dones = torch.zeros(Tn, Bn, dtype=torch.long)
    dones[1, 1] = 1
    h0 = torch.randn(2, 1, Bn, R, generator=g)
    gm, gv = torch.randn(Tn * Bn, K, generator=g), torch.randn(Tn * Bn, 1, generator=g)

    def loss():
        pol.update_distribution(obs, masks=dones, hidden_states=h0[0])
        return (pol.action_mean * gm).sum() + (pol.evaluate(cobs, masks=dones, hidden_states=h0[1]) * gv).sum()

    loss().backward()
    for p in (pol.stem[0].weight, pol.state_enc.weight):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
        flat, grad = p.data.view(-1), p.grad.view(-1)
        for i in (0, flat.numel() // 2, flat.numel() - 1):
            old, eps = float(flat[i]), 1e-6
            with torch.no_grad():
                flat[i] = old + eps
                up = float(loss())
                flat[i] = old - eps
                dn = float(loss())
                flat[i] = old
            fd = (up - dn) / (2 * eps)
            assert abs(fd - float(grad[i])) <= 1e-6 * max(abs(fd), abs(float(grad[i]))), (i, fd, float(grad[i]))


def test_registry_config_and_runner_table_resolve_on_both_vision_ids():
    for task in ("DiffLab-Quadcopter-CTBR-Racing-v0", "DiffLab-Quadcopter-CTBR-Racing-Vision-v0"):
        cfg = load_cfg_from_registry(task, "rsl_rl_recurrent_cfg_entry_point").to_dict()
        pol, alg = cfg["policy"], cfg["algorithm"]
        assert cfg["experiment_name"] == "racing_ppo_vision_recurrent" and alg["class_name"] == "PPO"
        ref_alg = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point").to_dict()["algorithm"]
        assert {**ref_alg, "class_name": "PPO"} == alg  # QuadcopterVisionPPORunnerCfg's algorithm block
        assert (pol["class_name"], pol["rnn_type"], pol["rnn_hidden_size"], pol["rnn_num_layers"]) == (
            "VisionActorCriticRecurrent", "gru", 192, 1)
        assert pol["dim_hidden_input"] == 192 and tuple(pol["img_res"]) == (72, 96) and pol["activation"] == "lrelu"
        assert pol["actor_hidden_dims"] == [128, 128] and pol["critic_hidden_dims"] == [128, 128]
        assert pol["init_noise_std"] == 1.0 and pol["noise_std_type"] == "scalar"
    assert POLICIES["VisionActorCriticRecurrent"] is VisionActorCriticRecurrent
    kw = {k: v for k, v in pol.items() if k != "class_name"}
    built = POLICIES[pol["class_name"]](vg.OBS, vg.OBS, 4, **kw)
    assert built.memory_a.rnn.input_size == 192 and built.actor[0].in_features == 192


def test_unsupported_combinations_raise():
    for kw in (dict(rnn_type="lstm"), dict(rnn_num_layers=2)):
        with pytest.raises(NotImplementedError, match="gru"):
            _policy(**kw)
    with pytest.raises(ValueError, match="recurrent"):
        PPOL2C2(_policy(), device="cpu")
    for kw in (dict(graph_update=True), dict(fused_rollout_inference=True), dict(update_autocast_bf16=True)):
        with pytest.raises(ValueError, match="recurrent"):
            PPO(_policy(), device="cpu", **kw)
    with pytest.raises(RuntimeError, match="recurrent"):
        exporter.export_policy_as_onnx(_policy(), "unused")


def test_torchscript_export_reproduces_act_inference_over_steps_with_a_reset(tmp_path):
    pol = _policy(seed=9).float().eval()
    path = exporter.export_policy_as_jit(pol, None, str(tmp_path), "policy.pt")
    m = torch.jit.load(path)
    n = 3
    h = torch.zeros(1, n, R)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for step in range(5):
            x = vg.rows(g, n).float()
            want = pol.act_inference(x)
            assert not isinstance(want, tuple) and want.shape == (n, K)  # the mean alone: no feature
            got, h = m(x, h)
            assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
            if step == 2:  # env 1 finishes: the caller zeroes its row, the policy resets it
                d = torch.tensor([0, 1, 0])
                pol.reset(d)
                h[0, 1] = 0.0
            assert float((h - pol.get_hidden_states()[0]).abs().max()) <= 1e-6
