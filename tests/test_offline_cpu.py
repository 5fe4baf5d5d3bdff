"""The offline auxiliary-head stage on the CPU: the eager attack and fine-tune loop against the reference's own numbers
(tests/golden/golden_offline.npz, make_golden_offline.py), the collector's torch selection against the numpy loop of
tests/offline_ref.py, the dataset files, the trainer command line and the argument checks of the two entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import offline_ref
from generalizableracing_amd import _abi
from generalizableracing_amd.offline import FeatureCollector, HeadFinetuner, pgd_attack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_offline.npz")))


def _head(gold):
    head = nn.Linear(192, 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(gold["w0"]))
        head.bias.copy_(torch.from_numpy(gold["b0"]))
    return head


check_x_adv = offline_ref.check_x_adv


def test_fixture_meets_its_conditions(gold):
    w0 = gold["w0"].reshape(-1)
    assert int((w0 == 0).sum()) == 3 and np.abs(w0[w0 != 0]).min() >= 1e-3
    for name, rows in (("a", 37), ("b", 256)):
        x, y = gold[f"x_{name}"], gold[f"y_{name}"]
        assert x.shape == (rows, 192) and x.min() < 0 and x.max() > 1 and 0 < y.sum() < rows


def test_eager_finetune_reproduces_the_reference(gold):
    """pgd_attack's x_adv bit for bit (fp32 add, sub and clamp only); the loss and the head after each of the five Adam
    steps within 1e-6 (the same torch, the same order)."""
    tuner = HeadFinetuner(_head(gold), lr=3e-4, device="cpu")
    assert not tuner.fused
    for s in range(STEPS):
        name = "ab"[s % 2]
        x, y = torch.from_numpy(gold[f"x_{name}"]), torch.from_numpy(gold[f"y_{name}"])
        x_adv, pert = pgd_attack(tuner.head, tuner.criterion, x, y, 0.1, 0.01, 3)
        check_x_adv(gold, s, x_adv.numpy())
        assert float(pert.abs().max()) <= float(np.float32(0.1))
        loss = tuner.eager_step(x, y)
        assert abs(float(loss) - float(gold[f"s{s}_loss"][0])) <= 1e-6
        assert np.abs(tuner.head.weight.detach().numpy() - gold[f"s{s}_w"]).max() <= 1e-6
        assert np.abs(tuner.head.bias.detach().numpy() - gold[f"s{s}_b"]).max() <= 1e-6


def test_restatement_agrees_with_the_reference(gold):
    """tests/offline_ref.py (what the GPU tests compare against) on the fixture: the attack bit for bit, the float64
    loss and Adam steps within 1e-6 of the reference's fp32 numbers."""
    w, b = gold["w0"].reshape(-1).astype(np.float64), float(gold["b0"][0])
    m, v = np.zeros(193), np.zeros(193)
    for s in range(STEPS):
        name = "ab"[s % 2]
        x, y = gold[f"x_{name}"], gold[f"y_{name}"][:, 0]
        x_adv = offline_ref.pgd(x, y, w, b, 0.1, 0.01, 3)
        check_x_adv(gold, s, x_adv)
        loss, gw, gb = offline_ref.loss_and_grads(x_adv, y, w, b)
        assert abs(loss - float(gold[f"s{s}_loss"][0])) <= 1e-6
        p, m, v = offline_ref.adam_step(np.append(w, b), np.append(gw, gb), m, v, s + 1)
        w, b = p[:192], p[192]
        assert np.abs(w - gold[f"s{s}_w"].reshape(-1)).max() <= 1e-6 and abs(b - gold[f"s{s}_b"][0]) <= 1e-6
    assert np.array_equal(offline_ref.pgd(x, y, w, b, 0.1, 0.01, 0), np.clip(x, 0, 1))


def collector_sequence(seed, steps, n, d, capacity):
    """`steps` env steps of (feat [n, d], aux [n]) that cross every branch of the selection: no positive, all positive,
    one positive at the last row, ~3 % positives, more positives than negatives; labels 1.0 (and one 2.0)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(steps):
        kind = t % 5
        if kind == 0:
            aux = np.zeros(n, np.float32)
        elif kind == 1:
            aux = (rng.random(n) < 0.03).astype(np.float32)
        elif kind == 2:
            aux = np.zeros(n, np.float32)
            aux[-1] = 2.0
        elif kind == 3:
            aux = (rng.random(n) < 0.7).astype(np.float32)
        else:
            aux = np.ones(n, np.float32)
        out.append((rng.standard_normal((n, d)).astype(np.float32), aux))
    return out


def test_collector_cpu_matches_the_reference_loop(tmp_path):
    """40 random steps: the dataset and the cursor after every step equal the numpy loop's, through cuts inside the
    positives and the negatives and calls on a full dataset; then the files round-trip."""
    n, d, cap = 50, 5, 700
    col, ref = FeatureCollector(cap, d, "cpu"), offline_ref.Collector(cap, d)
    cuts = set()
    for feat, aux in collector_sequence(3, 40, n, d, cap):
        before = ref.w
        kept = ref.add(feat, aux)
        col.add(torch.from_numpy(feat), torch.from_numpy(aux).reshape(n, 1))
        assert col.counts() == ref.cursor()
        npos = int((aux != 0).sum())
        if kept[0] < npos:
            cuts.add("positives" if before < cap else "full")
        elif kept[1] < min(npos, n - npos):
            cuts.add("negatives")
        if before == cap and npos:
            cuts.add("full")
    assert ref.w == cap and {"full"} <= cuts and cuts & {"positives", "negatives"}
    assert np.array_equal(col.features.numpy().view(np.uint32), ref.features.view(np.uint32))
    assert np.array_equal(col.supervision.numpy(), ref.supervision)
    # a half-filled dataset: only the rows written go to the files
    half = FeatureCollector(cap, d, "cpu")
    half.add(torch.from_numpy(feat), torch.from_numpy(np.ones(n, np.float32)))
    path = half.save(str(tmp_path / "data"))
    feats, sup = FeatureCollector.read(path)
    assert isinstance(feats, np.memmap) and feats.shape == (n, d) and sup.shape == (n, 1) and sup.dtype == np.int8
    back = FeatureCollector.load(path, "cpu", capacity=cap)
    assert back.counts() == half.counts() == (n, n, 0)
    assert torch.equal(back.features, half.features) and torch.equal(back.supervision, half.supervision)


@pytest.mark.parametrize("cap", [50, 60, 70])
def test_collector_cpu_capacity_cuts(cap):
    """20 positives and 20 negatives a step, 40 rows written by the first: the second step's cut falls inside the
    positives (capacity 50), exactly at w + |P| == capacity (60), inside the negatives (70); two more calls on the full
    dataset change nothing."""
    n, d = 40, 3
    aux = np.zeros(n, np.float32)
    aux[::2] = 1.0
    rng = np.random.default_rng(0)
    col, ref = FeatureCollector(cap, d, "cpu"), offline_ref.Collector(cap, d)
    for _ in range(4):
        feat = rng.standard_normal((n, d)).astype(np.float32)
        ref.add(feat, aux)
        col.add(torch.from_numpy(feat), torch.from_numpy(aux))
    assert col.counts() == ref.cursor() == (cap, min(cap - 20, 40), max(20, cap - 40))
    assert np.array_equal(col.features.numpy(), ref.features) and np.array_equal(col.supervision.numpy(), ref.supervision)


def _load_cli(name):
    spec = importlib.util.spec_from_file_location(f"offline_cli_{name}", os.path.join(ROOT, "standalone", "offline",
                                                                                      f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_cli_changes_only_the_head(tmp_path):
    """The trainer command line on a synthetic dataset and a runner.save-shaped checkpoint of the registered vision
    recipe: two epoch files, only aux_decoder.* differs from the input, and the policy loads the result."""
    from generalizableracing_amd.rsl_rl import VisionActorCritic

    torch.manual_seed(0)
    pol = VisionActorCritic(6928, 6928, 4, img_res=(72, 96), dim_hidden_input=192, actor_hidden_dims=[128, 128],
                            critic_hidden_dims=[128, 128], activation="lrelu", use_auxiliary_loss=True)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    ckpt = {"model_state_dict": pol.state_dict(), "optimizer_state_dict": opt.state_dict(), "iter": 7, "infos": None}
    torch.save(ckpt, tmp_path / "model_7.pt")
    rng = np.random.default_rng(1)
    col = FeatureCollector(600, 192, "cpu")
    for _ in range(3):
        col.add(torch.from_numpy(rng.random((200, 192)).astype(np.float32)),
                torch.from_numpy((rng.random(200) < 0.5).astype(np.float32)))
    rows = col.count()
    assert 300 < rows <= 600
    col.save(str(tmp_path / "data"))
    cli = _load_cli("train")
    out = cli.main(["--h5_path", str(tmp_path / "data"), "--policy_path", str(tmp_path / "model_7.pt"), "--save_path",
                    str(tmp_path / "out"), "--epochs", "2", "--batch_size", "128", "--device", "cpu"])
    assert out["rows"] == rows and not out["fused"] and out["steps"] == 2 * -(-rows // 128)
    assert all(np.isfinite(out["losses"])) and out["losses"][1] < out["losses"][0]
    before = ckpt["model_state_dict"]
    for e in range(2):
        new = torch.load(tmp_path / "out" / f"policy_finetune_epoch-{e}.pt", weights_only=True)
        assert new["iter"] == 7 and new["infos"] is None and set(new) == set(ckpt)
        assert set(new["model_state_dict"]) == set(before)
        for k, v in new["model_state_dict"].items():
            assert torch.equal(v, before[k]) != k.startswith("aux_decoder."), k
        assert str(new["optimizer_state_dict"]) == str(ckpt["optimizer_state_dict"])
    pol.load_state_dict(new["model_state_dict"])


def test_runner_has_get_decoder():
    from generalizableracing_amd.rsl_rl import OnPolicyRunner

    assert callable(OnPolicyRunner.get_decoder)


def test_entry_points_reject_bad_arguments():
    """gr_offline_collect / gr_offline_pgd_step: argument errors before any launch (no device needed)."""
    lib = _abi.load()
    p = 0x10000

    def collect(feat=p, ld=192, ld_aux=1, n=64, d=192, cap=1000, cursor=p):
        return lib.gr_offline_collect(feat, ld, p, ld_aux, n, d, p, p, cap, cursor, p, None)

    assert collect(d=0) == -1 and collect(n=-1) == -1 and collect(ld=100) == -1 and collect(ld_aux=0) == -1
    assert collect(cap=0) == -1 and collect(feat=None) == -1 and collect(cursor=None) == -1 and collect(n=2 ** 31) == -1
    assert collect(n=0) == 0  # nothing to do, nothing launched
    assert lib.gr_offline_scratch_ints(4096) >= 4096 and lib.gr_offline_scratch_ints(-1) == -1

    def pgd(rows=256, d=192, iters=3, wb=p, partial=p, loss=p):
        return lib.gr_offline_pgd_step(p, p, None, rows, d, wb, p, p, p, 0.1, 0.01, iters, 3e-4, 0.9, 0.999, 1e-8,
                                       partial, loss, None, None)

    assert pgd(rows=0) == -1 and pgd(d=0) == -1 and pgd(d=1025) == -1 and pgd(iters=-1) == -1
    assert pgd(wb=None) == -1 and pgd(partial=None) == -1 and pgd(loss=None) == -1 and pgd(rows=2 ** 31) == -1
    assert lib.gr_offline_pgd_partials(0, 192) == -1 and lib.gr_offline_pgd_partials(256, 0) == -1
    assert lib.gr_offline_pgd_partials(256, 192) == 64 * 196 and lib.gr_offline_pgd_partials(10 ** 6, 192) == 256 * 196
