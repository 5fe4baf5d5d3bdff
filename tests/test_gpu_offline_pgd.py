"""gr_offline_pgd_step (csrc/gr_offline.hip) through HeadFinetuner on the device.

Against the reference's own numbers (tests/golden/golden_offline.npz: its pgd_attack, BCEWithLogitsLoss and Adam on a
Linear(192, 1), five steps over a 37-row and a 256-row batch): x_adv bit for bit, the weights within 1e-6 (the
project's parameter bound for a graphed update against the eager one).  Against the float64 restatement of
tests/offline_ref.py fed the op's own x_adv: the loss and the gradients within 1e-5 of each tensor's norm (the bound
test_gpu_fused_mlp.py and test_gpu_lcp_kernels.py use for fp32 contractions of <= 256 terms and fixed-order row sums).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import offline_ref
from generalizableracing_amd.offline import HeadFinetuner, finetune

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
D = 192


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_offline.npz")))


def make_tuner(w, b, lr=3e-4, **kw):
    head = nn.Linear(len(w), 1)
    with torch.no_grad():
        head.weight.copy_(torch.as_tensor(w, dtype=torch.float32).reshape(1, -1))
        head.bias.fill_(float(b))
    tuner = HeadFinetuner(head, lr=lr, device=DEV, **kw)
    assert tuner.fused
    return tuner


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def step(tuner, x, y, index=None, **kw):
    """One fused step on dataset (x, y) -> (x_adv, the batch's mean loss)."""
    rows = len(index) if index is not None else len(x)
    x_adv = torch.full((rows, x.shape[1]), float("nan"), device=DEV)
    tuner.loss_acc.zero_()
    tuner.fused_step(dev(x, torch.float32), dev(y, torch.int8), None if index is None else dev(index, torch.int64),
                     x_adv=x_adv, **kw)
    return x_adv.cpu().numpy(), float(tuner.loss_acc.item()) / rows


def gradients(w, b, x, y, index=None):
    """[gw | gb] of a step read back through a zero-rate step from fresh Adam state: exp_avg = (1 - beta1) g."""
    probe = make_tuner(w, b, lr=0.0)
    step(probe, x, y, index)
    assert torch.equal(probe.wb.cpu(), torch.cat([torch.as_tensor(w, dtype=torch.float32), torch.tensor([float(b)])]))
    return probe.exp_avg.cpu().numpy().astype(np.float64) / float(np.float32(1.0 - 0.9))


def close(got, want, what):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    err, norm = np.linalg.norm(got - want), np.linalg.norm(want)
    print(f"{what}: |diff| {err:.3e}, |ref| {norm:.3e}, ratio {err / norm:.3e}")
    assert err <= 1e-5 * norm, what


def test_five_steps_reproduce_the_reference(gold):
    tuner = make_tuner(gold["w0"].reshape(-1), gold["b0"][0])
    calls = finetune.CALLS
    for s in range(5):
        name = "ab"[s % 2]
        x, y = gold[f"x_{name}"], gold[f"y_{name}"][:, 0]
        w, b = tuner.wb[:D].cpu().numpy(), float(tuner.wb[D])
        x_adv, loss = step(tuner, x, y)
        offline_ref.check_x_adv(gold, s, x_adv)
        ref_loss, gw, gb = offline_ref.loss_and_grads(x_adv, y, w, b)
        close(loss, ref_loss, f"step {s} loss")
        g = gradients(w, b, x, y)
        close(g[:D], gw, f"step {s} gw")
        close(g[D], gb, f"step {s} gb")
        dw = np.abs(tuner.wb[:D].cpu().numpy() - gold[f"s{s}_w"].reshape(-1)).max()
        db = abs(float(tuner.wb[D]) - float(gold[f"s{s}_b"][0]))
        print(f"step {s}: max |w - ref| {dw:.3e}, |b - ref| {db:.3e}, loss - ref {loss - float(gold[f's{s}_loss'][0]):.3e}")
        assert dw <= 1e-6 and db <= 1e-6
    assert finetune.CALLS - calls == 10 and float(tuner.step_count) == 5.0  # (5 steps and their 5 gradient probes)
    head = tuner.sync_head()
    assert torch.equal(head.weight.detach().reshape(-1), tuner.wb[:D]) and torch.equal(head.bias.detach(), tuner.wb[D:])


def problem(rows, seed, d=D, pool=1500):
    """A dataset of `pool` rows like the fixture's (features in [-0.2, 1.2], |w_j| in [0.005, 0.15] with three zeros, so
    |z| stays far below 12) and a gather index of `rows` entries (with repeats once rows > pool)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, (pool, d)).astype(np.float32)
    y = (rng.random(pool) < 0.4).astype(np.int8)
    w = (rng.uniform(0.005, 0.15, d) * rng.choice([-1.0, 1.0], d)).astype(np.float32)
    w[[0, d // 2, d - 1]] = 0.0
    index = rng.integers(0, pool, rows).astype(np.int64)
    return x, y, w, np.float32(-0.2), index


@pytest.mark.parametrize("rows", [1, 37, 256, 4109])
def test_gathered_batches(rows):
    """One step on a gathered batch: x_adv equals the restated attack bit for bit, the loss and gradients the float64
    restatement on that x_adv, the parameters Adam's first step in float64."""
    x, y, w, b, index = problem(rows, rows)
    if rows == 4109:
        assert len(np.unique(index)) < rows
    tuner = make_tuner(w, b)
    x_adv, loss = step(tuner, x, y, index)
    xg, yg = x[index], y[index].astype(np.float64)
    assert np.array_equal(x_adv.view(np.uint32), offline_ref.pgd(xg, yg, w, b, 0.1, 0.01, 3).view(np.uint32))
    ref_loss, gw, gb = offline_ref.loss_and_grads(x_adv, yg, w, b)
    close(loss, ref_loss, "loss")
    g = gradients(w, b, x, y, index)
    close(g[:D], gw, "gw")
    close(g[D], gb, "gb")
    p, _, _ = offline_ref.adam_step(np.append(w, b).astype(np.float64), np.append(gw, gb), np.zeros(D + 1),
                                    np.zeros(D + 1), 1)
    assert np.abs(tuner.wb.cpu().numpy() - p).max() <= 1e-6


@pytest.mark.parametrize("d", [5, 64, 65, 300, 1024])
def test_other_widths(d):
    """Every column-tile count of the row kernel (d = 5 .. 1024), not only the product's 192."""
    rows = 70
    x, y, w, b, index = problem(rows, d, d=d, pool=90)
    w = (w * min(1.0, 192.0 / d)).astype(np.float32)  # (keeps |z| small at the wide sizes)
    tuner = make_tuner(w, b)
    x_adv, loss = step(tuner, x, y, index)
    xg, yg = x[index], y[index].astype(np.float64)
    assert np.array_equal(x_adv.view(np.uint32), offline_ref.pgd(xg, yg, w, b, 0.1, 0.01, 3).view(np.uint32))
    ref_loss, gw, gb = offline_ref.loss_and_grads(x_adv, yg, w, b)
    close(loss, ref_loss, "loss")
    p, _, _ = offline_ref.adam_step(np.append(w, b).astype(np.float64), np.append(gw, gb), np.zeros(d + 1),
                                    np.zeros(d + 1), 1)
    assert np.abs(tuner.wb.cpu().numpy() - p).max() <= 1e-6


def test_no_iterations_only_clamps(gold):
    x, y = gold["x_b"], gold["y_b"][:, 0]
    tuner = make_tuner(gold["w0"].reshape(-1), gold["b0"][0])
    x_adv, loss = step(tuner, x, y, num_iters=0)
    assert np.array_equal(x_adv, np.clip(x, 0.0, 1.0))
    close(loss, offline_ref.loss_and_grads(x_adv, y, gold["w0"].reshape(-1), gold["b0"][0])[0], "loss")


def test_two_runs_are_bit_identical():
    x, y, w, b, index = problem(4109, 11)
    outs = []
    for _ in range(2):
        tuner = make_tuner(w, b)
        x_adv, loss = step(tuner, x, y, index)
        x_adv2, loss2 = step(tuner, x, y, index[:300])
        outs.append((x_adv, loss, x_adv2, loss2, tuner.wb.cpu().numpy(), tuner.exp_avg.cpu().numpy(),
                     tuner.exp_avg_sq.cpu().numpy()))
    for a, c in zip(*outs):
        assert np.array_equal(np.asarray(a), np.asarray(c))


def test_epoch_accumulates_the_batch_losses():
    """HeadFinetuner.epoch over 1000 rows in batches of 256 (the last of 232): its mean is the loss accumulator over
    the rows, and the accumulator is the sum, in order, of what each batch adds (loss * rows)."""
    x, y, w, b, _ = problem(1, 3, pool=1000)
    data = (dev(x, torch.float32), dev(y, torch.int8))
    tuner = make_tuner(w, b)
    mean = tuner.epoch(data, 256, torch.Generator(device=DEV).manual_seed(5))
    assert tuner.steps == 4 and float(tuner.step_count) == 4.0
    total = float(tuner.loss_acc.item())
    assert mean == total / 1000
    again = make_tuner(w, b)
    perm = torch.randperm(1000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    parts = []
    for start in range(0, 1000, 256):
        again.loss_acc.zero_()
        again.fused_step(*data, perm[start:start + 256])
        parts.append(float(again.loss_acc.item()))
    acc = 0.0
    for v in parts:
        acc += v
    assert acc == total and torch.equal(again.wb, tuner.wb)
    assert torch.equal(tuner.head.weight.detach().reshape(-1), tuner.wb[:D])
    # the eager loop on the same shuffles lands on the same head within the parameter bound
    head = nn.Linear(D, 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(w).reshape(1, -1))
        head.bias.fill_(float(b))
    eager = HeadFinetuner(head, device=DEV, fused=False)
    mean_eager = eager.epoch(data, 256, torch.Generator(device=DEV).manual_seed(5))
    print(f"epoch mean loss: fused {mean:.7f}, eager {mean_eager:.7f}")
    assert abs(mean - mean_eager) <= 1e-5 * abs(mean_eager)
    assert float((eager.head.weight.detach().reshape(-1) - tuner.wb[:D]).abs().max()) <= 1e-6
