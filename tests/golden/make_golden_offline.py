"""Golden vectors for the offline auxiliary-head fine-tune, produced by the REFERENCE's own pgd_attack.

Run in the development container (the reference tree is read in place; it never travels to the GPU box):

    python tests/golden/make_golden_offline.py

Loads standalone/offline/train.py by path with stand-ins in sys.modules for the two modules it imports that are not
installed here (h5py, tqdm: neither is used on this path) and runs, on the CPU in fp32, what its finetune_policy_head
runs per mini-batch (train.py:105-112): pgd_attack(epsilon 0.1, alpha 0.01, 3 iterations) under BCEWithLogitsLoss on
its HeadOnlyPolicy over a Linear(192, 1), the loss on the attacked features, Adam(lr 3e-4).  Five steps over two
mini-batches, a of 37 rows and b of 256: a b a b a.

Recorded: the inputs (features on the 1/256 grid in [-0.2, 1.2], which compresses; labels; the initial weight and
bias), and per step the loss, the weight and bias after the step, the SHA-256 of x_adv's bytes and each row's float64
sum of x_adv (to place a mismatch); x_adv itself for steps 0 and 2 in full and for step 1 as its first 32 rows (every
x_adv in full would put the file past the 200 kB it may take).

Asserted here, so the fixture pins what it is meant to: every logit the attack and the loss see has |z| <= 12
(sigmoid(z) - y is then never 0 in fp32, so the step direction is the label's); the initial weight has three exact
zeros (sign(0) = 0) and |w_j| >= 1e-3 elsewhere, and no weight comes within 1e-5 of zero after a step (a sign that a
1e-6 difference could turn); features below 0 and above 1 exist (the [0, 1] clamp acts); both labels occur in both
batches.
"""
from __future__ import annotations

import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import il_shim  # noqa: E402

OUT = os.path.join(HERE, "golden_offline.npz")
D = 192
ROWS = (37, 256)
STEPS = 5
EPSILON, ALPHA, ITERS, LR = 0.1, 0.01, 3, 3e-4
FULL_X_ADV = {0: None, 1: 32, 2: None}  # step -> rows of x_adv kept in full (None: all)


def load_reference():
    for name in ("h5py", "tqdm"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = lambda it, **kw: it
    return il_shim.load("grref_offline_train", os.path.join(il_shim.REF, "standalone/offline/train.py"))


def inputs():
    g = torch.Generator().manual_seed(20)
    out = {}
    for name, rows in zip("ab", ROWS):
        out[f"x_{name}"] = torch.randint(-51, 308, (rows, D), generator=g).float() / 256.0
        out[f"y_{name}"] = (torch.rand(rows, 1, generator=g) < 0.4).float()
    mag = 0.005 + 0.145 * torch.rand(D, generator=g)
    w = mag * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    w[[5, 77, 191]] = 0.0
    out["w0"] = w.reshape(1, D)
    out["b0"] = torch.tensor([0.1])
    return out


def main():
    ref = load_reference()
    rec = inputs()
    for name in "ab":
        x, y = rec[f"x_{name}"], rec[f"y_{name}"]
        assert float(x.min()) < 0.0 and float(x.max()) > 1.0
        assert 0 < int(y.sum()) < len(y)
    w0 = rec["w0"].reshape(-1)
    assert int((w0 == 0).sum()) == 3 and float(w0[w0 != 0].abs().min()) >= 1e-3
    head = nn.Linear(D, 1)
    with torch.no_grad():
        head.weight.copy_(rec["w0"])
        head.bias.copy_(rec["b0"])
    zmax = [0.0]
    head.register_forward_hook(lambda m, i, o: zmax.__setitem__(0, max(zmax[0], float(o.detach().abs().max()))))
    model = ref.HeadOnlyPolicy(head)
    criterion = nn.BCEWithLogitsLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=LR)
    model.train()
    for s in range(STEPS):
        name = "ab"[s % 2]
        x, y = rec[f"x_{name}"], rec[f"y_{name}"]
        x_adv, _ = ref.pgd_attack(model, criterion, x, y, "cpu", epsilon=EPSILON, alpha=ALPHA, num_iters=ITERS)
        loss = criterion(model(x_adv), y)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        xa = np.ascontiguousarray(x_adv.numpy())
        rec[f"s{s}_x_adv_sha256"] = torch.from_numpy(np.frombuffer(hashlib.sha256(xa.tobytes()).digest(), np.uint8).copy())
        rec[f"s{s}_x_adv_rowsum"] = torch.from_numpy(xa.astype(np.float64).sum(1))
        if s in FULL_X_ADV:
            rec[f"s{s}_x_adv"] = x_adv[:FULL_X_ADV[s]].clone()
        rec[f"s{s}_loss"] = loss.detach().double().reshape(1)
        rec[f"s{s}_w"] = head.weight.detach().clone()
        rec[f"s{s}_b"] = head.bias.detach().clone()
        assert float(head.weight.detach().abs().min()) >= 1e-5, s
    assert zmax[0] <= 12.0, zmax
    out = {k: np.ascontiguousarray(v.detach().numpy()) for k, v in rec.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB, {len(out)} arrays; max |z| {zmax[0]:.3f}; losses "
          + " ".join(f"{float(rec[f's{s}_loss']):.6f}" for s in range(STEPS)))


if __name__ == "__main__":
    main()
