"""Restatements the offline-stage tests compare against — TEST INFRASTRUCTURE.

* `Collector`: the reference collector's per-step selection as a plain numpy loop, written from
  standalone/offline/data_collector.py:124-146 (positive rows first, then at most as many zero-label rows, each in
  row order, each cut where the dataset fills up; a positive label is stored as 1).
* `pgd`: the attack of standalone/offline/train.py:11-31 for a linear head, with the step direction from a float64
  logit (its sign is what the fp32 logit's sign is whenever sigmoid(z) is not 0 or 1 in fp32) and the fp32 add, sub and
  clamp arithmetic of the original.
* `loss_and_grads`, `adam_step`: BCEWithLogitsLoss(mean), its gradient for the linear head and torch.optim.Adam's
  default update, in float64.
* `check_x_adv`: an attacked batch against tests/golden/golden_offline.npz, bit for bit.
"""
from __future__ import annotations

import hashlib

import numpy as np


class Collector:
    def __init__(self, capacity: int, dim: int):
        self.capacity = capacity
        self.features = np.zeros((capacity, dim), np.float32)
        self.supervision = np.zeros(capacity, np.int8)
        self.w = self.pos = self.neg = 0

    def add(self, feat: np.ndarray, aux: np.ndarray):
        cap = self.capacity
        positive = [i for i in range(len(aux)) if aux[i] != 0]
        negative = [i for i in range(len(aux)) if aux[i] == 0]
        if len(positive) > 0:
            if self.w + len(positive) >= cap:
                positive = positive[:cap - self.w]
            for i in positive:
                self.features[self.w] = feat[i]
                self.supervision[self.w] = 1
                self.w += 1
        if len(negative) > 0:
            if len(negative) > len(positive):
                negative = negative[:len(positive)]
            if self.w + len(negative) >= cap:
                negative = negative[:cap - self.w]
            for i in negative:
                self.features[self.w] = feat[i]
                self.supervision[self.w] = 0
                self.w += 1
        self.pos += len(positive)
        self.neg += len(negative)
        return len(positive), len(negative)

    def cursor(self):
        return (self.w, self.pos, self.neg)


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def pgd(x0, y, w, b, epsilon, alpha, iters):
    """x0 [rows, d] fp32, y [rows] in {0, 1}, w [d], b scalar -> x_adv [rows, d] fp32 (iters = 0: clamp(x0, 0, 1))."""
    x0 = np.asarray(x0, np.float32)
    eps32, alpha32 = np.float32(epsilon), np.float32(alpha)
    w64 = np.asarray(w, np.float64)
    sw = np.sign(np.asarray(w, np.float32)).astype(np.float32)
    if iters == 0:
        return np.clip(x0, np.float32(0), np.float32(1))
    x = x0.copy()
    for _ in range(iters):
        z = x.astype(np.float64) @ w64 + float(b)
        g = _sigmoid(z) - np.asarray(y, np.float64)
        s = np.sign(g).astype(np.float32)[:, None] * sw[None, :]
        x = (x + alpha32 * s).astype(np.float32)
        p = np.clip((x - x0).astype(np.float32), -eps32, eps32)
        x = np.clip((x0 + p).astype(np.float32), np.float32(0), np.float32(1))
    return x


def loss_and_grads(x, y, w, b):
    """float64: (mean softplus(z) - y z, gw [d], gb) on x [rows, d]."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    z = x @ np.asarray(w, np.float64) + float(b)
    loss = np.mean(np.maximum(z, 0.0) - y * z + np.log1p(np.exp(-np.abs(z))))
    g = _sigmoid(z) - y
    return float(loss), g @ x / len(y), float(g.sum() / len(y))


def adam_step(p, g, m, v, t, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's default update in float64 on (p, m, v) with gradient g at step t (1-based) -> (p, m, v)."""
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps
    return p - (lr / (1.0 - beta1 ** t)) * m / denom, m, v


def check_x_adv(gold, s, x_adv: np.ndarray):
    """x_adv of step s against the fixture, bit for bit: the rows it keeps in full, every row's float64 sum, and the
    SHA-256 of the whole array."""
    if f"s{s}_x_adv" in gold:
        want = gold[f"s{s}_x_adv"]
        assert np.array_equal(x_adv[:len(want)].view(np.uint32), want.view(np.uint32)), s
    bad = np.flatnonzero(x_adv.astype(np.float64).sum(1) != gold[f"s{s}_x_adv_rowsum"])
    assert bad.size == 0, (s, bad[:8])
    digest = hashlib.sha256(np.ascontiguousarray(x_adv).tobytes()).digest()
    assert digest == gold[f"s{s}_x_adv_sha256"].tobytes(), s
