"""The PGD-hardened fine-tune of the auxiliary head (reference: standalone/offline/train.py).

`pgd_attack` is the reference's attack in eager torch, for any head.  `HeadFinetuner` steps a head over a device
dataset one mini-batch at a time: for an nn.Linear with one output on a GPU each step is gr_offline_pgd_step
(csrc/gr_offline.hip: the attack, the loss, the gradient and Adam in two launches, the shuffled batch gathered in
the kernel); otherwise the reference's loop with torch.optim.Adam.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _abi

# the number of mini-batch steps taken through gr_offline_pgd_step (tests and the trainer CLI read it)
CALLS = 0

MAX_FUSED_DIM = 1024  # GR_OFFLINE_PGD_MAX_D
BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults, as the reference's optimizer


def pgd_attack(model, criterion, x, y, epsilon, alpha, num_iters):
    """train.py:11-31: `num_iters` signed-gradient steps of size alpha on the features, the perturbation clamped to
    [-epsilon, epsilon] and the features to [0, 1].  -> (adversarial features, perturbation)."""
    original = x.clone().detach()
    adv = x.clone().detach()
    perturbations = torch.zeros_like(original)
    for _ in range(num_iters):
        adv.requires_grad_(True)
        loss = criterion(model(adv), y)
        model.zero_grad()
        loss.backward()
        with torch.no_grad():
            adv = adv + alpha * adv.grad.sign()
            perturbations = torch.clamp(adv - original, min=-epsilon, max=epsilon)
            adv = torch.clamp(original + perturbations, 0, 1)
        adv = adv.detach()
    return adv, perturbations


def fusable(head, device) -> bool:
    return (torch.device(device).type == "cuda" and isinstance(head, nn.Linear) and head.out_features == 1
            and head.bias is not None and head.in_features <= MAX_FUSED_DIM and head.weight.dtype == torch.float32)


class HeadFinetuner:
    """Fine-tunes `head` in place.  fused=None: the HIP step when `fusable`; fused=True where it is not is an error."""

    def __init__(self, head: nn.Module, lr: float = 3e-4, device="cuda:0", fused=None, epsilon: float = 0.1,
                 alpha: float = 0.01, num_iters: int = 3):
        self.device = torch.device(device)
        self.head = head.to(self.device)
        self.lr = float(lr)
        self.epsilon, self.alpha, self.num_iters = float(epsilon), float(alpha), int(num_iters)
        ok = fusable(self.head, self.device)
        if fused and not ok:
            raise ValueError("HeadFinetuner: the fused step covers an nn.Linear(d <= 1024, 1) head on a GPU")
        self.fused = ok if fused is None else bool(fused)
        self.steps = 0
        if self.fused:
            d = self.head.in_features
            with torch.no_grad():
                self.wb = torch.cat([self.head.weight.reshape(-1), self.head.bias.reshape(-1)]).contiguous()
            self.exp_avg = torch.zeros(d + 1, device=self.device)
            self.exp_avg_sq = torch.zeros(d + 1, device=self.device)
            self.step_count = torch.zeros(1, device=self.device)
            self.loss_acc = torch.zeros(1, device=self.device, dtype=torch.float64)
            self._partial = None
        else:
            self.criterion = nn.BCEWithLogitsLoss()
            self.optimizer = torch.optim.Adam(self.head.parameters(), lr=self.lr)

    # ------------------------------------------------------------------ one mini-batch
    def fused_step(self, features, supervision, index=None, rows=None, x_adv=None, num_iters=None):
        """gr_offline_pgd_step on rows `index` (int64, device; None: the first `rows` rows) of the dataset.  The head's
        parameters live in self.wb until `sync_head`."""
        global CALLS
        if rows is None:
            rows = index.numel() if index is not None else features.shape[0]
        d = self.head.in_features
        if features.dtype != torch.float32 or not features.is_contiguous() or features.shape[1] != d:
            raise ValueError("fused_step: contiguous fp32 features [rows, d]")
        if supervision.dtype != torch.int8 or not supervision.is_contiguous():
            raise ValueError("fused_step: contiguous int8 labels")
        if index is not None and (index.dtype != torch.int64 or not index.is_contiguous()):
            raise ValueError("fused_step: a contiguous int64 index")
        need = int(_abi.load().gr_offline_pgd_partials(rows, d))
        if self._partial is None or self._partial.numel() < need:
            self._partial = torch.empty(need, device=self.device, dtype=torch.float32)
        iters = self.num_iters if num_iters is None else int(num_iters)
        _abi.call("gr_offline_pgd_step", features.data_ptr(), supervision.data_ptr(),
                  None if index is None else index.data_ptr(), rows, d, self.wb.data_ptr(), self.exp_avg.data_ptr(),
                  self.exp_avg_sq.data_ptr(), self.step_count.data_ptr(), self.epsilon, self.alpha, iters, self.lr,
                  BETAS[0], BETAS[1], EPS, self._partial.data_ptr(), self.loss_acc.data_ptr(),
                  None if x_adv is None else x_adv.data_ptr(), _abi.raw_stream(self.device))
        CALLS += 1
        self.steps += 1

    def eager_step(self, x, y):
        """train.py:105-112 on a gathered batch x [rows, d], y [rows, 1] fp32 -> the loss (a tensor)."""
        x, _ = pgd_attack(self.head, self.criterion, x, y, self.epsilon, self.alpha, self.num_iters)
        loss = self.criterion(self.head(x), y)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.steps += 1
        return loss.detach()

    def sync_head(self):
        """The fused step's parameters -> the head module."""
        if self.fused:
            d = self.head.in_features
            with torch.no_grad():
                self.head.weight.copy_(self.wb[:d].view(1, d))
                self.head.bias.copy_(self.wb[d:])
        return self.head

    # ------------------------------------------------------------------ one epoch
    def epoch(self, dataset, batch_size: int = 256, generator=None) -> float:
        """One shuffled pass over `dataset` = (features [n, d] fp32, supervision [n] or [n, 1] int8) on the device (or
        a FeatureCollector), every batch stepped, the short last one included (DataLoader(drop_last=False)).
        -> the epoch's mean loss (sum of loss * rows over n, train.py:113-116), read with one synchronisation."""
        feats, sup = dataset.dataset() if hasattr(dataset, "dataset") else dataset
        feats = feats.to(self.device)
        sup = sup.to(self.device).reshape(-1)
        n = feats.shape[0]
        if n == 0:
            raise ValueError("HeadFinetuner.epoch: an empty dataset")
        perm = torch.randperm(n, device=self.device, generator=generator)
        self.head.train()
        if self.fused:
            feats, sup = feats.contiguous(), sup.contiguous()
            self.loss_acc.zero_()
            for start in range(0, n, batch_size):
                self.fused_step(feats, sup, perm[start:start + batch_size])
            self.sync_head()
            return float(self.loss_acc.item()) / n
        total = torch.zeros((), device=self.device, dtype=torch.float64)
        for start in range(0, n, batch_size):
            idx = perm[start:start + batch_size]
            loss = self.eager_step(feats[idx], sup[idx].float().unsqueeze(1))
            total += loss.double() * idx.numel()
        return float(total.item()) / n
