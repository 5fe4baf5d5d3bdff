"""The balanced feature collector of the offline stage, on the device (gr_offline_collect, csrc/gr_offline.hip).

standalone/offline/data_collector.py:124-146 stores, per env step, the fused feature of every env whose auxiliary
label is non-zero and then of at most as many zero-label envs, both in env order, until N_positive + N_negative rows
are written; it does so with nonzero(), boolean-index slices and .cpu().numpy() copies into an HDF5 file every step.
Here the dataset lives on the device and one call per step compacts the selected rows into it; nothing is read back
until `count()`.

Files: `features.npy` (fp32 [rows, dim]) and `supervision.npy` (int8 [rows, 1]) in a directory, trimmed to the rows
written; with h5py installed also the reference's HDF5 layout (datasets `features` and `supervision`) for a path
ending in .h5.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _abi

# the number of env steps compacted through gr_offline_collect (tests read it: the device path was taken)
CALLS = 0


def select_rows(aux: torch.Tensor, written: int, capacity: int):
    """data_collector.py:124-146 on one step's labels aux [n]: (positive row ids kept, zero-label row ids kept)."""
    pos = torch.nonzero(aux, as_tuple=False).squeeze(-1)
    neg = torch.nonzero(aux == 0, as_tuple=False).squeeze(-1)
    if len(pos) > 0:
        if written + len(pos) >= capacity:
            pos = pos[:capacity - written]
        written += len(pos)
    if len(neg) > 0:
        if len(neg) > len(pos):
            neg = neg[:len(pos)]
        if written + len(neg) >= capacity:
            neg = neg[:capacity - written]
    return pos, neg


def _h5py():
    try:
        import h5py
    except ImportError:
        return None
    return h5py


class FeatureCollector:
    """A device dataset of `capacity` rows of `dim` features with an int8 label each, filled by `add`."""

    def __init__(self, capacity: int, dim: int, device="cuda:0"):
        if capacity < 1 or dim < 1:
            raise ValueError("FeatureCollector: capacity and dim must be positive")
        self.capacity, self.dim = int(capacity), int(dim)
        self.device = torch.device(device)
        self.features = torch.zeros(self.capacity, self.dim, device=self.device, dtype=torch.float32)
        self.supervision = torch.zeros(self.capacity, device=self.device, dtype=torch.int8)
        self.cursor = torch.zeros(3, device=self.device, dtype=torch.int64)  # rows, positives, negatives written
        self._scratch = None

    # ------------------------------------------------------------------ filling
    def add(self, feat: torch.Tensor, aux: torch.Tensor) -> None:
        """One env step: feat [n, dim] fp32 and aux [n] or [n, 1] fp32 (row-strided views are fine).  No sync."""
        if aux.dim() == 2:
            aux = aux[:, 0]
        if feat.dim() != 2 or feat.shape[1] != self.dim or aux.shape[0] != feat.shape[0]:
            raise ValueError(f"FeatureCollector.add: feat {tuple(feat.shape)} / aux {tuple(aux.shape)} for dim {self.dim}")
        if feat.dtype != torch.float32 or aux.dtype != torch.float32:
            raise ValueError("FeatureCollector.add: fp32 features and labels")
        if self.device.type != "cuda":
            return self._add_eager(feat, aux)
        global CALLS
        n = feat.shape[0]
        if n == 0:
            return
        if feat.stride(1) != 1:
            feat = feat.contiguous()
        if self._scratch is None or self._scratch.numel() < n + 4:
            self._scratch = torch.empty(int(_abi.load().gr_offline_scratch_ints(n)), device=self.device,
                                        dtype=torch.int32)
        _abi.call("gr_offline_collect", feat.data_ptr(), feat.stride(0), aux.data_ptr(), aux.stride(0), n, self.dim,
                  self.features.data_ptr(), self.supervision.data_ptr(), self.capacity, self.cursor.data_ptr(),
                  self._scratch.data_ptr(), _abi.raw_stream(self.device))
        CALLS += 1

    def _add_eager(self, feat, aux):
        """The same selection in plain torch (the CPU tests' path and the timing script's baseline)."""
        w = int(self.cursor[0])
        pos, neg = select_rows(aux, w, self.capacity)
        for ids, label in ((pos, 1), (neg, 0)):
            k = len(ids)
            if k:
                self.features[w:w + k] = feat[ids]
                self.supervision[w:w + k] = label
                w += k
        self.cursor += torch.tensor([len(pos) + len(neg), len(pos), len(neg)], device=self.cursor.device)

    # ------------------------------------------------------------------ reading
    def counts(self):
        """(rows, positives, negatives) written: reads the device cursor (the only synchronisation)."""
        return tuple(int(v) for v in self.cursor.tolist())

    def count(self) -> int:
        return self.counts()[0]

    def full(self) -> bool:
        return self.count() >= self.capacity

    def dataset(self):
        """(features [rows, dim], supervision [rows]) views of the rows written."""
        n = self.count()
        return self.features[:n], self.supervision[:n]

    # ------------------------------------------------------------------ files
    def save(self, path: str) -> str:
        feats, sup = self.dataset()
        feats = feats.cpu().numpy()
        sup = sup.cpu().numpy().reshape(-1, 1)
        if path.endswith(".h5"):
            h5py = _h5py()
            if h5py is None:
                raise RuntimeError("an .h5 dataset needs the h5py package; save to a directory instead")
            with h5py.File(path, "w") as f:
                f.create_dataset("features", data=feats, maxshape=(None, self.dim))
                f.create_dataset("supervision", data=sup, maxshape=(None, 1))
            return path
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, "features.npy"), feats)
        np.save(os.path.join(path, "supervision.npy"), sup)
        return path

    @staticmethod
    def read(path: str):
        """(features [rows, dim] fp32, supervision [rows, 1] int8) of a saved dataset: memory-mapped .npy files of a
        directory, or the reference's .h5 file where h5py is installed."""
        if os.path.isdir(path):
            feats = np.load(os.path.join(path, "features.npy"), mmap_mode="r")
            sup = np.load(os.path.join(path, "supervision.npy"), mmap_mode="r")
        else:
            h5py = _h5py()
            if h5py is None:
                raise RuntimeError(f"{path} is not a dataset directory, and reading an .h5 file needs h5py")
            with h5py.File(path, "r") as f:
                feats, sup = np.asarray(f["features"]), np.asarray(f["supervision"])
        if feats.dtype != np.float32 or sup.dtype != np.int8 or sup.shape != (feats.shape[0], 1):
            raise ValueError(f"{path}: features fp32 [rows, dim] and supervision int8 [rows, 1] expected")
        return feats, sup

    @classmethod
    def load(cls, path: str, device="cuda:0", capacity: int | None = None) -> "FeatureCollector":
        feats, sup = cls.read(path)
        n = feats.shape[0]
        c = cls(max(int(capacity or n), n, 1), feats.shape[1], device)
        c.features[:n] = torch.from_numpy(np.array(feats)).to(c.device)
        labels = torch.from_numpy(np.array(sup[:, 0])).to(c.device)
        c.supervision[:n] = labels
        pos = int((labels != 0).sum())
        c.cursor.copy_(torch.tensor([n, pos, n - pos]))
        return c
