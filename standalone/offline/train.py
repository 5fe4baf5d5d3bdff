"""Fine-tune the auxiliary head of a trained checkpoint on a collected dataset (reference: standalone/offline/train.py).

The reference's finetune_policy_head: load the checkpoint, train aux_decoder alone under BCEWithLogitsLoss and
Adam(lr) on 3-step PGD-attacked features (epsilon 0.1, alpha 0.01), and after every epoch write
policy_finetune_epoch-{e}.pt: the checkpoint with the new head, every other entry untouched, so runner.load, play.py
and the exporters take it as they take any checkpoint.  Here the dataset is loaded onto the device once and an epoch
is generalizableracing_amd.offline.HeadFinetuner.epoch (on a GPU: two launches per mini-batch, gr_offline_pgd_step).
The policy class comes from the registry (--task / --agent) with its sizes read from the checkpoint, where the
reference hard-codes a constructor.

    python standalone/offline/train.py --h5_path racing_data --policy_path logs/.../model_3999.pt --save_path out
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Fine-tune the policy's auxiliary head on offline data.")
    p.add_argument("--h5_path", type=str, required=True, help="dataset directory (features.npy, supervision.npy) "
                                                              "or an HDF5 file where h5py is installed")
    p.add_argument("--policy_path", type=str, required=True, help="checkpoint written by the runner")
    p.add_argument("--save_path", type=str, default="policy_finetuned", help="directory for the fine-tuned checkpoints")
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--task", type=str, default="DiffLab-Quadcopter-CTBR-Racing-v0")
    p.add_argument("--agent", type=str, default="rsl_rl_cfg_entry_point")
    p.add_argument("--device", type=str, default=None, help="default: cuda:0 when there is a GPU, else cpu")
    return p


def load_full_policy_model(path, task, agent):
    """-> (the checkpoint dict, its policy built from the registry's recipe).  The observation and action sizes are
    the checkpoint's own (state_enc's input plus the recipe's image; the actor's last layer)."""
    import importlib

    import torch

    registry = importlib.import_module("generalizableracing_amd.registry")
    from generalizableracing_amd.rsl_rl.on_policy_runner import POLICIES

    loaded = torch.load(path, weights_only=True, map_location="cpu")
    state = loaded["model_state_dict"]
    if "aux_decoder.weight" not in state or "state_enc.weight" not in state:
        raise SystemExit(f"{path}: the checkpoint's policy has no auxiliary head (aux_decoder)")
    cfg = dict(registry.load_cfg_from_registry(task, agent).to_dict()["policy"])
    policy_class = POLICIES[cfg.pop("class_name")]
    h, w = cfg.get("img_res", (72, 96))
    num_obs = int(state["state_enc.weight"].shape[1]) + int(h) * int(w)
    last = max((k for k in state if k.startswith("actor.") and k.endswith(".weight")), key=lambda k: int(k.split(".")[1]))
    model = policy_class(num_obs, num_obs, int(state[last].shape[0]), **cfg)
    model.load_state_dict(state)
    return loaded, model


def finetune_policy_head(h5_path, policy_path, save_path, epochs=3, batch_size=256, lr=3e-4, task=None, agent=None,
                         device=None):
    import torch

    from generalizableracing_amd.offline import FeatureCollector, HeadFinetuner

    device = torch.device(device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    feats, sup = FeatureCollector.read(h5_path)
    print(f"[INFO] Loaded dataset with {len(feats)} samples from {h5_path}")
    import numpy as np

    dataset = (torch.from_numpy(np.array(feats)).to(device),
               torch.from_numpy(np.array(sup[:, 0])).to(device))
    loaded, full_policy = load_full_policy_model(policy_path, task, agent)
    if full_policy.aux_decoder.in_features != dataset[0].shape[1]:
        raise SystemExit(f"the dataset's features have {dataset[0].shape[1]} columns, the head takes "
                         f"{full_policy.aux_decoder.in_features}")
    tuner = HeadFinetuner(full_policy.aux_decoder, lr=lr, device=device)
    os.makedirs(save_path, exist_ok=True)
    losses, files = [], []
    for epoch in range(epochs):
        avg_loss = tuner.epoch(dataset, batch_size)
        losses.append(avg_loss)
        print(f"[Epoch {epoch + 1}/{epochs}] Loss: {avg_loss:.6f}")
        head = tuner.sync_head()
        state = loaded["model_state_dict"]
        for k, v in head.state_dict().items():
            key = f"aux_decoder.{k}"
            state[key] = v.detach().to(device=state[key].device, dtype=state[key].dtype).clone()
        out = os.path.join(save_path, f"policy_finetune_epoch-{epoch}.pt")
        torch.save(loaded, out)
        files.append(out)
        print(f"Fine-tuned policy saved to: {out}")
    return {"rows": int(len(feats)), "epochs": epochs, "losses": losses, "files": files, "fused": bool(tuner.fused),
            "steps": tuner.steps, "device": str(device)}


def main(argv=None):
    args = build_parser().parse_args(argv)
    summary = finetune_policy_head(args.h5_path, args.policy_path, args.save_path, args.epochs, args.batch_size,
                                   args.lr, args.task, args.agent, args.device)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
