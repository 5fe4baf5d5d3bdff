"""The offline auxiliary-head stage (reference: standalone/offline/data_collector.py, standalone/offline/train.py):
a balanced (feature, label) dataset collected on the device while a checkpoint plays, and the PGD-hardened fine-tune
of VisionActorCritic.aux_decoder on it."""
from .collector import FeatureCollector
from .finetune import HeadFinetuner, pgd_attack

__all__ = ["FeatureCollector", "HeadFinetuner", "pgd_attack"]
