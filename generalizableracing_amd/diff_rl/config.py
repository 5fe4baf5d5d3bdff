"""Runner configuration of the diff_rl workflow (QuadcopterDIffRLRunnerCfg, diff_rl_naive_cfg.py:9-32, over
standalone/diff_rl/algorithms/config.py) as plain dataclasses; `to_dict()` is what AlgoRunner takes."""
from __future__ import annotations

from dataclasses import asdict, dataclass, field


@dataclass
class DiffRLModelCfg:
    class_name: str = "BaseModel"
    init_noise_std: float = 1.0
    noise_std_type: str = "scalar"
    actor_hidden_dims: list = field(default_factory=lambda: [256, 128])
    critic_hidden_dims: list = field(default_factory=lambda: [256, 128])
    activation: str = "lrelu"


@dataclass
class DiffRLAlgorithmCfg:
    class_name: str = "BPTT"
    schedule: str = "CosineAnnealingLR"
    optimizer: str = "AdamW"
    learning_rate: float = 5e-4


@dataclass
class QuadcopterDiffRLRunnerCfg:
    seed: int = 42
    device: str = "cuda:0"
    num_steps_per_env: int = 48
    max_iterations: int = 2000
    save_interval: int = 200
    experiment_name: str = "test_hover"
    run_name: str = ""
    logger: str = "tensorboard"
    empirical_normalization: bool = False
    init_at_random_ep_len: bool = True
    resume: bool = False
    load_run: str = ".*"
    load_checkpoint: str = "model_.*.pt"
    policy: DiffRLModelCfg = field(default_factory=DiffRLModelCfg)
    algorithm: DiffRLAlgorithmCfg = field(default_factory=DiffRLAlgorithmCfg)
    # not in the reference: the tape's record / loss / adjoint as HIP kernels (False: the torch path, the reference's
    # structure)
    fused: bool = True

    def to_dict(self) -> dict:
        return asdict(self)


QuadcopterDIffRLRunnerCfg = QuadcopterDiffRLRunnerCfg  # (the reference's spelling)
