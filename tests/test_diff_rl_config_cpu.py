"""The diff_rl workflow's configuration: the registry key, the runner cfg's values against the reference's
(diff_rl_naive_cfg.py:9-32 over RslRlOnPolicyRunnerCfg, listed here as data), the env cfg's new fields, and the
checks that need no GPU: a configuration that is not lean is refused, stepping past the tape raises."""
import ctypes as C
import importlib

import pytest
import torch

from generalizableracing_amd import _abi
from generalizableracing_amd.diff_rl import diff_ops
from generalizableracing_amd.envs.racing_cfg import LossesCfg, RacingEnvCfg, SceneCfg, SimCfg

TASK = "DiffLab-Quadcopter-CTBR-Racing-State-v0"
REFERENCE = {
    "num_steps_per_env": 48, "max_iterations": 2000, "save_interval": 200, "experiment_name": "test_hover",
    "empirical_normalization": False, "init_at_random_ep_len": True,
    "algorithm": {"class_name": "BPTT", "schedule": "CosineAnnealingLR", "optimizer": "AdamW", "learning_rate": 5e-4},
    "policy": {"class_name": "BaseModel", "actor_hidden_dims": [256, 128], "critic_hidden_dims": [256, 128],
               "activation": "lrelu", "init_noise_std": 1.0},
}


def test_registry_key_resolves_to_the_reference_values():
    registry = importlib.import_module("generalizableracing_amd.registry")
    cfg = registry.load_cfg_from_registry(TASK, "diff_rl_cfg_entry_point")
    d = cfg.to_dict()
    for k, v in REFERENCE.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                assert d[k][kk] == vv, (k, kk)
        else:
            assert d[k] == v, k
    assert d["fused"] is True  # not in the reference
    assert "diff_rl_cfg_entry_point" not in registry.registry()["DiffLab-Quadcopter-CTBR-Racing-v0"]


def test_env_cfg_fields():
    cfg = RacingEnvCfg(scene=SceneCfg(num_envs=16), sim=SimCfg(device="cpu"))
    assert cfg.is_differentiable_physics is False
    assert cfg.losses.weights() == (1.0, 0.05, 0.5) and cfg.grad_decay_factor == 0.92 and cfg.diff_window == 48
    assert LossesCfg(racing_vel=0.0).weights() == (1.0, 0.0, 0.5)  # a weight of 0 disables a term


@pytest.mark.parametrize("field,value", [("integrator", _abi.GR_INTEGRATOR_SEMI_IMPLICIT), ("use_motor_model", 1),
                                         ("dr_rotor", 1)])
def test_not_lean_is_refused(field, value):
    c = RacingEnvCfg(scene=SceneCfg(num_envs=16), sim=SimCfg(device="cpu")).to_gr_config()
    assert diff_ops.lean_error(c) is None
    setattr(c, field, value)
    assert diff_ops.lean_error(c)
    with pytest.raises(ValueError, match="cannot be differentiated"):
        diff_ops.DiffTape(None, c, 4, "cpu", fused=False)
    # the library refuses it too, with its reason, before any device use
    ctx = C.c_void_p()
    _abi.call("gr_create", C.byref(c), C.byref(ctx))
    lib = _abi.load()
    assert lib.gr_diff_record(ctx, 16, 16, None) == -1
    assert b"not lean" in lib.gr_last_error(ctx)
    assert lib.gr_diff_backward(ctx, 16, 1, 1.0, 16, None) == -1
    lib.gr_destroy(ctx)


def test_tape_overflow_raises():
    from oracle_diff_vecenv import OracleDiffVecEnv

    env = OracleDiffVecEnv(num_envs=4, t_max=2, dtype=torch.float32, types=1)
    a = torch.zeros(4, 4)
    env.detach()
    env.step(a)
    env.step(a)
    with pytest.raises(RuntimeError, match="detach"):
        env.step(a)
    env.detach()
    env.step(a)
    with pytest.raises(ValueError, match="32-bit"):
        diff_ops.DiffTape(None, env.gr_config, 2 ** 31 // (18 * 4) + 1, "meta", fused=False)
