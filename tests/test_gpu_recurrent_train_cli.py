"""standalone/rsl_rl/train.py with the recurrent recipe (--agent rsl_rl_recurrent_cfg_entry_point) on the State task,
in a fresh child process as a user starts it: it exits 0, logs finite losses and writes a checkpoint that
standalone/rsl_rl/play.py loads, exports (TorchScript with the hidden state in and out) and steps."""
import glob
import json
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "DiffLab-Quadcopter-CTBR-Racing-State-v0"
AGENT = "rsl_rl_recurrent_cfg_entry_point"


def _run(script, *args, limit=240):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "standalone", "rsl_rl", script),
           "--task", TASK, "--agent", AGENT, "--headless", *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)


def test_train_then_play_the_recurrent_recipe(tmp_path):
    out = _run("train.py", "--num_envs", "64", "--max_iterations", "2", "--log_root", str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"Mean (?:value_function|surrogate) loss:\s*(\S+)", out.stdout)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), out.stdout[-2000:]  # 2 iterations x 2 terms
    ckpts = glob.glob(str(tmp_path / "rsl_rl" / "racing_ppo_recurrent" / "*" / "model_*.pt"))
    assert ckpts
    import torch

    keys = torch.load(ckpts[0], weights_only=True, map_location="cpu")["model_state_dict"].keys()
    assert "memory_a.rnn.weight_hh_l0" in keys and "memory_c.rnn.bias_ih_l0" in keys
    played = _run("play.py", "--num_envs", "64", "--max_steps", "5", "--log_root", str(tmp_path))
    assert played.returncode == 0, played.stdout[-2000:] + played.stderr[-2000:]
    summary = json.loads(played.stdout.strip().splitlines()[-1])
    assert summary["steps"] == 5 and summary["num_envs"] == 64
    m = torch.jit.load(summary["exported"]["jit"])
    actions, h = m(torch.zeros(3, 16), torch.zeros(1, 3, 192))
    assert actions.shape == (3, 4) and h.shape == (1, 3, 192)
