"""standalone/rsl_rl/train.py with the recurrent recipe (--agent rsl_rl_recurrent_cfg_entry_point) on the vision task,
in a fresh child process as a user starts it: it exits 0, logs finite losses and writes a checkpoint; --resume runs one
more iteration from it; standalone/rsl_rl/play.py loads it, exports (TorchScript with the hidden state in and out) and
steps; --graph_update with this agent exits with PPO's refusal."""
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
TASK = "DiffLab-Quadcopter-CTBR-Racing-v0"
AGENT = "rsl_rl_recurrent_cfg_entry_point"
LOSS = r"Mean (?:value_function|surrogate) loss:\s*(\S+)"


def _run(script, *args, limit=240):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "standalone", "rsl_rl", script),
           "--task", TASK, "--agent", AGENT, "--headless", *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)


def test_train_resume_play_and_the_graph_refusal(tmp_path):
    out = _run("train.py", "--num_envs", "16", "--max_iterations", "2", "--log_root", str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    losses = [float(v) for v in re.findall(LOSS, out.stdout)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), out.stdout[-2000:]  # 2 iterations x 2 terms
    runs = str(tmp_path / "rsl_rl" / "racing_ppo_vision_recurrent" / "*" / "model_*.pt")
    ckpts = glob.glob(runs)
    assert ckpts
    import torch

    keys = torch.load(ckpts[0], weights_only=True, map_location="cpu")["model_state_dict"].keys()
    assert {"memory_a.rnn.weight_ih_l0", "memory_c.rnn.bias_hh_l0", "stem.0.weight", "state_enc.weight"} <= set(keys)
    resumed = _run("train.py", "--num_envs", "16", "--max_iterations", "1", "--resume", "True", "--log_root",
                   str(tmp_path))
    assert resumed.returncode == 0, resumed.stdout[-2000:] + resumed.stderr[-2000:]
    assert "Loading model checkpoint" in resumed.stdout
    again = [float(v) for v in re.findall(LOSS, resumed.stdout)]
    assert len(again) == 2 and all(math.isfinite(v) for v in again), resumed.stdout[-2000:]
    played = _run("play.py", "--num_envs", "16", "--max_steps", "5", "--log_root", str(tmp_path))
    assert played.returncode == 0, played.stdout[-2000:] + played.stderr[-2000:]
    summary = json.loads(played.stdout.strip().splitlines()[-1])
    assert summary["steps"] == 5 and summary["num_envs"] == 16
    m = torch.jit.load(summary["exported"]["jit"])
    actions, h = m(torch.zeros(3, 16 + 72 * 96), torch.zeros(1, 3, 192))
    assert actions.shape == (3, 4) and h.shape == (1, 3, 192)
    assert "recurrent" in summary["exported"]["onnx"]  # ONNX stays refused for a recurrent policy
    refused = _run("train.py", "--num_envs", "16", "--max_iterations", "1", "--graph_update", "--log_root",
                   str(tmp_path))
    assert refused.returncode != 0
    assert "graph_update=True is not supported with a recurrent policy" in refused.stderr
