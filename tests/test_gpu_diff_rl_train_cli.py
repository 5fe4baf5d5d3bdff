"""standalone/diff_rl/train.py on the State task in a fresh child process: three BPTT iterations at 256 envs write a
checkpoint and the scalars under logs/diff_rl/<experiment>/; standalone/diff_rl/play.py loads the checkpoint and
steps the env 10 times."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "DiffLab-Quadcopter-CTBR-Racing-State-v0"


def run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "standalone", "diff_rl", script), "--task", TASK, *args],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_train_then_play(tmp_path):
    out = run("train.py", "--num_envs", "256", "--max_iterations", "3", "--headless", "--log_root", str(tmp_path))
    assert "Learning iteration 2/3" in out
    exp = tmp_path / "diff_rl" / "test_hover"
    runs = list(exp.iterdir())
    assert len(runs) == 1
    files = {p.name for p in runs[0].iterdir()}
    assert "model_0.pt" in files and "model_2.pt" in files and "params" in files
    if "scalars.csv" in files:
        text = (runs[0] / "scalars.csv").read_text()
        for key in ("Loss/policy", "Policy/mean_noise_std", "Perf/total_fps", "Perf/collection_time",
                    "Perf/learning_time", "Loss/learning_rate"):
            assert key in text, key
    else:
        assert any(f.startswith("events.out.tfevents") for f in files)
    out = run("play.py", "--num_envs", "64", "--steps", "10", "--headless", "--log_root", str(tmp_path))
    assert "model_2.pt" in out and "played 10 steps" in out
