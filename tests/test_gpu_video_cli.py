"""standalone/rsl_rl/train.py and play.py with --video on the State task, in fresh child processes as a user starts
them: the GIFs the RecordVideo wrapper writes from the HIP viewer's frames, and no trace of the viewer without the flag."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "DiffLab-Quadcopter-CTBR-Racing-State-v0"


def _run(script, *args, limit=240):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "standalone", "rsl_rl", script),
           "--task", TASK, "--headless", *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)


def _gif(path):
    from PIL import Image

    im = Image.open(path)
    frames = []
    for k in range(im.n_frames):
        im.seek(k)
        frames.append(np.array(im.convert("RGB")))
    return im.size, frames


def test_train_and_play_record_videos(tmp_path):
    out = _run("train.py", "--num_envs", "64", "--max_iterations", "2", "--video", "--video_length", "4",
               "--video_interval", "24", "--video_size", "160x120", "--log_root", str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    vids = sorted(glob.glob(str(tmp_path / "rsl_rl" / "*" / "*" / "videos" / "train" / "*")))
    assert [os.path.basename(v) for v in vids] == ["rl-video-step-0.gif", "rl-video-step-24.gif"], vids
    for v in vids:
        size, frames = _gif(v)
        assert size == (160, 120) and len(frames) == 4, (v, size, len(frames))
        assert all(f.std() > 5 for f in frames)  # pictures, not flat images
    played = _run("play.py", "--num_envs", "64", "--video", "--video_length", "6", "--max_steps", "8", "--log_root",
                  str(tmp_path))
    assert played.returncode == 0, played.stdout[-2000:] + played.stderr[-2000:]
    summary = json.loads(played.stdout.strip().splitlines()[-1])
    assert summary["steps"] == 8 and summary["num_envs"] == 64
    pv = glob.glob(os.path.join(os.path.dirname(summary["checkpoint"]), "videos", "play", "*"))
    assert [os.path.basename(v) for v in pv] == ["rl-video-step-0.gif"], pv
    size, frames = _gif(pv[0])
    assert size == (640, 480) and len(frames) == 6


def test_train_without_video_leaves_no_videos_folder(tmp_path):
    out = _run("train.py", "--num_envs", "64", "--max_iterations", "2", "--video_length", "4", "--video_interval", "24",
               "--video_size", "160x120", "--log_root", str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert glob.glob(str(tmp_path / "rsl_rl" / "*" / "*" / "model_*.pt"))
    assert not glob.glob(str(tmp_path / "**" / "videos"), recursive=True)
    assert "Recording videos" not in out.stdout
