"""bench.py's plain run and --dump-outputs: the plain line holds the headline alone (no roofline, no extra legs),
--steps is the number of timed steps (70 = one 64-step hipGraph + a 6-step graph), and the dumped arrays are the
last timed step's results: the inputs are seeded, so two runs with the same arguments leave bit-identical files
(what lets two builds be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8192
NAMES = {"obs_policy": (N, 16), "obs_critic": (N, 16), "obs_auxiliary": (N, 1), "reward": (N,), "terminated": (N,),
         "time_out": (N,)}


def _bench(out, *more):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "70", "--warmup", "3",
                        "--num-envs", str(N), "--dump-outputs", str(out), *more], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    line = _bench(tmp_path / "graph")
    assert line["steps"] == 70 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["config"]["launch"] == "hipgraph"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - N * 70 / (line["ms_per_step"] * 1e-3 * 70)) < 1e-6 * line["value"]
    # nothing but the headline ran
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None
    for leg in ("steady_state_env_steps_per_s_per_gpu", "env_only_fp32", "with_obstacles", "env_count_sweep",
                "c5_32_gates", "terrain_regeneration", "vision_camera", "distributed_train",
                "train_total_fps_4096_envs", "train_total_fps_65536_envs", "vision_train_total_fps_4096_envs"):
        assert leg not in line, leg
    again = _bench(tmp_path / "again")
    assert again["steps"] == 70
    assert sorted(os.listdir(tmp_path / "graph")) == sorted(f"{k}.npy" for k in NAMES)
    for name, shape in NAMES.items():
        g, e = np.load(tmp_path / "graph" / f"{name}.npy"), np.load(tmp_path / "again" / f"{name}.npy")
        assert g.dtype == np.float32 and g.shape == shape, name
        assert np.isfinite(g).all(), name
        assert np.array_equal(g.view(np.uint32), e.view(np.uint32)), name
    # the step wrote something: observations are not all zero, and the flags are flags
    assert np.abs(np.load(tmp_path / "graph" / "obs_policy.npy")).max() > 0
    assert set(np.unique(np.load(tmp_path / "graph" / "terminated.npy"))) <= {0.0, 1.0}
