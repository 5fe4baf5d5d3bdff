"""Time the RGB viewer's frame (gr_view_render: view_setup_kernel + view_render_kernel, csrc/gr_viewer.hip) and the
device-to-host copy render() adds, on an obstacle track: HIP events around `reps` calls.  Run under rocprofv3
--kernel-trace --stats for the split between the two kernels.

    python scripts/time_viewer.py [--size 640x480] [--mode chase] [--reps 200] [--out profiles/viewer_frame.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg, SceneCfg, SimCfg, TerrainCfg  # noqa: E402
from generalizableracing_amd.envs.racing_env import RacingEnv  # noqa: E402
from generalizableracing_amd.envs.viewer import ViewerCfg, parse_size  # noqa: E402


def _events_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--mode", default="chase")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = parse_size(a.size)
    cfg = RacingEnvCfg(scene=SceneCfg(num_envs=64), sim=SimCfg(device="cuda:0"), terrain=TerrainCfg(obstacles=True))
    env = RacingEnv(cfg, render_mode="rgb_array", viewer=ViewerCfg(width=w, height=h, mode=a.mode))
    env.reset()
    host = torch.empty(h, w, 3, dtype=torch.uint8, pin_memory=True)
    rgb = env.render_view()  # (allocates the buffers and the context's scratch)
    torch.cuda.synchronize()
    for _ in range(10):
        env.render_view()
    res = {"size": [w, h], "mode": a.mode, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "obstacles_in_track_0": int(env.obstacle_table.counts[0]),
           "render_view_rgb_ms": _events_ms(env.render_view, a.reps),
           "render_view_rgb_gbuffer_ms": _events_ms(lambda: env.render_view(gbuffer=True), a.reps),
           "copy_to_pinned_host_ms": _events_ms(lambda: host.copy_(rgb, non_blocking=True), a.reps)}
    import time

    t = time.perf_counter()
    for _ in range(a.reps):
        env.render()
    res["render_numpy_wall_ms"] = (time.perf_counter() - t) / a.reps * 1e3
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    env.close()


if __name__ == "__main__":
    main()
