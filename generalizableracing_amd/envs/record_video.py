"""RecordVideo: gymnasium's video wrapper as the reference's launchers use it (standalone/rsl_rl/train.py:102-113,
play.py: `gym.wrappers.RecordVideo(env, video_folder, step_trigger, video_length)`), for the HIP env.

It sits between `RacingEnv` (render_mode="rgb_array") and `RslRlVecEnvWrapper`.  When `step_trigger(k)` is true for
the k-th `step` call (k = 0 for the first), the frames of `video_length` consecutive steps, one per step, rendered
after the step has returned, go to `<video_folder>/<name_prefix>-step-<k>.gif`; a trigger that fires while a
recording runs is ignored, as in gymnasium.  Everything else is the wrapped env's own attribute, so the runner's
fast paths (`unwrapped`, `set_obs_sink`, `episode_length_buf`, the output sets) see the env as before.

Frames are written as an animated GIF through PIL when it imports, else as numbered binary PPM files
`<name_prefix>-step-<k>/frame_00000.ppm` ... (no other encoder is assumed).  With several ranks only rank 0 records.
"""
from __future__ import annotations

import os

import numpy as np

_OWN = ("env", "video_folder", "step_trigger", "video_length", "name_prefix", "fps", "enabled", "step_id",
        "recording", "_frames", "_name", "written")


def _import_pil():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def write_video(stem: str, frames: list, fps: float) -> str:
    """Frames (uint8 [H, W, 3]) to `stem`.gif (PIL), else to the folder `stem` of binary PPM files.  Returns the path."""
    Image = _import_pil()
    if Image is not None:
        path = stem + ".gif"
        imgs = [Image.fromarray(f, "RGB") for f in frames]
        imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(20, int(round(1000.0 / fps))), loop=0)
        return path
    os.makedirs(stem, exist_ok=True)
    for k, f in enumerate(frames):
        with open(os.path.join(stem, f"frame_{k:05d}.ppm"), "wb") as fh:
            fh.write(f"P6 {f.shape[1]} {f.shape[0]} 255\n".encode())
            fh.write(np.ascontiguousarray(f).tobytes())
    return stem


class RecordVideo:
    def __init__(self, env, video_folder: str, step_trigger, video_length: int, name_prefix: str = "rl-video",
                 rank: int = 0):
        if video_length <= 0:
            raise ValueError("video_length must be positive")
        if getattr(env, "render_mode", None) != "rgb_array":
            raise ValueError('RecordVideo needs an env made with render_mode="rgb_array"')
        self.env = env
        self.video_folder = os.path.abspath(video_folder)
        self.step_trigger = step_trigger
        self.video_length = int(video_length)
        self.name_prefix = name_prefix
        step_dt = getattr(env, "step_dt", None)
        self.fps = 1.0 / step_dt if step_dt else 30.0
        self.enabled = rank == 0
        self.step_id = 0
        self.recording = False
        self._frames: list = []
        self._name = None
        self.written: list = []  # paths of the finished videos
        if self.enabled:
            os.makedirs(self.video_folder, exist_ok=True)

    # everything else is the wrapped env's
    def __getattr__(self, name):
        return getattr(self.__dict__["env"], name)

    def __setattr__(self, name, value):
        if name in _OWN:
            object.__setattr__(self, name, value)
        else:
            setattr(self.env, name, value)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def step(self, action):
        out = self.env.step(action)
        if self.enabled:
            if not self.recording and self.step_trigger(self.step_id):
                self.recording = True
                self._frames = []
                self._name = f"{self.name_prefix}-step-{self.step_id}"
            if self.recording:
                self._frames.append(np.asarray(self.env.render()))
                if len(self._frames) >= self.video_length:
                    self._finish()
        self.step_id += 1
        return out

    def _finish(self):
        if self.recording and self._frames:
            self.written.append(write_video(os.path.join(self.video_folder, self._name), self._frames, self.fps))
        self.recording = False
        self._frames = []

    def close(self):
        self._finish()  # (a recording cut short by the end of the run keeps the frames it has)
        return self.env.close()
