"""The RGB viewer's configuration and its `view` array (gr_view_render, include/gr.h).

The reference records videos through gym's `render_mode="rgb_array"` and Isaac Sim's viewport
(standalone/rsl_rl/train.py:102-113); here a frame is a HIP ray cast of one env's analytic track
(csrc/gr_viewer.hip) from a first-person, chase or fixed camera.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .. import _abi

MODES = {"fpv": _abi.GR_VIEW_FPV, "chase": _abi.GR_VIEW_CHASE, "fixed": _abi.GR_VIEW_FIXED}


@dataclass
class ViewerCfg:
    width: int = 640
    height: int = 480
    env_id: int = 0
    mode: str = "chase"           # "fpv" | "chase" | "fixed"
    fov_deg: float = 90.0         # vertical field of view; square pixels, principal point at the centre
    max_distance: float = 40.0
    chase_back: float = 1.5       # the chase camera: metres behind the drone along its heading,
    chase_up: float = 0.6         # above it,
    chase_ahead: float = 1.0      # and the point ahead of it the camera looks at
    eye: tuple = (-3.0, 0.0, 2.0)     # the fixed camera, env-local frame, z up
    target: tuple = (0.0, 0.0, 0.5)


def mode_id(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"unknown viewer mode {mode!r}: one of {sorted(MODES)}")
        return MODES[mode]
    return int(mode)


def view_array(cfg: ViewerCfg, width: int | None = None, height: int | None = None, *, fx=None, fy=None, cx=None,
               cy=None, max_distance=None, eye=None, target=None) -> np.ndarray:
    """The float32 [GR_VIEW_FLOATS] host array of gr_view_render for `cfg` at width x height; the keywords replace
    single entries (the depth sensor's intrinsics for a first-person frame, another fixed camera)."""
    w = cfg.width if width is None else int(width)
    h = cfg.height if height is None else int(height)
    v = np.zeros(_abi.GR_VIEW_FLOATS, dtype=np.float32)
    f = 0.5 * h / math.tan(math.radians(0.5 * cfg.fov_deg))
    v[_abi.GR_VIEW_FX] = f if fx is None else fx
    v[_abi.GR_VIEW_FY] = f if fy is None else fy
    v[_abi.GR_VIEW_CX] = 0.5 * w if cx is None else cx
    v[_abi.GR_VIEW_CY] = 0.5 * h if cy is None else cy
    v[_abi.GR_VIEW_MAX_DISTANCE] = cfg.max_distance if max_distance is None else max_distance
    v[_abi.GR_VIEW_CHASE_BACK] = cfg.chase_back
    v[_abi.GR_VIEW_CHASE_UP] = cfg.chase_up
    v[_abi.GR_VIEW_CHASE_AHEAD] = cfg.chase_ahead
    v[_abi.GR_VIEW_EYE:_abi.GR_VIEW_EYE + 3] = cfg.eye if eye is None else eye
    v[_abi.GR_VIEW_TARGET:_abi.GR_VIEW_TARGET + 3] = cfg.target if target is None else target
    return v


def parse_size(text: str) -> tuple[int, int]:
    """'WxH' -> (W, H) (the CLI's --video_size)."""
    try:
        w, h = (int(t) for t in text.lower().split("x"))
    except ValueError:
        raise ValueError(f"expected WxH, e.g. 640x480, got {text!r}") from None
    return w, h
