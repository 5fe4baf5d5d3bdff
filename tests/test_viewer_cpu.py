"""The RGB viewer without a GPU: known answers of the float64 restatement (tests/viewer_ref.py), the argument checks
of gr_view_render / gr_view_default, RecordVideo on a stub env, the launchers' flags and the env's metadata."""
import ctypes as C
import glob
import math
import os
import sys

import numpy as np
import pytest

import viewer_ref as vr
from generalizableracing_amd import _abi
from generalizableracing_amd.envs import record_video
from generalizableracing_amd.envs.racing_cfg import RacingEnvCfg
from generalizableracing_amd.envs.tracks import build_tracks
from generalizableracing_amd.envs.viewer import ViewerCfg, parse_size, view_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def _rec(centre, sizes, kind=None, yaw=0.0):
    """A gate / obstacle record at `centre`, rotated by yaw about z (rows of the world -> local rotation)."""
    r = np.zeros(20)
    r[0:3] = centre
    c, s = math.cos(yaw), math.sin(yaw)
    r[4:7], r[8:11], r[12:15] = (c, s, 0.0), (-s, c, 0.0), (0.0, 0.0, 1.0)
    if kind is None:  # gate: inner half width / height, half thickness, outer half width / height
        r[7], r[11], r[15], r[16], r[17] = sizes
    else:
        r[7], r[11], r[15], r[16] = sizes[0], sizes[1], sizes[2], kind
    return r


def _level_camera(h=1.0):
    return np.array([0.0, 0.0, h]), np.eye(3)  # forward +x, left +y, up +z


def _trace(gates=(), obst=(), cam=None, n=33, maxd=40.0, gz=0.0):
    o, Cm = cam if cam is not None else _level_camera()
    sc = vr.make_scene(np.array(gates).reshape(-1, 20), (gz, 0.0, 0, len(gates)),
                       np.array(obst).reshape(-1, 20) if len(obst) else None)
    A, B = vr.ray_grid(n / 2, n / 2, n / 2, n / 2, n, n)
    return vr.trace(sc, o, Cm, A, B, maxd), (A, B)


def test_sphere_dead_ahead():
    d, r = 5.0, 0.5
    (ids, depth, nrm, _, _), _ = _trace(obst=[_rec((d, 0.0, 1.0), (r, r, r), vr.SPHERE)])
    c = 16  # the centre pixel of 33: a = b = 0
    assert ids[c, c] == 1 and abs(depth[c, c] - (d - r)) < 1e-12
    assert np.allclose(nrm[:, c, c], (-1.0, 0.0, 0.0), atol=1e-12)


def test_centre_ray_through_a_gates_hole_hits_what_is_behind():
    # the gate frame: x width, y height, z thickness (the axis flown along); here that axis is the world x
    g = np.zeros(20)
    g[0:3] = (3.0, 0.0, 1.0)
    g[4:7], g[8:11], g[12:15] = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)  # local x = world y, y = z, z = x
    g[7], g[11], g[15], g[16], g[17] = 0.4, 0.4, 0.05, 0.6, 0.6
    wall = _rec((6.0, 0.0, 1.0), (0.1, 2.0, 2.0), vr.BOX)
    (ids, depth, nrm, _, _), (A, B) = _trace(gates=[g], obst=[wall])
    c = 16
    assert ids[c, c] == 2 and abs(depth[c, c] - 5.9) < 1e-12  # through the hole: the box behind (1 + G + 0)
    assert np.allclose(nrm[:, c, c], (-1.0, 0.0, 0.0))
    # a ray into the top bar (z = 1.5 at x = 2.95: b = 0.5 / 2.95) hits the bar's outer face
    bar = np.argmin(np.abs(B[:, 0] - 0.5 / 2.95))
    assert ids[bar, c] == 1 and abs(depth[bar, c] - 2.95) < 1e-12
    assert np.allclose(nrm[:, bar, c], (-1.0, 0.0, 0.0))
    # from inside the hole's prism, looking up at a bar: the hole wall, whose normal points into the hole (down)
    o = np.array([3.0, 0.0, 1.0])
    Cm = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    (ids2, depth2, nrm2, _, _), _ = _trace(gates=[g], cam=(o, Cm))
    assert ids2[c, c] == 1 and abs(depth2[c, c] - 0.4) < 1e-12 and np.allclose(nrm2[:, c, c], (0.0, 0.0, -1.0))


def test_ground_under_a_level_camera():
    h = 1.25
    (ids, depth, nrm, _, _), (A, B) = _trace(cam=_level_camera(h), maxd=1e6)
    below = B[:, 0] < 0
    assert below.sum() == 16
    assert np.allclose(depth[below, :], (h / np.abs(B[below, 0]))[:, None], rtol=1e-13)
    assert (ids[below] == 0).all() and (ids[~below] == -1).all()
    assert (nrm[2][below] == 1.0).all() and (nrm[:, ~below] == 0.0).all()


@pytest.mark.parametrize("kind,sizes,depth,normal", [
    (vr.BOX, (0.5, 1.0, 1.0), 3.5, (-1.0, 0.0, 0.0)),
    (vr.CYLINDER, (0.5, 0.5, 1.0), 3.5, (-1.0, 0.0, 0.0)),
    (vr.CAPSULE, (0.5, 0.5, 1.0), 3.5, (-1.0, 0.0, 0.0)),
])
def test_solids_dead_ahead(kind, sizes, depth, normal):
    (ids, d, nrm, _, _), _ = _trace(obst=[_rec((4.0, 0.0, 1.0), sizes, kind)])
    assert ids[16, 16] == 1 and abs(d[16, 16] - depth) < 1e-12 and np.allclose(nrm[:, 16, 16], normal, atol=1e-12)


def test_capsule_cap_and_cylinder_cap_from_above():
    o = np.array([0.0, 0.0, 5.0])
    down = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    (ids, d, nrm, _, _), _ = _trace(obst=[_rec((0.0, 0.0, 1.0), (0.3, 0.3, 0.5), vr.CAPSULE)], cam=(o, down))
    assert abs(d[16, 16] - (5.0 - 1.8)) < 1e-12 and np.allclose(nrm[:, 16, 16], (0.0, 0.0, 1.0))
    (ids, d, nrm, _, _), _ = _trace(obst=[_rec((0.0, 0.0, 1.0), (0.3, 0.3, 0.5), vr.CYLINDER)], cam=(o, down))
    assert abs(d[16, 16] - 3.5) < 1e-12 and np.allclose(nrm[:, 16, 16], (0.0, 0.0, 1.0))


def test_cameras():
    o, Cm = vr.camera_fixed((0.0, 0.0, 2.0), (3.0, 4.0, 2.0))
    assert np.allclose(Cm[0], (0.6, 0.8, 0.0)) and np.allclose(Cm[1], (-0.8, 0.6, 0.0)) and np.allclose(Cm[2], (0, 0, 1))
    yaw = 0.5 * math.pi
    q = (math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2))
    o, Cm = vr.camera_chase((1.0, 2.0, 3.0), q)
    assert np.allclose(o, (1.0, 0.5, 3.6)) and np.allclose(Cm @ Cm.T, np.eye(3), atol=1e-12)
    assert Cm[0][1] > 0 and Cm[0][2] < 0 and abs(Cm[0][0]) < 1e-12  # looks along +y and down at the point ahead
    # a vertical body x axis: the heading falls back to the world x axis
    o, _ = vr.camera_chase((0.0, 0.0, 1.0), (math.cos(math.pi / 4), 0.0, -math.sin(math.pi / 4), 0.0))
    assert np.allclose(o, (-1.5, 0.0, 1.6))
    o, Cm = vr.camera_fpv((0.0, 0.0, 1.0), IDENT, (0.01, 0.0, 0.0), (0.991, 0.0, -0.131, 0.0))
    assert np.allclose(o, (0.01, 0.0, 1.0)) and Cm[0][2] > 0.2 and np.allclose(Cm[1], (0, 1, 0))  # pitched up


def test_colour_formula_on_known_pixels():
    ids = np.array([[vr.ID_MISS, vr.ID_GROUND, 1, 2, 10, vr.ID_DRONE]], dtype=np.int32)
    depth = np.full((1, 6), 4.0, dtype=np.float32)
    nrm = np.zeros((3, 1, 6), dtype=np.float32)
    nrm[2] = 1.0
    A = np.zeros((1, 6), dtype=np.float32)
    B = np.full((1, 6), -0.5, dtype=np.float32)
    rgb = vr.colour(ids, depth, nrm, A, B, (0.5, 0.5, 2.0), np.eye(3), 40.0, 8, 1, [vr.SPHERE, vr.CAPSULE])
    sky = vr.HORIZON
    assert tuple(rgb[0, 0]) == tuple(int(c * 255 + 0.5) for c in sky)  # b < 0: the horizon colour
    shade, fog = 0.35 + 0.65 * 0.8, 0.01

    def expect(base):
        return tuple(int((b * shade + fog * (s - b * shade)) * 255 + 0.5) for b, s in zip(base, sky))

    # ground at x = 0.5 + 4, y = 0.5: floor 4 + 0 even -> CHECK0; gate 0; the next gate (gate_id 1 -> id 2); obstacle
    # 10 - 1 - 8 = 1 (a capsule); the drone
    for k, base in ((1, vr.CHECK[0]), (2, vr.GATE), (3, vr.NEXT), (4, vr.KINDS[vr.CAPSULE]), (5, vr.DRONE)):
        assert np.abs(rgb[0, k].astype(int) - np.array(expect(base))).max() <= 1, k


# ------------------------------------------------------------------ the ambiguity masks of the GPU test's views
@pytest.fixture(scope="module")
def tracks():
    t = RacingEnvCfg().terrain
    return {obst: build_tracks(num_types=t.num_cols, num_levels=t.num_rows, num_gates=t.num_gates, seed=t.seed,
                               obstacles=obst, cell=t.obstacle_cell) for obst in (False, True)}


@pytest.mark.parametrize("obstacles", [False, True])
def test_ambiguity_masks_of_the_shared_views_are_thin(tracks, obstacles):
    """The band is 2e-3 of a pixel wide around silhouettes and edges: at most 1 % of a view's pixels."""
    gates, recs, obst = tracks[obstacles]
    k = vr.SHARED_TRACK
    p, q = vr.start_pose(gates[k], recs[k])
    half = tuple(_abi.default_config().collider_half)
    orec = obst.records[k][:int(obst.counts[k])] if obst is not None else None
    for name, mode, w, h, fov, maxd, eye, target in vr.shared_views(gates[k], recs[k]):
        fx, fy, cx, cy = vr.intrinsics(w, h, fov)
        A, B = vr.ray_grid(fx, fy, cx, cy, w, h)
        o, Cm = vr.camera_fixed(eye, target) if mode == "fixed" else vr.camera_chase(p, q)
        sc = vr.make_scene(gates[k], recs[k], orec, drone=(p, q, half))
        amb = vr.ambiguity_mask(sc, o, Cm, A, B, maxd, 1.0 / fx, 1.0 / fy)
        ids = vr.trace(sc, o, Cm, A, B, maxd)[0]
        assert amb.mean() <= 0.01, (name, amb.mean())
        assert len(np.unique(ids)) >= 3, (name, np.unique(ids))  # the view shows something


# ------------------------------------------------------------------ C ABI argument checks (no device)
def test_view_default_fills_and_rejects():
    lib = _abi.load()
    v = (C.c_float * _abi.GR_VIEW_FLOATS)()
    assert lib.gr_view_default(v, 640, 480) == 0
    assert v[_abi.GR_VIEW_FX] == 240.0 and v[_abi.GR_VIEW_FY] == 240.0 and v[_abi.GR_VIEW_CX] == 320.0
    assert v[_abi.GR_VIEW_MAX_DISTANCE] == 40.0 and v[_abi.GR_VIEW_CHASE_BACK] == 1.5
    assert abs(v[_abi.GR_VIEW_CHASE_UP] - 0.6) < 1e-7 and v[_abi.GR_VIEW_CHASE_AHEAD] == 1.0
    assert np.array_equal(np.array(v[:]), view_array(ViewerCfg()))
    assert lib.gr_view_default(None, 640, 480) == -1
    for w, h in ((15, 480), (1921, 480), (640, 15), (640, 1081)):
        assert lib.gr_view_default(v, w, h) == -1


def test_view_render_rejects_bad_arguments_before_any_launch():
    lib = _abi.load()
    c = _abi.default_config()
    c.num_envs = 64
    ctx = C.c_void_p()
    assert lib.gr_create(C.byref(c), C.byref(ctx)) == 0
    good = view_array(ViewerCfg())
    p = 0x10000

    def render(env=0, mode=_abi.GR_VIEW_CHASE, view=good, w=640, h=480, rgb=p, gbuf=p):
        v = None if view is None else np.ascontiguousarray(view, dtype=np.float32)
        rc = lib.gr_view_render(ctx, env, mode, None if v is None else v.ctypes.data, w, h, rgb, gbuf, None)
        return rc, lib.gr_last_error(ctx).decode()

    def bad(i, value):
        v = good.copy()
        v[i] = value
        return v

    assert lib.gr_view_render(None, 0, 1, good.ctypes.data, 640, 480, p, p, None) == -1
    cases = [(dict(env=-1), "env"), (dict(env=64), "env"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
             (dict(w=15), "width"), (dict(w=1921), "width"), (dict(h=15), "width"), (dict(h=1081), "width"),
             (dict(rgb=None, gbuf=None), "both null"), (dict(rgb=p + 2), "aligned"), (dict(gbuf=p + 4), "aligned"),
             (dict(view=None), "null"),
             (dict(view=bad(_abi.GR_VIEW_FX, 0.0)), "positive"), (dict(view=bad(_abi.GR_VIEW_FY, -1.0)), "positive"),
             (dict(view=bad(_abi.GR_VIEW_FX, float("nan"))), "finite"),
             (dict(view=bad(_abi.GR_VIEW_CY, float("inf"))), "finite"),
             (dict(view=bad(_abi.GR_VIEW_MAX_DISTANCE, 0.0)), "positive"),
             (dict(view=bad(_abi.GR_VIEW_MAX_DISTANCE, float("inf"))), "finite"),
             (dict(mode=_abi.GR_VIEW_FIXED, view=view_array(ViewerCfg(), eye=(1, 2, 3), target=(1, 2, 3))), "coincide"),
             # every argument fine, but no terrain was loaded into this context
             (dict(), "terrain not loaded"), (dict(rgb=None), "terrain not loaded"), (dict(gbuf=None), "terrain not loaded")]
    for kw, word in cases:
        rc, msg = render(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert lib.gr_destroy(ctx) == 0


# ------------------------------------------------------------------ RecordVideo on a stub env
class _StubEnv:
    render_mode = "rgb_array"
    step_dt = 0.03

    def __init__(self, w=20, h=12):
        self.w, self.h, self.steps, self.renders, self.closed = w, h, 0, [], False
        self.episode_length_buf = np.zeros(4)

    @property
    def unwrapped(self):
        return self

    def step(self, action):
        self.steps += 1
        return ("obs", self.steps)

    def render(self):
        self.renders.append(self.steps)  # (rendered after step number `steps` returned)
        return np.full((self.h, self.w, 3), self.steps % 256, dtype=np.uint8)

    def close(self):
        self.closed = True


def _gif_frames(path):
    from PIL import Image

    im = Image.open(path)
    frames = []
    for k in range(im.n_frames):
        im.seek(k)
        frames.append(np.array(im.convert("RGB")))
    return im.size, frames


def test_record_video_triggers_lengths_and_names(tmp_path):
    env = _StubEnv()
    rv = record_video.RecordVideo(env, str(tmp_path / "v"), lambda s: s % 5 == 0 and s != 15, video_length=7)
    assert rv.unwrapped is env and rv.step_dt == 0.03
    rv.episode_length_buf = np.ones(4)  # forwarded to the env, like every attribute the wrapper does not own
    assert env.episode_length_buf[0] == 1.0 and "episode_length_buf" not in rv.__dict__
    for k in range(24):
        assert rv.step(None) == ("obs", k + 1)
    # step 0 fires: frames of steps 0-6 (step 5 fires inside the recording: ignored); step 10 fires: 10-16; step 15 is
    # excluded by the trigger, step 20 fires: 20-23 so far
    assert env.renders == [1, 2, 3, 4, 5, 6, 7] + list(range(11, 18)) + [21, 22, 23, 24]
    names = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "v" / "*")))
    assert names == ["rl-video-step-0.gif", "rl-video-step-10.gif"]
    size, frames = _gif_frames(str(tmp_path / "v" / "rl-video-step-10.gif"))
    assert size == (20, 12) and len(frames) == 7
    assert [int(f[0, 0, 0]) for f in frames] == list(range(11, 18))
    rv.close()  # the recording under way keeps its 4 frames
    assert env.closed and len(_gif_frames(str(tmp_path / "v" / "rl-video-step-20.gif"))[1]) == 4
    assert [os.path.basename(p) for p in rv.written] == names + ["rl-video-step-20.gif"]


def test_record_video_only_on_rank_0_and_needs_rgb_array(tmp_path):
    env = _StubEnv()
    rv = record_video.RecordVideo(env, str(tmp_path / "v"), lambda s: True, video_length=2, rank=1)
    for _ in range(4):
        rv.step(None)
    assert env.renders == [] and not os.path.exists(tmp_path / "v")
    env.render_mode = None
    with pytest.raises(ValueError, match="rgb_array"):
        record_video.RecordVideo(env, str(tmp_path / "w"), lambda s: True, video_length=2)


def test_record_video_ppm_fallback_without_pil(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "PIL", None)  # `from PIL import Image` now raises ImportError
    env = _StubEnv(w=6, h=4)
    rv = record_video.RecordVideo(env, str(tmp_path), lambda s: s == 1, video_length=3, name_prefix="clip")
    for _ in range(6):
        rv.step(None)
    folder = tmp_path / "clip-step-1"
    files = sorted(os.listdir(folder))
    assert files == ["frame_00000.ppm", "frame_00001.ppm", "frame_00002.ppm"]
    raw = open(folder / files[2], "rb").read()
    assert raw.startswith(b"P6 6 4 255\n") and raw[len(b"P6 6 4 255\n"):] == bytes([4]) * (6 * 4 * 3)


# ------------------------------------------------------------------ CLI and metadata
@pytest.mark.parametrize("script", ["train", "play"])
def test_launchers_accept_the_video_flags(script):
    import importlib.util

    path = os.path.join(ROOT, "standalone", "rsl_rl", f"{script}.py")
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location(f"_viewer_cli_{script}", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
    args = mod.build_parser().parse_args(["--video", "--video_env", "3", "--video_size", "320x240"])
    assert args.video and args.video_env == 3 and parse_size(args.video_size) == (320, 240)
    assert args.video_length == 200 and (script == "play" or args.video_interval == 2000)  # the reference's defaults
    assert not mod.build_parser().parse_args([]).video
    with pytest.raises(ValueError):
        parse_size("320")


def test_env_metadata_lists_rgb_array():
    from generalizableracing_amd.envs.racing_env import RacingEnv, RslRlVecEnvWrapper

    assert RacingEnv.metadata["render_modes"] == [None, "rgb_array"]
    assert callable(RacingEnv.render) and callable(RacingEnv.render_view) and callable(RslRlVecEnvWrapper.render)
