"""The RGB viewer restated in numpy (float64 by default), independently of csrc/gr_camera.h: plain ray / solid
algebra in the world (env-local) frame, one primitive at a time, vectorised over the pixels.

  cameras   camera_fpv / camera_chase / camera_fixed -> (o [3], C [3, 3] rows forward / left / up)
  rays      pixel (u, v) looks along C[0] + a_u C[1] + b_v C[2], a_u = (cx - (u + 0.5)) / fx, b_v likewise; the ray
            parameter is the distance to the image plane
  solids    gate = box minus an open prism through it, box, cylinder, sphere, capsule (a segment's offset surface),
            the ground plane; the first surface crossing with s > 0 (from inside a solid: its exit)
  trace()   nearest id, clipped depth, outward unit normal, and the second-nearest crossing
  ambiguity_mask()  the pixels whose answer a perturbation of 1e-3 pixel can change
  colour()  the documented colour formula (csrc/gr_viewer.h) in float32

`dtype=np.float32` evaluates the same algebra in float32: its error against float64 sizes the depth tolerance of
tests/test_gpu_viewer.py.
"""
import math

import numpy as np

ID_MISS, ID_GROUND, ID_DRONE = -1, 0, 1000000
BOX, CYLINDER, SPHERE, CAPSULE = 0, 1, 2, 3
FAR = np.inf


# ------------------------------------------------------------------ cameras
def quat_matrix(q):
    w, x, y, z = (float(t) for t in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def lookat(eye, target):
    """(o, C) of a camera at eye looking at target, z up.  The op order is that of gr_view_lookat64 (include/gr.h's
    GR_VIEW_FIXED), so float32(C) is the kernel's basis bit for bit."""
    e = np.asarray(eye, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    f = t - e
    n = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
    c0 = f / n
    h = np.sqrt(c0[0] * c0[0] + c0[1] * c0[1])
    c1 = np.array([0.0, 1.0, 0.0]) if h < 1e-6 else np.array([-c0[1] / h, c0[0] / h, 0.0])
    c2 = np.array([-(c0[2] * c1[1]), c0[2] * c1[0], c0[0] * c1[1] - c0[1] * c1[0]])
    return e, np.stack([c0, c1, c2])


def camera_fixed(eye, target):
    return lookat(eye, target)


def camera_chase(p, q, back=1.5, up=0.6, ahead=1.0):
    p = np.asarray(p, dtype=np.float64)
    R = quat_matrix(q)
    h = np.array([R[0, 0], R[1, 0]])
    n = np.hypot(h[0], h[1])
    h = np.array([1.0, 0.0]) if n < 1e-3 else h / n
    eye = np.array([p[0] - back * h[0], p[1] - back * h[1], p[2] + up])
    tgt = np.array([p[0] + ahead * h[0], p[1] + ahead * h[1], p[2]])
    f = tgt - eye
    c0 = f / np.linalg.norm(f)
    l = np.array([-c0[1], c0[0], 0.0])
    ln = np.linalg.norm(l)
    c1 = np.array([0.0, 1.0, 0.0]) if ln < 1e-6 else l / ln
    return eye, np.stack([c0, c1, np.cross(c0, c1)])


def camera_fpv(p, q, off_p, off_q):
    """Isaac Lab's combine_frame_transforms: o = p + R(q) off_p, axes = columns of R(q) R(off_q / |off_q|)."""
    R = quat_matrix(q)
    oq = np.asarray(off_q, dtype=np.float64)
    Rc = R @ quat_matrix(oq / np.linalg.norm(oq))
    return np.asarray(p, dtype=np.float64) + R @ np.asarray(off_p, dtype=np.float64), Rc.T.copy()


def ray_grid(fx, fy, cx, cy, width, height, dtype=np.float64):
    """(A, B) [H, W]: the tangents of every pixel, computed in `dtype` (float32: the kernel's own values)."""
    t = dtype
    a = (t(cx) - (np.arange(width, dtype=t) + t(0.5))) / t(fx)
    b = (t(cy) - (np.arange(height, dtype=t) + t(0.5))) / t(fy)
    return np.broadcast_to(a[None, :], (height, width)).copy(), np.broadcast_to(b[:, None], (height, width)).copy()


# ------------------------------------------------------------------ scene
def make_scene(gates, track_rec, obst_records=None, drone=None):
    """gates [G][20] / obst_records [K][20] in the GR_GATE_FLOATS / GR_OBST_FLOATS layouts (centre 0-2, rows of the
    world -> local rotation at 4-6 / 8-10 / 12-14, sizes at 7 / 11 / 15 (/ 16 / 17)); track_rec = (ground z, origin z,
    start gate, gate count); drone = (p, q, half extents) or None."""
    ng = int(track_rec[3])
    sc = {"gz": float(track_rec[0]), "gates": np.asarray(gates[:ng], dtype=np.float64),
          "obst": np.zeros((0, 20)) if obst_records is None else np.asarray(obst_records, dtype=np.float64),
          "drone": drone}
    return sc


def _frame(rec):
    return rec[0:3], np.stack([rec[4:7], rec[8:11], rec[12:15]])


def _local(rec, o, D, t):
    c, M = _frame(rec)
    ol = (M.astype(t) @ (o.astype(t) - c.astype(t))).astype(t)
    dl = np.einsum("jk,khw->jhw", M.astype(t), D).astype(t)
    return ol, dl, M


def _slab(ol, dl, e, t):
    """entry / exit parameters of |x| <= e along ol + s dl (elementwise; a ray parallel to the slab is inside it
    everywhere or nowhere)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (t(-e) - ol) / dl
        t2 = (t(e) - ol) / dl
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par = dl == 0
    inside = abs(ol) <= e
    lo = np.where(par, -np.inf if inside else np.inf, lo)
    hi = np.where(par, np.inf if inside else -np.inf, hi)
    return lo, hi


def _quadratic(A, Bh, Cc):
    """roots of A s^2 + 2 Bh s + Cc = 0 as (lo, hi); (inf, -inf) without real roots"""
    disc = Bh * Bh - A * Cc
    ok = (disc >= 0) & (A > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = np.sqrt(np.where(ok, disc, 0))
        lo = np.where(ok, (-Bh - sq) / A, np.inf)
        hi = np.where(ok, (-Bh + sq) / A, -np.inf)
    return lo, hi


def _first(lo, hi):
    """first crossing with s > 0 of the interval [lo, hi] and whether it is the exit"""
    ok = (lo <= hi) & (hi > 0)
    ex = lo <= 0
    return np.where(ok, np.where(ex, hi, lo), np.inf), ex & ok


def _unit(v):
    n = np.sqrt((v * v).sum(axis=0))
    return v / np.where(n > 0, n, 1)


def _axis_normal(l, e, sign=1.0):
    """unit axis normal of the axis whose |l_i| / e_i is largest (e: the candidate axes' half sizes)"""
    q = np.stack([np.abs(l[i]) / e[i] for i in range(len(e))])
    k = np.argmax(q, axis=0)
    n = np.zeros((3,) + l.shape[1:], dtype=l.dtype)
    for i in range(len(e)):
        n[i] = np.where(k == i, sign * np.where(l[i] < 0, -1.0, 1.0), 0.0)
    return n


def _hit_box(ol, dl, e, t):
    lo = np.full(dl.shape[1:], -np.inf, dtype=t)
    hi = np.full(dl.shape[1:], np.inf, dtype=t)
    for j in range(3):
        a, b = _slab(ol[j], dl[j], e[j], t)
        lo, hi = np.maximum(lo, a), np.minimum(hi, b)
    s, _ = _first(lo, hi)
    l = ol[:, None, None] + np.where(np.isfinite(s), s, 0) * dl
    return s, _axis_normal(l, e)


def _hit_sphere(ol, dl, r, t):
    A = (dl * dl).sum(axis=0)
    Bh = (ol[:, None, None] * dl).sum(axis=0)
    Cc = (ol * ol).sum() - t(r) * t(r)
    s, _ = _first(*_quadratic(A, Bh, Cc))
    l = ol[:, None, None] + np.where(np.isfinite(s), s, 0) * dl
    return s, _unit(l)


def _hit_cylinder(ol, dl, r, hh, t):
    zlo, zhi = _slab(ol[2], dl[2], hh, t)
    A = dl[0] * dl[0] + dl[1] * dl[1]
    Bh = ol[0] * dl[0] + ol[1] * dl[1]
    Cc = ol[0] * ol[0] + ol[1] * ol[1] - t(r) * t(r)
    rlo, rhi = _quadratic(A, Bh, Cc)
    par = A < 1e-12  # parallel to the axis: inside the radius everywhere or nowhere
    rlo = np.where(par, -np.inf if Cc <= 0 else np.inf, rlo)
    rhi = np.where(par, np.inf if Cc <= 0 else -np.inf, rhi)
    lo, hi = np.maximum(zlo, rlo), np.minimum(zhi, rhi)
    s, ex = _first(lo, hi)
    cap = np.where(ex, zhi < rhi, zlo > rlo)
    l = ol[:, None, None] + np.where(np.isfinite(s), s, 0) * dl
    side = _unit(np.stack([l[0], l[1], np.zeros_like(l[2])]))
    capn = np.stack([np.zeros_like(l[2]), np.zeros_like(l[2]), np.where(l[2] < 0, -1.0, 1.0)])
    return s, np.where(cap, capn, side)


def _hit_capsule(ol, dl, r, hs, t):
    """the union of the cylinder |z| <= hs and the two end spheres, as intervals along the ray: from outside the
    nearest entry, from inside the exit of the connected run of intervals around the origin"""
    ivs = []
    zlo, zhi = _slab(ol[2], dl[2], hs, t)
    A = dl[0] * dl[0] + dl[1] * dl[1]
    rlo, rhi = _quadratic(A, ol[0] * dl[0] + ol[1] * dl[1], ol[0] * ol[0] + ol[1] * ol[1] - t(r) * t(r))
    par = A < 1e-12
    inr = ol[0] * ol[0] + ol[1] * ol[1] <= t(r) * t(r)
    rlo = np.where(par, -np.inf if inr else np.inf, rlo)
    rhi = np.where(par, np.inf if inr else -np.inf, rhi)
    ivs.append((np.maximum(zlo, rlo), np.minimum(zhi, rhi)))
    AA = (dl * dl).sum(axis=0)
    for zc in (hs, -hs):
        oc = ol - np.array([0, 0, zc], dtype=t)
        ivs.append(_quadratic(AA, (oc[:, None, None] * dl).sum(axis=0), (oc * oc).sum() - t(r) * t(r)))
    ivs = [(np.where(lo <= hi, lo, np.inf), np.where(lo <= hi, hi, -np.inf)) for lo, hi in ivs]
    inside = np.zeros(dl.shape[1:], dtype=bool)
    for lo, hi in ivs:
        inside |= (lo <= 0) & (hi > 0)
    ent = np.full(dl.shape[1:], np.inf, dtype=t)
    for lo, hi in ivs:
        ent = np.minimum(ent, np.where((lo > 0), lo, np.inf))
    ext = np.zeros(dl.shape[1:], dtype=t)
    for _ in range(3):
        for lo, hi in ivs:
            ext = np.where((lo <= ext) & (hi > ext), hi, ext)
    s = np.where(inside, ext, ent)
    l = ol[:, None, None] + np.where(np.isfinite(s), s, 0) * dl
    v = np.stack([l[0], l[1], l[2] - np.clip(l[2], -hs, hs)])
    return s, _unit(v)


def _hit_gate(ol, dl, hw, hh, ht, how, hoh, t):
    """box {|x| <= how, |y| <= hoh, |z| <= ht} minus the open prism {|x| < hw, |y| < hh}: the first parameter at
    which the ray crosses the solid's surface.  Candidates: the box interval's ends (on the surface unless inside the
    prism there) and the prism interval's ends (on the surface when strictly inside the box interval)."""
    lo = np.full(dl.shape[1:], -np.inf, dtype=t)
    hi = np.full(dl.shape[1:], np.inf, dtype=t)
    for j, e in enumerate((how, hoh, ht)):
        a, b = _slab(ol[j], dl[j], e, t)
        lo, hi = np.maximum(lo, a), np.minimum(hi, b)
    plo = np.full(dl.shape[1:], -np.inf, dtype=t)
    phi = np.full(dl.shape[1:], np.inf, dtype=t)
    for j, e in enumerate((hw, hh)):
        a, b = _slab(ol[j], dl[j], e, t)
        plo, phi = np.maximum(plo, a), np.minimum(phi, b)
    box = lo <= hi
    prism = plo < phi
    best = np.full(dl.shape[1:], np.inf, dtype=t)
    wall = np.zeros(dl.shape[1:], dtype=bool)
    for c in (lo, hi):
        ok = box & (c > 0) & ~(prism & (c > plo) & (c < phi))
        best = np.where(ok & (c < best), c, best)
    for c in (plo, phi):
        ok = box & prism & (c > 0) & (c > lo) & (c < hi)
        take = ok & (c < best)
        best = np.where(take, c, best)
        wall |= take
    l = ol[:, None, None] + np.where(np.isfinite(best), best, 0) * dl
    return best, np.where(wall, _axis_normal(l[:2], (hw, hh), sign=-1.0), _axis_normal(l, (how, hoh, ht)))


def trace(scene, o, C, A, B, max_distance, dtype=np.float64):
    """-> ids int32 [H, W], depth [H, W] (clipped), normal [3, H, W] (zero for a miss), best and second [H, W]: the
    nearest and second-nearest crossings (inf when there is none), all evaluated in `dtype`."""
    t = dtype
    o = np.asarray(o).astype(t)
    C = np.asarray(C).astype(t)
    A, B = np.asarray(A).astype(t), np.asarray(B).astype(t)
    D = (C[0][:, None, None] + A[None] * C[1][:, None, None] + B[None] * C[2][:, None, None]).astype(t)
    shape = A.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        sg = (t(scene["gz"]) - o[2]) / D[2]
    best = np.where(sg > 0, sg, np.inf).astype(t)
    ids = np.where(np.isfinite(best), ID_GROUND, ID_MISS).astype(np.int32)
    nrm = np.zeros((3,) + shape, dtype=t)
    nrm[2] = np.where(np.isfinite(best), 1.0, 0.0)
    second = np.full(shape, np.inf, dtype=t)

    def merge(s, n_local, M, pid):
        nonlocal best, ids, nrm, second
        s = np.where(np.isnan(s), np.inf, s).astype(t)
        nw = np.einsum("kj,khw->jhw", M.astype(t), n_local.astype(t))
        take = s < best
        second = np.where(take, best, np.minimum(second, s))
        best = np.where(take, s, best)
        ids = np.where(take, pid, ids)
        nrm = np.where(take, nw, nrm)

    ng = len(scene["gates"])
    for g, rec in enumerate(scene["gates"]):
        ol, dl, M = _local(rec, o, D, t)
        s, n = _hit_gate(ol, dl, rec[7], rec[11], rec[15], rec[16], rec[17], t)
        merge(s, n, M, 1 + g)
    prims = [(1 + ng + k, rec) for k, rec in enumerate(scene["obst"])]
    if scene["drone"] is not None:
        p, q, half = scene["drone"]
        rec = np.zeros(20)
        rec[0:3] = p
        Rt = quat_matrix(q).T
        rec[4:7], rec[8:11], rec[12:15] = Rt[0], Rt[1], Rt[2]
        rec[7], rec[11], rec[15], rec[16] = half[0], half[1], half[2], BOX
        prims.append((ID_DRONE, rec))
    for pid, rec in prims:
        ol, dl, M = _local(rec, o, D, t)
        kind, e = int(rec[16]), (rec[7], rec[11], rec[15])
        if kind == BOX:
            s, n = _hit_box(ol, dl, e, t)
        elif kind == SPHERE:
            s, n = _hit_sphere(ol, dl, e[0], t)
        elif kind == CYLINDER:
            s, n = _hit_cylinder(ol, dl, e[0], e[2], t)
        else:
            s, n = _hit_capsule(ol, dl, e[0], e[2], t)
        merge(s, n, M, pid)
    hit = best < t(max_distance)
    ids = np.where(hit, ids, ID_MISS).astype(np.int32)
    nrm = np.where(hit, nrm, 0.0)
    depth = np.where(hit, best, t(max_distance)).astype(t)
    return ids, depth, nrm, np.where(hit, best, np.inf), second


def ambiguity_mask(scene, o, C, A, B, max_distance, pitch_a, pitch_b):
    """Pixels whose float64 answer is not robust: a ray displaced by +-1e-3 of a pixel's pitch in a or in b gets
    another id or a normal more than 1e-3 away, or the two nearest crossings lie within 1e-5 relative."""
    ids, _, nrm, best, second = trace(scene, o, C, A, B, max_distance)
    with np.errstate(invalid="ignore"):
        amb = np.isfinite(second) & np.isfinite(best) & (second - best <= 1e-5 * np.abs(best))
    # (a hit next to the clip distance: the displaced rays decide through the id)
    for da, db in ((1e-3 * pitch_a, 0), (-1e-3 * pitch_a, 0), (0, 1e-3 * pitch_b), (0, -1e-3 * pitch_b)):
        i2, _, n2, _, _ = trace(scene, o, C, A + da, B + db, max_distance)
        amb |= (i2 != ids) | (np.abs(n2 - nrm).max(axis=0) > 1e-3)
    return amb


# ------------------------------------------------------------------ colour (float32, the documented formula)
LIGHT = np.array([0.36, 0.48, 0.8], dtype=np.float32)
AMBIENT = np.float32(0.35)
HORIZON = np.array([0.80, 0.86, 0.94], dtype=np.float32)
ZENITH = np.array([0.35, 0.55, 0.85], dtype=np.float32)
CHECK = np.array([[0.32, 0.36, 0.30], [0.46, 0.50, 0.42]], dtype=np.float32)
GATE = np.array([0.90, 0.45, 0.10], dtype=np.float32)
NEXT = np.array([0.15, 0.85, 0.25], dtype=np.float32)
DRONE = np.array([0.95, 0.85, 0.10], dtype=np.float32)
KINDS = np.array([[0.62, 0.60, 0.58], [0.30, 0.50, 0.75], [0.75, 0.30, 0.35], [0.65, 0.45, 0.75]], dtype=np.float32)


def colour(ids, depth, normal, A, B, o, C, max_distance, num_gates, gate_id, obst_kinds):
    """uint8 [H, W, 3] from a g-buffer (ids, depth, normal), the pixels' float32 tangents, the view's float32 camera,
    the track's gate count, the env's next gate and the kinds of the track's obstacles.  Every op float32, in the
    kernel's order."""
    f32 = np.float32
    ids = np.asarray(ids)
    depth, normal = np.asarray(depth, dtype=f32), np.asarray(normal, dtype=f32)
    A, B = np.asarray(A, dtype=f32), np.asarray(B, dtype=f32)
    o, C = np.asarray(o, dtype=f32), np.asarray(C, dtype=f32)
    t = np.clip(B, f32(0), f32(1))
    sky = HORIZON[:, None, None] + t[None] * (ZENITH - HORIZON)[:, None, None]
    x = o[0] + depth * ((C[0, 0] + A * C[1, 0]) + B * C[2, 0])
    y = o[1] + depth * ((C[0, 1] + A * C[1, 1]) + B * C[2, 1])
    odd = (np.floor(x).astype(np.int64) + np.floor(y).astype(np.int64)) & 1
    base = np.where(odd[None] == 1, CHECK[1][:, None, None], CHECK[0][:, None, None])
    is_gate = (ids >= 1) & (ids <= num_gates)
    base = np.where(is_gate[None], GATE[:, None, None], base)
    base = np.where((is_gate & (ids == 1 + gate_id))[None], NEXT[:, None, None], base)
    is_ob = (ids > num_gates) & (ids != ID_DRONE)
    if len(obst_kinds):
        k = np.asarray(obst_kinds, dtype=np.int64)[np.clip(ids - 1 - num_gates, 0, len(obst_kinds) - 1)] & 3
        base = np.where(is_ob[None], np.moveaxis(KINDS[k], -1, 0), base)
    base = np.where((ids == ID_DRONE)[None], DRONE[:, None, None], base).astype(f32)
    lam = np.maximum((normal[0] * LIGHT[0] + normal[1] * LIGHT[1]) + normal[2] * LIGHT[2], f32(0))
    shade = AMBIENT + (f32(1) - AMBIENT) * lam
    fog = depth / f32(max_distance)
    fog = fog * fog
    lit = base * shade[None]
    out = lit + fog[None] * (sky - lit)
    out = np.where((ids == ID_MISS)[None], sky, out).astype(f32)
    byte = (np.clip(out, f32(0), f32(1)) * f32(255) + f32(0.5)).astype(np.int32)
    return np.moveaxis(byte, 0, -1).astype(np.uint8)


# ------------------------------------------------------------------ the views both test files use
SHARED_TYPE, SHARED_LEVEL = 3, 2  # the track (terrain column, row) of the default 20 x 10 terrain they look at
SHARED_TRACK = SHARED_TYPE * 10 + SHARED_LEVEL


def start_pose(gates, track_rec):
    """(p, q): a level pose 2 m from the track's start gate on the gate's axis (the gate frame's z, projected to the
    horizontal), heading along that axis."""
    g = np.asarray(gates[int(track_rec[2])], dtype=np.float64)
    n = g[12:15].copy()
    n[2] = 0.0
    n = n / np.linalg.norm(n)
    p = g[0:3] - 2.0 * n
    yaw = math.atan2(n[1], n[0])
    return p, np.array([math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw)])


def shared_views(gates, track_rec):
    """[(name, mode, width, height, fov_deg, max_distance, eye, target)] for a track: the views of
    test_gbuffer_matches_float64_restatement and of the CPU test that bounds their ambiguity masks."""
    ng = int(track_rec[3])
    c = np.asarray(gates[:ng, 0:3], dtype=np.float64).mean(axis=0)
    gz = float(track_rec[0])
    p, _ = start_pose(gates, track_rec)
    g0 = np.asarray(gates[int(track_rec[2]), 0:3], dtype=np.float64)
    return [
        ("fixed_top_16", "fixed", 16, 16, 120.0, 60.0, (c[0] - 8.0, c[1] - 6.0, gz + 12.0), (c[0], c[1], gz + 1.0)),
        ("fixed_side_40x30", "fixed", 40, 30, 90.0, 40.0, (p[0] - 2.0, p[1] + 1.5, p[2] + 1.5), tuple(g0)),
        ("fixed_96x72", "fixed", 96, 72, 90.0, 40.0, (c[0] + 6.0, c[1] - 9.0, gz + 4.0), (c[0], c[1], gz + 1.0)),
        ("chase_40x30", "chase", 40, 30, 90.0, 40.0, None, None),
        ("chase_96x72", "chase", 96, 72, 90.0, 40.0, None, None),
    ]


def intrinsics(width, height, fov_deg):
    """(fx, fy, cx, cy) as float32, the values viewer.view_array puts into the view array."""
    f = np.float32(0.5 * height / math.tan(math.radians(0.5 * fov_deg)))
    return f, f, np.float32(0.5 * width), np.float32(0.5 * height)
