/*
 * gr_viewer.h — the RGB viewer (gr_view_render, gr_viewer.hip): what the depth camera's shared headers do not
 * have.  The rays, slots and hit functions are gr_camera.h's and gr_obstacles.h's, unchanged (an FPV g-buffer's
 * depth is the depth camera's bits); this header adds the third-person cameras, the surface normal of a hit and
 * the colour of a pixel.  Viewer only: the oracle does not include it.
 *
 * Cameras (env-local frame, z up; c0 / c1 / c2 = forward / left / up, the frame of gr_camera.h):
 *   FPV   gr_cam_pose of the env's sensor (offset of the enabled camera, else gr_camera_config_default's).
 *   CHASE h = (R00, R10) of the body rotation (the body x axis on the horizontal), normalised, (1, 0) when shorter
 *         than 1e-3; eye = p - back h + (0, 0, up), target = p + ahead h; then the look-at below, in fp32 on the
 *         device (gr_view_chase).
 *   FIXED eye / target from the view array; the look-at below in float64 on the host (gr_view_lookat64), rounded
 *         to fp32 once, so a test restates the basis bit for bit.
 *   look-at: c0 = (t - e) / |t - e|; l = (-c0y, c0x, 0), c1 = l / |l|, (0, 1, 0) when |l| < 1e-6 (looking straight
 *         up or down); c2 = c0 x c1 = (-c0z c1y, c0z c1x, c0x c1y - c0y c1x).
 *
 * G-buffer (GR_VIEW_GBUF_WORDS planes of [H][W] words): id, depth (the clipped distance to the image plane),
 * normal x / y / z (unit, env-local, outward from the solid; zero for a miss).  A hit at or beyond max_distance is a
 * miss.  Of equal nearest hits the lowest primitive index wins (the list order of a tile does not matter).
 *
 * Colour (every op fp32, no contraction; a test recomputes it from the g-buffer, the pixel's (a, b), the view's
 * camera, the env's gate_id and the hit obstacle's kind):
 *   sky   = HORIZON + clamp(b, 0, 1) * (ZENITH - HORIZON)
 *   base  = miss: sky.  ground: x = o + depth * ((c0 + a c1) + b c2), CHECK0 when floor(x.x) + floor(x.y) is even,
 *           else CHECK1.  gate: GATE, the env's next gate (id == 1 + gate_id) NEXT.  obstacle: KIND[kind].  drone: DRONE.
 *   shade = AMBIENT + (1 - AMBIENT) * max(n . LIGHT, 0)
 *   lit   = base * shade
 *   f     = (depth / max_distance)^2
 *   out   = lit + f * (sky - lit)           (a miss: out = sky)
 *   byte  = (int)(clamp(out, 0, 1) * 255 + 0.5)
 */
#ifndef GR_VIEWER_H
#define GR_VIEWER_H

#include "gr_camera.h"

#define GR_VIEW_HDR_FLOATS 32 /* scratch header: o, c0, c1, c2 (12 floats), ground z, then the ints below */
#define GR_VH_GZ 12
#define GR_VH_NG 16    /* (int) gates of the track */
#define GR_VH_NOB 17   /* (int) obstacles of the track */
#define GR_VH_NPRIM 18 /* (int) gates + obstacles (+ 1: the drone) */
#define GR_VH_NEXT 19  /* (int) the env's gate_id */
#define GR_VIEW_OSLOT 24 /* floats per obstacle slot: gr_cam_obst_setup's frame and primitive (0-15) and its window (17-21) */

#define GR_VIEW_LIGHT {0.36f, 0.48f, 0.8f}
#define GR_VIEW_AMBIENT 0.35f
#define GR_VIEW_HORIZON {0.80f, 0.86f, 0.94f}
#define GR_VIEW_ZENITH {0.35f, 0.55f, 0.85f}
#define GR_VIEW_CHECK0 {0.32f, 0.36f, 0.30f}
#define GR_VIEW_CHECK1 {0.46f, 0.50f, 0.42f}
#define GR_VIEW_GATE {0.90f, 0.45f, 0.10f}
#define GR_VIEW_NEXT {0.15f, 0.85f, 0.25f}
#define GR_VIEW_DRONE {0.95f, 0.85f, 0.10f}
/* obstacle kinds: box, cylinder, sphere, capsule */
#define GR_VIEW_KINDS {{0.62f, 0.60f, 0.58f}, {0.30f, 0.50f, 0.75f}, {0.75f, 0.30f, 0.35f}, {0.65f, 0.45f, 0.75f}}

/* look-at basis in fp32 (CHASE, on the device) */
GR_HD void gr_view_lookat(const float e[3], const float t[3], float c0[3], float c1[3], float c2[3]) {
  const float f[3] = {t[0] - e[0], t[1] - e[1], t[2] - e[2]};
  const float n = gr_sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
  for (int i = 0; i < 3; ++i) c0[i] = f[i] / n;
  const float h = gr_sqrtf(c0[0] * c0[0] + c0[1] * c0[1]);
  if (h < 1.0e-6f) {
    c1[0] = 0.0f;
    c1[1] = 1.0f;
  } else {
    c1[0] = -c0[1] / h;
    c1[1] = c0[0] / h;
  }
  c1[2] = 0.0f;
  c2[0] = -(c0[2] * c1[1]);
  c2[1] = c0[2] * c1[0];
  c2[2] = c0[0] * c1[1] - c0[1] * c1[0];
}

/* the same in float64 (FIXED, on the host); out = o, c0, c1, c2 as 12 floats */
static inline void gr_view_lookat64(const float e[3], const float t[3], float out[12]) {
  const double f[3] = {(double)t[0] - (double)e[0], (double)t[1] - (double)e[1], (double)t[2] - (double)e[2]};
  const double n = __builtin_sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
  const double c0[3] = {f[0] / n, f[1] / n, f[2] / n};
  const double h = __builtin_sqrt(c0[0] * c0[0] + c0[1] * c0[1]);
  double c1[3] = {0.0, 1.0, 0.0};
  if (!(h < 1.0e-6)) {
    c1[0] = -c0[1] / h;
    c1[1] = c0[0] / h;
  }
  const double c2[3] = {-(c0[2] * c1[1]), c0[2] * c1[0], c0[0] * c1[1] - c0[1] * c1[0]};
  for (int i = 0; i < 3; ++i) {
    out[i] = e[i];
    out[3 + i] = (float)c0[i];
    out[6 + i] = (float)c1[i];
    out[9 + i] = (float)c2[i];
  }
}

/* CHASE: eye and target from the body pose (R row-major, gr_cam_quat_matrix) */
GR_HD void gr_view_chase(const float p[3], const float R[9], float back, float up, float ahead, float e[3], float t[3]) {
  float hx = R[0], hy = R[3];
  const float n = gr_sqrtf(hx * hx + hy * hy);
  if (n < 1.0e-3f) {
    hx = 1.0f;
    hy = 0.0f;
  } else {
    hx = hx / n;
    hy = hy / n;
  }
  e[0] = p[0] - back * hx;
  e[1] = p[1] - back * hy;
  e[2] = p[2] + up;
  t[0] = p[0] + ahead * hx;
  t[1] = p[1] + ahead * hy;
  t[2] = p[2];
}

/* the drone as a GR_OBST_BOX record: centre p, rows of R^T (= columns of R), the collider's half extents */
GR_HD void gr_view_drone_record(const float p[3], const float R[9], const float half[3], float* r) {
  for (int i = 0; i < GR_OBST_FLOATS; ++i) r[i] = 0.0f;
  for (int i = 0; i < 3; ++i) {
    r[i] = p[i];
    r[4 + i] = R[3 * i];
    r[8 + i] = R[3 * i + 1];
    r[12 + i] = R[3 * i + 2];
  }
  r[7] = half[0];
  r[11] = half[1];
  r[15] = half[2];
  r[16] = (float)GR_OBST_BOX;
}

/* local hit point of pixel ray (a, b) at depth d: O + d (D0 + a D1 + b D2) (slot floats 0-11) */
GR_HD void gr_view_local(const float* s, float a, float b, float d, float l[3]) {
  for (int j = 0; j < 3; ++j)
    l[j] = gr_fmaf(d, gr_fmaf(b, s[GR_CS_D2 + j], gr_fmaf(a, s[GR_CS_D1 + j], s[GR_CS_D0 + j])), s[GR_CS_O + j]);
}

GR_HD float gr_view_sign(float x) { return x < 0.0f ? -1.0f : 1.0f; }

/* box: the face whose |l_i| / e_i is largest */
GR_HD void gr_view_box_normal(const float l[3], float e0, float e1, float e2, float n[3]) {
  const float q0 = gr_fabsf(l[0]) / e0, q1 = gr_fabsf(l[1]) / e1, q2 = gr_fabsf(l[2]) / e2;
  const int k = (q0 >= q1 && q0 >= q2) ? 0 : (q1 >= q2 ? 1 : 2);
  n[0] = n[1] = n[2] = 0.0f;
  n[k] = gr_view_sign(l[k]);
}

/* obstacle slot (gr_cam_obst_setup): local normal at the local hit point */
GR_HD void gr_view_obst_normal(const float* s, const float l[3], float n[3]) {
  const int kind = (int)s[GR_OS_KIND];
  const float e0 = s[GR_OS_E0], e1 = s[GR_OS_E1], e2 = s[GR_OS_E2];
  if (kind == GR_OBST_BOX) {
    gr_view_box_normal(l, e0, e1, e2, n);
    return;
  }
  float v[3] = {l[0], l[1], l[2]};
  if (kind == GR_OBST_CYLINDER) {
    const float rho = gr_sqrtf(l[0] * l[0] + l[1] * l[1]);
    if (gr_fabsf(gr_fabsf(l[2]) - e2) < gr_fabsf(rho - e0)) { /* nearer a cap than the side */
      n[0] = n[1] = 0.0f;
      n[2] = gr_view_sign(l[2]);
      return;
    }
    v[2] = 0.0f;
  } else if (kind == GR_OBST_CAPSULE) {
    v[2] = l[2] - gr_clampf(l[2], -e2, e2); /* radial from the segment */
  }
  const float m = gr_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const float im = m > 0.0f ? 1.0f / m : 0.0f;
  n[0] = v[0] * im;
  n[1] = v[1] * im;
  n[2] = v[2] * im;
}

/* gate slot (gr_cam_gate_setup): the outer face or the hole wall the hit lies on (the nearest of the five planes the
 * point can be on; a hole wall counts only within the other hole slab); a hole wall's normal points into the hole */
GR_HD void gr_view_gate_normal(const float* s, const float l[3], float n[3]) {
  const float ax = gr_fabsf(l[0]), ay = gr_fabsf(l[1]), az = gr_fabsf(l[2]);
  const float hw = s[GR_CS_HW], hh = s[GR_CS_HH];
  const float tol = 1.0e-4f;
  float best = gr_fabsf(ax - s[GR_CS_HOW]);
  int k = 0;
  float sg = gr_view_sign(l[0]);
  float r = gr_fabsf(ay - s[GR_CS_HOH]);
  if (r < best) { best = r; k = 1; sg = gr_view_sign(l[1]); }
  r = gr_fabsf(az - s[GR_CS_HT]);
  if (r < best) { best = r; k = 2; sg = gr_view_sign(l[2]); }
  r = gr_fabsf(ax - hw);
  if (ay <= hh + tol && r < best) { best = r; k = 0; sg = -gr_view_sign(l[0]); }
  r = gr_fabsf(ay - hh);
  if (ax <= hw + tol && r < best) { best = r; k = 1; sg = -gr_view_sign(l[1]); }
  n[0] = n[1] = n[2] = 0.0f;
  n[k] = sg;
}

/* local normal -> env-local frame: n_w = sum_k (D_k . n) c_k (the slot's D_k = M c_k, so M^T = C D^T) */
GR_HD void gr_view_normal_world(const float* s, const float nl[3], const float c0[3], const float c1[3],
                                const float c2[3], float nw[3]) {
  const float k0 = gr_cam_dot3(s + GR_CS_D0, nl), k1 = gr_cam_dot3(s + GR_CS_D1, nl), k2 = gr_cam_dot3(s + GR_CS_D2, nl);
  for (int i = 0; i < 3; ++i) nw[i] = (k0 * c0[i] + k1 * c1[i]) + k2 * c2[i];
}

/* pixel colour (the formula at the top).  cls: -1 miss, 0 ground, 1 gate, 2 next gate, 3 + kind obstacle, 7 drone */
#define GR_VIEW_CLS_MISS -1
#define GR_VIEW_CLS_GROUND 0
#define GR_VIEW_CLS_GATE 1
#define GR_VIEW_CLS_NEXT 2
#define GR_VIEW_CLS_OBST 3
#define GR_VIEW_CLS_DRONE 7
GR_HD void gr_view_colour(int cls, float depth, const float n[3], float a, float b, const float o[3], const float c0[3],
                          const float c1[3], const float c2[3], float max_distance, unsigned char rgb[3]) {
  const float L[3] = GR_VIEW_LIGHT, hz[3] = GR_VIEW_HORIZON, zn[3] = GR_VIEW_ZENITH;
  const float ck0[3] = GR_VIEW_CHECK0, ck1[3] = GR_VIEW_CHECK1, gt[3] = GR_VIEW_GATE, nx[3] = GR_VIEW_NEXT,
              dr[3] = GR_VIEW_DRONE;
  const float kinds[4][3] = GR_VIEW_KINDS;
  const float t = gr_clampf(b, 0.0f, 1.0f);
  float out[3];
  for (int i = 0; i < 3; ++i) out[i] = hz[i] + t * (zn[i] - hz[i]);
  if (cls != GR_VIEW_CLS_MISS) {
    float base[3];
    if (cls == GR_VIEW_CLS_GROUND) {
      const float x = o[0] + depth * ((c0[0] + a * c1[0]) + b * c2[0]);
      const float y = o[1] + depth * ((c0[1] + a * c1[1]) + b * c2[1]);
      const int odd = ((int)gr_floorf(x) + (int)gr_floorf(y)) & 1;
      for (int i = 0; i < 3; ++i) base[i] = odd ? ck1[i] : ck0[i];
    } else {
      for (int i = 0; i < 3; ++i)
        base[i] = cls == GR_VIEW_CLS_GATE ? gt[i] : cls == GR_VIEW_CLS_NEXT ? nx[i] : cls == GR_VIEW_CLS_DRONE
                                                                                          ? dr[i]
                                                                                          : kinds[(cls - GR_VIEW_CLS_OBST) & 3][i];
    }
    const float lam = gr_maxf((n[0] * L[0] + n[1] * L[1]) + n[2] * L[2], 0.0f);
    const float shade = GR_VIEW_AMBIENT + (1.0f - GR_VIEW_AMBIENT) * lam;
    float f = depth / max_distance;
    f = f * f;
    for (int i = 0; i < 3; ++i) {
      const float lit = base[i] * shade;
      out[i] = lit + f * (out[i] - lit);
    }
  }
  for (int i = 0; i < 3; ++i) rgb[i] = (unsigned char)(int)(gr_clampf(out[i], 0.0f, 1.0f) * 255.0f + 0.5f);
}

#if defined(__cplusplus) && (defined(__HIPCC__) || defined(__HIP__))
#include <hip/hip_runtime.h>
namespace gr {
struct ViewArgs {
  const float* state;    // [GR_NUM_PLANES][num_envs][4]
  const int32_t* istate; // [num_envs][4]
  const float* table;    // packed track table
  const float* obst;     // obstacle records (null: none)
  const int32_t* obst_counts;
  int max_obst, track_stride, num_levels, max_gates, num_envs;
  int env, mode, width, height;
  float fx, fy, cx, cy, max_distance;
  float back, up, ahead;
  float cam[12];    // FIXED: o, c0, c1, c2
  float off_p[3];   // FPV: the sensor's offset (gr_cam_const off_p, R_off)
  float R_off[9];
  float half[3];    // the collider's half extents (the drone box)
  float* scratch;   // header [GR_VIEW_HDR_FLOATS] | gate slots [max_gates][GR_CAM_SLOT] | obstacle slots
  float* gbuf;      // [GR_VIEW_GBUF_WORDS][H][W] or null
  unsigned char* rgb;  // [H][W][3] or null
};
// floats of the scratch for a context's maxima (one drone slot after the obstacles)
inline size_t view_scratch_floats(int max_gates, int max_obst) {
  return (size_t)GR_VIEW_HDR_FLOATS + (size_t)max_gates * GR_CAM_SLOT + ((size_t)max_obst + 1) * GR_VIEW_OSLOT;
}
hipError_t launch_view(const ViewArgs& a, hipStream_t s);  // gr_viewer.hip
}  // namespace gr
#endif

#endif /* GR_VIEWER_H */
