// gr_viewer.hip — the RGB viewer (gr_view_render): one frame of one env from an arbitrary pinhole camera at an
// arbitrary resolution, for gfx950.  Rays, slots and hits are the depth camera's (gr_camera.h, gr_obstacles.h);
// cameras, normals and colour are gr_viewer.h's.
//
// Two launches.  view_setup_kernel: one lane per primitive of the env's track (gates, obstacles, in the third-person
// modes the drone as a box) sets its slot up in the context's scratch, every lane from the same camera; lane 0 also
// writes the header (camera, ground height, counts).  view_render_kernel: one 256-thread workgroup per 16 x 16 pixel
// tile culls the slots against the tile's (a, b) range into an LDS list (room for every primitive: one tile can see
// them all), then each lane runs its pixel's hits over the list and keeps the nearest hit's index.  The nearest-hit
// minimum is exact in any order and ties go to the lowest index, so the frame does not depend on the list's order.
// Plain stores, no atomics on the image.  Not a hot path of training: launched only when a frame is asked for.
#include "gr_viewer.h"

namespace gr {

namespace {

struct ViewCam {
  float o[3], c0[3], c1[3], c2[3];
};

// the view's camera from the env's pose (every lane of the set-up computes the same one)
__device__ __forceinline__ void view_camera(const ViewArgs& a, const float p[3], const float R[9], const float q[4],
                                            ViewCam& c) {
  if (a.mode == GR_VIEW_FIXED) {
    for (int i = 0; i < 3; ++i) {
      c.o[i] = a.cam[i];
      c.c0[i] = a.cam[3 + i];
      c.c1[i] = a.cam[6 + i];
      c.c2[i] = a.cam[9 + i];
    }
  } else if (a.mode == GR_VIEW_CHASE) {
    float t[3];
    gr_view_chase(p, R, a.back, a.up, a.ahead, c.o, t);
    gr_view_lookat(c.o, t, c.c0, c.c1, c.c2);
  } else {
    // gr_cam_pose's expressions on the sensor's offset (the depth camera's pose, bit for bit)
    for (int i = 0; i < 3; ++i) {
      const float r0 = R[3 * i], r1 = R[3 * i + 1], r2 = R[3 * i + 2];
      c.o[i] = p[i] + gr_fmaf(r2, a.off_p[2], gr_fmaf(r1, a.off_p[1], r0 * a.off_p[0]));
      c.c0[i] = gr_fmaf(r2, a.R_off[6], gr_fmaf(r1, a.R_off[3], r0 * a.R_off[0]));
      c.c1[i] = gr_fmaf(r2, a.R_off[7], gr_fmaf(r1, a.R_off[4], r0 * a.R_off[1]));
      c.c2[i] = gr_fmaf(r2, a.R_off[8], gr_fmaf(r1, a.R_off[5], r0 * a.R_off[2]));
    }
  }
}

__device__ __forceinline__ float* gate_slot(float* scratch, int g) {
  return scratch + GR_VIEW_HDR_FLOATS + (size_t)g * GR_CAM_SLOT;
}
__device__ __forceinline__ float* obst_slot(float* scratch, int max_gates, int k) {
  return scratch + GR_VIEW_HDR_FLOATS + (size_t)max_gates * GR_CAM_SLOT + (size_t)k * GR_VIEW_OSLOT;
}

}  // namespace

__global__ __launch_bounds__(64) void view_setup_kernel(ViewArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  const int N = a.num_envs, i = a.env, G = a.max_gates;
  const float4 posq = reinterpret_cast<const float4*>(a.state)[(size_t)GR_P_POSQ * N + i];
  const float4 qv = reinterpret_cast<const float4*>(a.state)[(size_t)GR_P_QV * N + i];
  const float pos[3] = {posq.x, posq.y, posq.z}, q[4] = {posq.w, qv.x, qv.y, qv.z};
  float R[9];
  gr_cam_quat_matrix(q, R);
  ViewCam c;
  view_camera(a, pos, R, q, c);
  const int packed = a.istate[4 * i + GR_I_PACKED];
  const int track = ((packed >> 24) & 0xff) * a.num_levels + ((packed >> 8) & 0xff);
  const float* tb = a.table + (size_t)track * a.track_stride;
  const float* rec = tb + G * GR_GATE_FLOATS;
  int ng = (int)rec[3];
  ng = ng < 0 ? 0 : (ng > G ? G : ng);
  int nob = a.obst ? a.obst_counts[track] : 0;
  nob = nob < 0 ? 0 : (nob > a.max_obst ? a.max_obst : nob);
  const int drone = a.mode != GR_VIEW_FPV;
  const int nprim = ng + nob + drone;
  if (p == 0) {
    float* h = a.scratch;
    for (int k = 0; k < 3; ++k) {
      h[k] = c.o[k];
      h[3 + k] = c.c0[k];
      h[6 + k] = c.c1[k];
      h[9 + k] = c.c2[k];
    }
    h[GR_VH_GZ] = rec[0];
    int* hi = reinterpret_cast<int*>(h);
    hi[GR_VH_NG] = ng;
    hi[GR_VH_NOB] = nob;
    hi[GR_VH_NPRIM] = nprim;
    hi[GR_VH_NEXT] = packed & 0xff;
  }
  if (p >= nprim) return;
  float s[GR_CAM_SLOT];
  if (p < ng) {
    gr_cam_gate_setup(tb + p * GR_GATE_FLOATS, c.o, c.c0, c.c1, c.c2, a.max_distance, s);
    float* dst = gate_slot(a.scratch, p);
    for (int k = 0; k < GR_CAM_SLOT; ++k) dst[k] = s[k];
    return;
  }
  float r[GR_OBST_FLOATS];
  if (p < ng + nob) {
    const float* src = a.obst + ((size_t)track * a.max_obst + (size_t)(p - ng)) * GR_OBST_FLOATS;
    for (int k = 0; k < GR_OBST_FLOATS; ++k) r[k] = src[k];
  } else {
    gr_view_drone_record(pos, R, a.half, r);
  }
  gr_cam_obst_setup(r, c.o, c.c0, c.c1, c.c2, a.max_distance, s);
  float* dst = obst_slot(a.scratch, G, p - ng);
  for (int k = 0; k < GR_VIEW_OSLOT; ++k) dst[k] = s[k];
}

__global__ __launch_bounds__(256) void view_render_kernel(ViewArgs a) {
  extern __shared__ int s_list[];  // [max_gates + max_obst + 1] primitives that may cover a pixel of this tile
  __shared__ int s_n;
  const float* hdr = a.scratch;
  const int* hdri = reinterpret_cast<const int*>(hdr);
  float o[3], c0[3], c1[3], c2[3];
  for (int k = 0; k < 3; ++k) {
    o[k] = hdr[k];
    c0[k] = hdr[3 + k];
    c1[k] = hdr[6 + k];
    c2[k] = hdr[9 + k];
  }
  const float gz = hdr[GR_VH_GZ], maxd = a.max_distance;
  const int ng = hdri[GR_VH_NG], nob = hdri[GR_VH_NOB], nprim = hdri[GR_VH_NPRIM], next = hdri[GR_VH_NEXT];
  const int W = a.width, H = a.height, G = a.max_gates;
  const int u0 = blockIdx.x * 16, v0 = blockIdx.y * 16;
  const int u1 = u0 + 15 < W ? u0 + 15 : W - 1, v1 = v0 + 15 < H ? v0 + 15 : H - 1;
  // a_u, b_v decrease with u, v
  const float a_hi = gr_cam_tan(a.cx, a.fx, u0), a_lo = gr_cam_tan(a.cx, a.fx, u1);
  const float b_hi = gr_cam_tan(a.cy, a.fy, v0), b_lo = gr_cam_tan(a.cy, a.fy, v1);
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < nprim; p += 256) {
    const float* s = p < ng ? gate_slot(a.scratch, p) : obst_slot(a.scratch, G, p - ng);
    bool meet = s[GR_CS_VALID] != 0.0f && !(s[GR_CS_AMAX] < a_lo || s[GR_CS_AMIN] > a_hi || s[GR_CS_BMAX] < b_lo ||
                                            s[GR_CS_BMIN] > b_hi);
    if (meet) meet = p < ng ? !gr_cam_gate_outside(s, a_lo, a_hi, b_lo, b_hi) : !gr_cam_obst_outside(s, a_lo, a_hi, b_lo, b_hi);
    if (meet) s_list[atomicAdd(&s_n, 1)] = p;  // (LDS; at most nprim entries)
  }
  __syncthreads();
  const int u = u0 + (threadIdx.x & 15), v = v0 + (threadIdx.x >> 4);
  if (u >= W || v >= H) return;
  const float ra = gr_cam_tan(a.cx, a.fx, u), rb = gr_cam_tan(a.cy, a.fy, v);
  const float dz = gr_fmaf(rb, c2[2], gr_fmaf(ra, c1[2], c0[2]));
  float best = gr_cam_ground_hit(o[2], gz, dz);
  int bp = -1;  // -1: the ground (or nothing), else the primitive
  const int n = s_n;
  for (int k = 0; k < n; ++k) {
    const int p = s_list[k];
    const float* s = p < ng ? gate_slot(a.scratch, p) : obst_slot(a.scratch, G, p - ng);
    if (!(ra >= s[GR_CS_AMIN] && ra <= s[GR_CS_AMAX] && rb >= s[GR_CS_BMIN] && rb <= s[GR_CS_BMAX])) continue;
    const float d = p < ng ? gr_cam_gate_hit(s, ra, rb) : gr_cam_obst_hit(s, ra, rb);
    if (d < best || (d == best && d < GR_CAM_FAR && bp >= 0 && p < bp)) {
      best = d;
      bp = p;
    }
  }
  const float depth = gr_cam_clip(best, maxd);
  const bool hit = best < maxd;
  int id = GR_VIEW_ID_MISS, cls = GR_VIEW_CLS_MISS;
  float nw[3] = {0.0f, 0.0f, 0.0f};
  if (hit) {
    if (bp < 0) {
      id = GR_VIEW_ID_GROUND;
      cls = GR_VIEW_CLS_GROUND;
      nw[2] = 1.0f;
    } else {
      const float* s = bp < ng ? gate_slot(a.scratch, bp) : obst_slot(a.scratch, G, bp - ng);
      float l[3], nl[3];
      gr_view_local(s, ra, rb, best, l);
      if (bp < ng) {
        gr_view_gate_normal(s, l, nl);
        cls = bp == next ? GR_VIEW_CLS_NEXT : GR_VIEW_CLS_GATE;
        id = 1 + bp;
      } else {
        gr_view_obst_normal(s, l, nl);
        const bool drone = bp == ng + nob;
        cls = drone ? GR_VIEW_CLS_DRONE : GR_VIEW_CLS_OBST + ((int)s[GR_OS_KIND] & 3);
        id = drone ? GR_VIEW_ID_DRONE : 1 + bp;
      }
      gr_view_normal_world(s, nl, c0, c1, c2, nw);
    }
  }
  const size_t npix = (size_t)W * H, pix = (size_t)v * W + u;
  if (a.gbuf) {
    reinterpret_cast<int*>(a.gbuf)[GR_VIEW_G_ID * npix + pix] = id;
    a.gbuf[GR_VIEW_G_DEPTH * npix + pix] = depth;
    a.gbuf[(GR_VIEW_G_NORMAL + 0) * npix + pix] = nw[0];
    a.gbuf[(GR_VIEW_G_NORMAL + 1) * npix + pix] = nw[1];
    a.gbuf[(GR_VIEW_G_NORMAL + 2) * npix + pix] = nw[2];
  }
  if (a.rgb) {
    unsigned char c[3];
    gr_view_colour(cls, depth, nw, ra, rb, o, c0, c1, c2, maxd, c);
    a.rgb[3 * pix] = c[0];
    a.rgb[3 * pix + 1] = c[1];
    a.rgb[3 * pix + 2] = c[2];
  }
}

hipError_t launch_view(const ViewArgs& a, hipStream_t s) {
  const int nmax = a.max_gates + a.max_obst + 1;
  const size_t lds = (size_t)nmax * sizeof(int);
  if (lds > 60000) return hipErrorInvalidValue;
  hipLaunchKernelGGL(view_setup_kernel, dim3((nmax + 63) / 64), dim3(64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(view_render_kernel, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace gr
