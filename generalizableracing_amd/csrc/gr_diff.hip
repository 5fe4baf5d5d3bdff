// gr_diff.hip — BPTT through the analytic step for MI355X (gfx950): the reference's second training workflow
// (standalone/diff_rl: algorithms/bptt.py, ManagerBasedDiffRLEnv.step's losses, DroneDynamics.align) as two small
// read-only launches around gr_step, which write a tape, and one reverse-time adjoint launch per window.
//
//   diff_record_kernel   before gr_step: replays the controller and the integrator from the pre-step planes (the
//                        default plant of the step kernel IS DroneDynamics.step) and writes the step's tape row
//   diff_loss_kernel     after gr_step: the three loss terms on the row's x+ against the env's current gate centre
//   diff_backward_kernel one lane per env, t = T-1 .. 0, the adjoints of (p, q, v, w_b, T, tau) in registers
//
// Tape: per step GR_DIFF_PLANES float4 planes of [num_envs] (gr.h GR_DT_*): every lane's access is 16 bytes and
// coalesced.  The arithmetic is gr_diff.h's.  None of this touches gr_step or the planes it writes.
#include <hip/hip_runtime.h>

#include "../../include/gr.h"
#include "gr_diff.h"
#include "gr_kernels.h"

namespace gr {

#define DIFF_BLOCK 64  // one wave per workgroup: a window of 4 096 envs spreads over 64 CUs

namespace {

__device__ __forceinline__ void unpack_env(const float4 s0, const float4 s1, const float4 s2, const float4 s3,
                                           const float4 s4, const float4 u, const float4 r0, const float4 r1,
                                           const float4 p0, const float4 p1, const float4 p2, const float4 p3,
                                           gr_diff_env& e) {
  e.p[0] = s0.x; e.p[1] = s0.y; e.p[2] = s0.z; e.q[0] = s0.w;
  e.q[1] = s1.x; e.q[2] = s1.y; e.q[3] = s1.z; e.v[0] = s1.w;
  e.v[1] = s2.x; e.v[2] = s2.y; e.w[0] = s2.z; e.w[1] = s2.w;
  e.w[2] = s3.x; e.al[0] = s3.y; e.al[1] = s3.z; e.al[2] = s3.w;
  e.T = s4.x; e.tau[0] = s4.y; e.tau[1] = s4.z; e.tau[2] = s4.w;
  e.u[0] = u.x; e.u[1] = u.y; e.u[2] = u.z; e.u[3] = u.w;
  e.thr = r0.x; e.k2[0] = r0.z; e.k2[1] = r0.w;
  e.k2[2] = r1.x; e.k1[0] = r1.y; e.k1[1] = r1.z; e.k1[2] = r1.w;
  e.Kp[0] = p0.x; e.Kp[1] = p0.y; e.Kp[2] = p0.z; e.cT = p0.w;
  e.Kd[0] = p1.x; e.Kd[1] = p1.y; e.Kd[2] = p1.z; e.mp = p1.w;
  e.ct[0] = p2.x; e.ct[1] = p2.y; e.ct[2] = p2.z; e.mc = p2.w;
  e.J[0] = p3.x; e.J[1] = p3.y; e.J[2] = p3.z;
}

}  // namespace

__global__ __launch_bounds__(DIFF_BLOCK) void diff_record_kernel(gr_diff_consts k, const float4* __restrict__ S,
                                                                 const float4* __restrict__ actions,
                                                                 float4* __restrict__ row) {
  const int i = blockIdx.x * DIFF_BLOCK + threadIdx.x;
  const int n = k.num_envs;
  if (i >= n) return;
  const size_t N = (size_t)n;
  // every plane load is issued before the first use
  const float4 s0 = S[GR_P_POSQ * N + i], s1 = S[GR_P_QV * N + i], s2 = S[GR_P_VW * N + i], s3 = S[GR_P_WA * N + i];
  const float4 s4 = S[GR_P_CTRL * N + i], r0 = S[GR_P_RST0 * N + i], r1 = S[GR_P_RST1 * N + i];
  const float4 p0 = S[GR_P_PAR0 * N + i], p1 = S[GR_P_PAR1 * N + i], p2 = S[GR_P_PAR2 * N + i];
  const float4 p3 = S[GR_P_PAR3 * N + i];
  float4 u;
  if (k.lag) {
    u = S[GR_P_LAG * N + i];  // tanh(a_{t-1}): the lag buffer is kept squashed
  } else {
    const float4 a = actions[i];
    u = make_float4(gr_tanhf(a.x), gr_tanhf(a.y), gr_tanhf(a.z), gr_tanhf(a.w));
  }
  gr_diff_env e;
  unpack_env(s0, s1, s2, s3, s4, u, r0, r1, p0, p1, p2, p3, e);
  float tt[4];
  gr_diff_forward(k, e, tt);
  row[GR_DT_POSQ * N + i] = s0;
  row[GR_DT_QV * N + i] = s1;
  row[GR_DT_VW * N + i] = s2;
  row[GR_DT_WA * N + i] = s3;
  row[GR_DT_CTRL * N + i] = s4;
  row[GR_DT_U * N + i] = u;
  row[GR_DT_RST0 * N + i] = r0;
  row[GR_DT_RST1 * N + i] = r1;
  row[GR_DT_PAR0 * N + i] = p0;
  row[GR_DT_PAR1 * N + i] = p1;
  row[GR_DT_PAR2 * N + i] = p2;
  row[GR_DT_PAR3 * N + i] = p3;
  row[GR_DT_TT * N + i] = make_float4(tt[0], tt[1], tt[2], tt[3]);
  row[GR_DT_XP0 * N + i] = make_float4(e.p[0], e.p[1], e.p[2], e.q[0]);
  row[GR_DT_XP1 * N + i] = make_float4(e.q[1], e.q[2], e.q[3], e.v[0]);
  row[GR_DT_XP2 * N + i] = make_float4(e.v[1], e.v[2], e.w[0], e.w[1]);
  row[GR_DT_XP3 * N + i] = make_float4(e.w[2], 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(DIFF_BLOCK) void diff_loss_kernel(gr_diff_consts k, const int4* __restrict__ istate,
                                                               const long long* __restrict__ dones,
                                                               const float* __restrict__ gates, float4* __restrict__ row,
                                                               float* __restrict__ loss, float* __restrict__ terms) {
  const int i = blockIdx.x * DIFF_BLOCK + threadIdx.x;
  const int n = k.num_envs;
  if (i >= n) return;
  const size_t N = (size_t)n;
  const int4 ii = istate[i];
  const float4 x0 = row[GR_DT_XP0 * N + i], x1 = row[GR_DT_XP1 * N + i], x2 = row[GR_DT_XP2 * N + i];
  const long long dn = dones[i];
  // the gate the env flies at after this step's reset and command update; indices clamped into the table
  int gate = ii.w & 0xff, lvl = (ii.w >> 8) & 0xff, type = (ii.w >> 24) & 0xff;
  gate = min(gate, k.max_gates - 1);
  lvl = min(lvl, k.num_levels - 1);
  type = min(type, k.num_types - 1);
  const float* gr = gates + ((size_t)(type * k.num_levels + lvl) * k.max_gates + gate) * GR_GATE_FLOATS;
  const float g[3] = {gr[0], gr[1], gr[2]};
  const float pp[3] = {x0.x, x0.y, x0.z}, vp[3] = {x1.w, x2.x, x2.y};
  float t3[3];
  gr_diff_loss_terms(k, pp, vp, g, t3);
  loss[i] = (t3[0] + t3[1]) + t3[2];
  terms[3 * (size_t)i + 0] = t3[0];
  terms[3 * (size_t)i + 1] = t3[1];
  terms[3 * (size_t)i + 2] = t3[2];
  row[GR_DT_GOAL * N + i] = make_float4(g[0], g[1], g[2], dn != 0 ? 1.0f : 0.0f);
}

// the planes of one tape row the reverse sweep reads
struct DiffRow {
  float4 s0, s1, s2, s3, s4, u, r0, r1, p0, p1, p2, p3, x0, x1, x2, gl;
};
__global__ __launch_bounds__(DIFF_BLOCK) void diff_backward_kernel(gr_diff_consts k, const float4* __restrict__ tape,
                                                                   int T, float scale, float4* __restrict__ grad) {
  const int i = blockIdx.x * DIFF_BLOCK + threadIdx.x;
  const unsigned n = (unsigned)k.num_envs;
  if (i >= (int)n) return;
  const unsigned rowv = GR_DIFF_PLANES * n;  // float4 per tape row
  auto fetch = [&](int t, DiffRow& r) {
    const float4* b = tape + ((unsigned)t * rowv + (unsigned)i);
    r.s0 = b[GR_DT_POSQ * n]; r.s1 = b[GR_DT_QV * n]; r.s2 = b[GR_DT_VW * n]; r.s3 = b[GR_DT_WA * n];
    r.s4 = b[GR_DT_CTRL * n]; r.u = b[GR_DT_U * n]; r.r0 = b[GR_DT_RST0 * n]; r.r1 = b[GR_DT_RST1 * n];
    r.p0 = b[GR_DT_PAR0 * n]; r.p1 = b[GR_DT_PAR1 * n]; r.p2 = b[GR_DT_PAR2 * n]; r.p3 = b[GR_DT_PAR3 * n];
    r.x0 = b[GR_DT_XP0 * n]; r.x1 = b[GR_DT_XP1 * n]; r.x2 = b[GR_DT_XP2 * n]; r.gl = b[GR_DT_GOAL * n];
  };
  gr_diff_adj a;
  for (int j = 0; j < 3; ++j) { a.p[j] = 0.0f; a.v[j] = 0.0f; a.w[j] = 0.0f; a.tau[j] = 0.0f; }
  for (int j = 0; j < 4; ++j) a.q[j] = 0.0f;
  a.T = 0.0f;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (k.lag) grad[(unsigned)(T - 1) * n + i] = zero;  // no step of the window applies the last action
  DiffRow cur, nxt;
  fetch(T - 1, nxt);
  for (int t = T - 1; t >= 0; --t) {
    cur = nxt;
    if (t > 0) fetch(t - 1, nxt);  // row t - 1 is in flight while row t computes
    gr_diff_env e;
    unpack_env(cur.s0, cur.s1, cur.s2, cur.s3, cur.s4, cur.u, cur.r0, cur.r1, cur.p0, cur.p1, cur.p2, cur.p3, e);
    const float pp[3] = {cur.x0.x, cur.x0.y, cur.x0.z}, qp[4] = {cur.x0.w, cur.x1.x, cur.x1.y, cur.x1.z};
    const float vp[3] = {cur.x1.w, cur.x2.x, cur.x2.y}, g[3] = {cur.gl.x, cur.gl.y, cur.gl.z};
    float ga[4];
    gr_diff_backward(k, e, pp, qp, vp, g, cur.gl.w != 0.0f, scale, a, ga);
    const int r = t - k.lag;  // under the lag step t applied the action of step t - 1 (step 0's is from before the window)
    if (r >= 0) grad[(unsigned)r * n + i] = make_float4(ga[0], ga[1], ga[2], ga[3]);
  }
}

hipError_t launch_diff_record(const gr_diff_consts& k, const float* state, const float* actions, float* row,
                              hipStream_t s) {
  const int nb = (k.num_envs + DIFF_BLOCK - 1) / DIFF_BLOCK;
  hipLaunchKernelGGL(diff_record_kernel, dim3(nb), dim3(DIFF_BLOCK), 0, s, k, reinterpret_cast<const float4*>(state),
                     reinterpret_cast<const float4*>(actions), reinterpret_cast<float4*>(row));
  return hipGetLastError();
}

hipError_t launch_diff_loss(const gr_diff_consts& k, const int32_t* istate, const int64_t* dones, const float* gates,
                            float* row, float* loss, float* terms, hipStream_t s) {
  const int nb = (k.num_envs + DIFF_BLOCK - 1) / DIFF_BLOCK;
  hipLaunchKernelGGL(diff_loss_kernel, dim3(nb), dim3(DIFF_BLOCK), 0, s, k, reinterpret_cast<const int4*>(istate),
                     reinterpret_cast<const long long*>(dones), gates, reinterpret_cast<float4*>(row), loss, terms);
  return hipGetLastError();
}

hipError_t launch_diff_backward(const gr_diff_consts& k, const float* tape, int T, float scale, float* grad,
                                hipStream_t s) {
  const int nb = (k.num_envs + DIFF_BLOCK - 1) / DIFF_BLOCK;
  hipLaunchKernelGGL(diff_backward_kernel, dim3(nb), dim3(DIFF_BLOCK), 0, s, k, reinterpret_cast<const float4*>(tape),
                     T, scale, reinterpret_cast<float4*>(grad));
  return hipGetLastError();
}

}  // namespace gr
