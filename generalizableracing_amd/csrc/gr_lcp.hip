// gr_lcp.hip — the Lipschitz-constrained-policy gradient penalty of PPOLCP and its gradient as whole-network
// fp32-MFMA passes over the actor (gr_lcp_forward / gr_lcp_backward, include/gr.h).
//
// Reference: PPOLCP._calc_grad_penalty (standalone/rsl_rl/ext/algorithms/ppo_lcp.py:105-108):
//   P = mean_rows | d sum(log pi(a | x)) / dx |^2
// through torch's double backward.  For the actor x -> z1 = W1 x + b1 -> h1 = lrelu(z1) -> z2 = W2 h1 + b2 ->
// h2 = lrelu(z2) -> mu = W3 h2 + b3 with a state-independent std, LeakyReLU's second derivative is zero, so both
// the penalty and its gradient are first-order chains over the activation masks D = (z > 0 ? 1 : slope) the
// forward already saved (the sign of h1 is the sign of z1):
//   lcp_fwd : delta = (a - mu) / std^2;  v2 = D2 (W3^T delta);  v1 = D1 (W2^T v2);  g = W1^T v1;  P = mean |g|^2
//             (mlp_bwd's chain with gy := delta, continued one layer to the input), 32-row tiles, the wave's W2
//             columns in registers.  g's contraction over the hidden units is split over the waves (each wave's v1
//             accumulator tile is directly the B operand) and summed in wave order through LDS.
//   lcp_bwd : with gb = (2 c / rows) g (c = dloss/dP, a device scalar):  s1 = D1 (W1 gb);  s2 = D2 (W2 s1);
//             dbar = W3 s2;  dmu = -dbar / std^2;  dstd = sum -2 delta dbar / std;  gW1 = v1^T gb;  gW3 = delta^T s2
//             (mlp_fwd's chain with x := gb, no biases, a mask multiply where the activation was; the small weight
//             gradients on MFMA contracting over the tile's rows as in mlp_bwd), one partial row per workgroup.
//   gW2 = v2^T s1 is mlp_wgrad (gr_mlp.hip) on (gz2 := v2, h1 := s1); lcp_final sums every partial in a fixed order.
// No atomics; every sum has a fixed order, so the results are bit-reproducible.  The MFMA fragment convention,
// the fragment helpers, the tile geometry (MW waves, BE-row tiles) and what these passes share with gr_mlp.hip's:
// gr_mfma.h.
#include <hip/hip_runtime.h>

#include "../../include/gr.h"
#include "gr_kernels.h"
#include "gr_mfma.h"

namespace gr {
namespace lcp {

constexpr int L_BLOCKS = 256;  // persistent workgroups (one per CU)

struct Args {
  const float* mu;   // [rows][ld_mu], first k columns
  const float* act;  // [rows][ld_act], first k columns
  const float* std;  // [k]
  const float* h1;   // [rows][H]
  const float* z2;   // [rows][H]
  const float* w1;   // [H][d]
  const float* w2;   // [H][H]
  const float* w3;   // [k][H]
  float* g;          // [rows][d]
  float* v1;         // [rows][H]
  float* v2;         // [rows][H]
  float* s1;         // [rows][H] (backward)
  const float* g_pen;  // [1] (backward)
  float* dmu;        // [rows][k] (backward)
  float* part;       // per-workgroup partials
  int rows, ld_mu, ld_act, d, k;
  float slope;
};

// per-workgroup partial row of the backward (floats): [gW1 (H d) | gW3 (k H) | dstd (k)], padded to 4
__host__ __device__ constexpr int bwd_row(int h, int d, int k) { return (h * d + k * h + k + 3) & ~3; }

// delta rows of the tile -> LDS [BE][4] (rows past the end and outputs >= k: 0, so they add nothing anywhere)
__device__ __forceinline__ void stage_delta(const Args& a, int base, float* dls) {
  if (threadIdx.x < BE * 4) {
    const int row = threadIdx.x >> 2, kk = threadIdx.x & 3;
    const int r = base + row;
    float v = 0.0f;
    if (r < a.rows && kk < a.k) {
      const float s = a.std[kk];
      v = (a.act[r * a.ld_act + kk] - a.mu[r * a.ld_mu + kk]) / (s * s);
    }
    dls[threadIdx.x] = v;
  }
}

// ------------------------------------------------------------------------------------------------ penalty pass
// LDS (floats): v2 [BE][H + 4], delta [BE][4], g partials [MW][BE][16 DT], the workgroup's |g|^2 sums [MW]
constexpr size_t fwd_lds_bytes(int h, int dt) { return 4 * ((size_t)BE * (h + 4) + BE * 4 + MW * BE * 16 * dt + MW); }

template <int H, int DT>
__global__ __launch_bounds__(MW * 64) void lcp_fwd(Args a) {
  constexpr int TW = H / (16 * MW);
  constexpr int Q = H / 16;
  constexpr int HP = H + 4;
  constexpr int XW = 16 * DT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int n = a.rows;  // (gr_lcp_* check rows * max(H, ld) < 2^31: 32-bit offsets)
  const int D = a.d, K = a.k;
  const float slope = a.slope;
  extern __shared__ float lds[];
  float* v2s = lds;                   // [BE][HP]
  float* dls = v2s + BE * HP;         // [BE][4]
  float* gps = dls + BE * 4;          // [MW][BE][XW]
  float* red = gps + MW * BE * XW;    // [MW]
  const float* __restrict__ W1 = a.w1;
  const float* __restrict__ W2 = a.w2;
  const float* __restrict__ W3 = a.w3;

  // A operands (as mlp_bwd): row j of tile t is hidden unit 16 (wave TW + t) + j of h1
  float w2c[TW][4 * Q], w3a[TW];
  // g^T = W1^T v1^T over the wave's units: row j = input 16 dt + j, k step r of tile t = unit 16 (wave TW + t) + 4 g + r
  float w1a[TW][DT][4];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    load_w2_column<H>(W2, W3, K, 16 * (wave * TW + t) + j, g, w2c[t], w3a[t]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int dcol = 16 * dt + j;
        w1a[t][dt][r] = dcol < D ? W1[(size_t)(16 * (wave * TW + t) + 4 * g + r) * D + dcol] : 0.0f;
      }
  }
  float psum = 0.0f;

  const int stride = gridDim.x * BE;
  for (int base = blockIdx.x * BE; base < n; base += stride) {
    stage_delta(a, base, dls);
    __syncthreads();  // (1) delta staged; the previous tile's readers of v2s / gps are done
    // ---- v2 = (delta W3) lrelu'(z2)
#pragma unroll
    for (int c = 0; c < BC; ++c) {
      const int r = base + 16 * c + j;
      const int rr = r < n ? r : n - 1;
      const float dv = dls[(16 * c + j) * 4 + g];  // B[k = g][row j]
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const int u = 16 * (wave * TW + t) + 4 * g;
        const m4 gh = mf(w3a[t], dv, zero4());
        const m4 z = ld4(a.z2 + rr * H + u);
        m4 gz;
#pragma unroll
        for (int q = 0; q < 4; ++q) gz[q] = gh[q] * lrelu_d(z[q], slope);
        st4(v2s + (16 * c + j) * HP + u, gz);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // (2) v2 of the tile in LDS
    // ---- gh1 = v2 W2 for the wave's h1 units, all rows of the tile
    m4 acc[TW][BC];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int c = 0; c < BC; ++c) acc[t][c] = zero4();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      m4 gb[BC];
#pragma unroll
      for (int c = 0; c < BC; ++c) gb[c] = ld4(v2s + (16 * c + j) * HP + 16 * q + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int c = 0; c < BC; ++c) acc[t][c] = mf(w2c[t][4 * q + r], gb[c][r], acc[t][c]);
      __builtin_amdgcn_sched_barrier(0);  // (no hoisting of later fragments' loads: registers)
    }
    // ---- v1 = gh1 lrelu'(h1) -> global (lane (g, j): units 16 t' + 4 g .. + 3 of row 16 c + j)
#pragma unroll
    for (int c = 0; c < BC; ++c) {
      const int r = base + 16 * c + j;
      const int rr = r < n ? r : n - 1;
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const int u = 16 * (wave * TW + t) + 4 * g;
        const m4 hv = ld4(a.h1 + rr * H + u);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][c][q] *= lrelu_d(hv[q], slope);
        if (r < n) st4(a.v1 + r * H + u, acc[t][c]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // v2 rows -> global (coalesced rows)
    if (4 * lane < H) {
#pragma unroll
      for (int rr = 0; rr < BE / MW; ++rr) {
        const int row = wave + MW * rr;
        if (base + row < n) st4(a.v2 + (base + row) * H + 4 * lane, ld4(v2s + row * HP + 4 * lane));
      }
    }
    // ---- the wave's part of g^T = W1^T v1^T: C rows = inputs 16 dt + 4 g + q, col j = row 16 c + j
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int c = 0; c < BC; ++c) {
        m4 gp = zero4();
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) gp = mf(w1a[t][dt][r], acc[t][c][r], gp);
        st4(gps + (size_t)(wave * BE + 16 * c + j) * XW + 16 * dt + 4 * g, gp);
      }
    __syncthreads();  // (3) the 8 waves' partials of g in LDS
    if (threadIdx.x < BE * (XW / 4)) {
      const int row = threadIdx.x / (XW / 4), c4 = 4 * (threadIdx.x % (XW / 4));
      m4 v = ld4(gps + (size_t)row * XW + c4);
#pragma unroll
      for (int w = 1; w < MW; ++w) v += ld4(gps + (size_t)(w * BE + row) * XW + c4);
      const int r = base + row;
      if (r < n && c4 < D) {
        st4(a.g + r * D + c4, v);
        psum += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
    }
  }
  // ---- the workgroup's sum of |g|^2 (fixed butterfly order, then the waves in order)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) psum += __shfl_xor(psum, off);
  if (lane == 0) red[wave] = psum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = red[0];
#pragma unroll
    for (int w = 1; w < MW; ++w) v += red[w];
    a.part[blockIdx.x] = v;
  }
}

// penalty[0] = (sum of the workgroups' partials, in a fixed order) / rows
__global__ __launch_bounds__(64) void lcp_penalty(const float* __restrict__ part, int blocks, int rows,
                                                   float* __restrict__ penalty) {
  float v = 0.0f;
  for (int b = threadIdx.x; b < blocks; b += 64) v += part[b];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  if (threadIdx.x == 0) penalty[0] = v / (float)rows;
}

// ------------------------------------------------------------------------------------------------ gradient pass
// LDS (floats): s1 then s2 [BE][H + 4], v1 [BE][H + 4], layer-3 partials [MW][BE][4], delta [BE][4], dstd sums [2][4]
constexpr size_t bwd_lds_bytes(int h) { return 4 * ((size_t)2 * BE * (h + 4) + MW * BE * 4 + BE * 4 + 8); }

template <int H, int DT>
__global__ __launch_bounds__(MW * 64) void lcp_bwd(Args a, int row_floats) {
  constexpr int TW = H / (16 * MW);
  constexpr int Q = H / 16;
  constexpr int HP = H + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int n = a.rows;  // (gr_lcp_* check rows * max(H, ld) < 2^31: 32-bit offsets)
  const int D = a.d, K = a.k;
  const float slope = a.slope;
  // gb = (2 c / rows) g: the scale applied where g is read
  const float scale = 2.0f * a.g_pen[0] / (float)n;
  extern __shared__ float lds[];
  float* s1s = lds;                     // [BE][HP]: s1, then s2
  float* v1s = s1s + BE * HP;           // [BE][HP]
  float* parts = v1s + BE * HP;         // [MW][BE][4]
  float* dls = parts + MW * BE * 4;     // [BE][4]
  float* red = dls + BE * 4;            // [2][4]
  const float* __restrict__ W1 = a.w1;
  const float* __restrict__ W2 = a.w2;
  const float* __restrict__ W3 = a.w3;

  // A operands (as mlp_fwd): layer 1 / 2 row j of tile t = unit 16 (wave TW + t) + j, k order over the inputs / the
  // h1 units; layer 3 rows = outputs (j < K), k = the wave's units
  float w1r[TW][DT][4], w2r[TW][4 * Q], w3r[TW][4];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int row = 16 * (wave * TW + t) + j;
#pragma unroll
    for (int q = 0; q < DT; ++q) {
      const int k = 16 * q + 4 * g;
      const m4 v0 = ld4(W1 + (size_t)row * D + (k < D ? k : 0));
      const m4 v = k < D ? v0 : zero4();
#pragma unroll
      for (int r = 0; r < 4; ++r) w1r[t][q][r] = v[r];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const m4 v = ld4(W2 + (size_t)row * H + 16 * q + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) w2r[t][4 * q + r] = v[r];
    }
    const m4 v3l = ld4(W3 + (size_t)(j < K ? j : 0) * H + 16 * (wave * TW + t) + 4 * g);
    const m4 v3 = j < K ? v3l : zero4();
#pragma unroll
    for (int r = 0; r < 4; ++r) w3r[t][r] = v3[r];
  }
  m4 gw1[TW][DT], gw3[TW];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    gw3[t] = zero4();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) gw1[t][dt] = zero4();
  }
  float dstd = 0.0f;  // threads < BE * 4: output kk = threadIdx.x & 3

  const int stride = gridDim.x * BE;
  for (int base = blockIdx.x * BE; base < n; base += stride) {
    stage_delta(a, base, dls);
    // v1 rows of the tile -> LDS (coalesced rows; past the end: 0, so they add nothing to gW1)
    if (4 * lane < H) {
#pragma unroll
      for (int rr = 0; rr < BE / MW; ++rr) {
        const int row = wave + MW * rr;
        const int r = base + row;
        const m4 v = ld4(a.v1 + (r < n ? r : n - 1) * H + 4 * lane);
        st4(v1s + row * HP + 4 * lane, r < n ? v : zero4());
      }
    }
    // ---- layer 1: s1 = (gb W1^T) lrelu'(h1) for the wave's units -> LDS [row][unit]
    m4 acc[TW][BC];
#pragma unroll
    for (int c = 0; c < BC; ++c) {
      const int r = base + 16 * c + j;
      const int rr = r < n ? r : n - 1;
      m4 xo[DT];
#pragma unroll
      for (int q = 0; q < DT; ++q) {
        const int k = 16 * q + 4 * g;
        const m4 v = ld4(a.g + rr * D + (k < D ? k : 0));
        xo[q] = k < D ? v * scale : zero4();
      }
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        m4 s = zero4();
#pragma unroll
        for (int kk = 0; kk < 4 * DT; ++kk) s = mf(w1r[t][kk >> 2][kk & 3], xo[kk >> 2][kk & 3], s);
        const int u = 16 * (wave * TW + t) + 4 * g;
        const m4 hv = ld4(a.h1 + rr * H + u);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] *= lrelu_d(hv[q], slope);
        st4(s1s + (16 * c + j) * HP + u, s);
      }
    }
    __syncthreads();  // (A) s1, v1 and delta of the tile in LDS
    // s1 rows -> global for mlp_wgrad (coalesced rows)
    if (4 * lane < H) {
#pragma unroll
      for (int rr = 0; rr < BE / MW; ++rr) {
        const int row = wave + MW * rr;
        if (base + row < n) st4(a.s1 + (base + row) * H + 4 * lane, ld4(s1s + row * HP + 4 * lane));
      }
    }
    // ---- layer 2: s2 = (s1 W2^T) lrelu'(z2) for the wave's units
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int c = 0; c < BC; ++c) acc[t][c] = zero4();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      m4 hb[BC];
#pragma unroll
      for (int c = 0; c < BC; ++c) hb[c] = ld4(s1s + (16 * c + j) * HP + 16 * q + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int c = 0; c < BC; ++c) acc[t][c] = mf(w2r[t][4 * q + r], hb[c][r], acc[t][c]);
      __builtin_amdgcn_sched_barrier(0);  // (no hoisting of later fragments' loads: registers)
    }
#pragma unroll
    for (int c = 0; c < BC; ++c) {
      const int r = base + 16 * c + j;
      const int rr = r < n ? r : n - 1;
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const m4 z = ld4(a.z2 + rr * H + 16 * (wave * TW + t) + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][c][q] *= lrelu_d(z[q], slope);
      }
    }
    // ---- layer 3 partial over the wave's units -> LDS (C rows = outputs 4 g + q, col j = row)
#pragma unroll
    for (int c = 0; c < BC; ++c) {
      m4 o = zero4();
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o = mf(w3r[t][r], acc[t][c][r], o);
      if (g == 0) st4(parts + (size_t)(wave * BE + 16 * c + j) * 4, o);
    }
    // ---- gW1 += v1^T gb: rows = the wave's units, cols = inputs (DT tiles of 16), k step = rows 4 s + g
#pragma unroll 4
    for (int s = 0; s < BE / 4; ++s) {
      const int row = 4 * s + g;
      int r = base + row;
      r = r < n ? r : n - 1;  // (the tail rows' v1 is 0)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int dcol = 16 * dt + j;
        const float xv = dcol < D ? a.g[r * D + dcol] * scale : 0.0f;
#pragma unroll
        for (int t = 0; t < TW; ++t) gw1[t][dt] = mf(v1s[row * HP + 16 * (wave * TW + t) + j], xv, gw1[t][dt]);
      }
    }
    __syncthreads();  // (B) every wave is done with s1 (layer 2); the layer-3 partials are complete
    // s2 -> LDS, over s1
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int c = 0; c < BC; ++c) st4(s1s + (16 * c + j) * HP + 16 * (wave * TW + t) + 4 * g, acc[t][c]);
    // dbar = W3 s2 (the waves' partials in wave order) -> dmu = -dbar / std^2, dstd += -2 delta dbar / std
    if (threadIdx.x < BE * 4) {
      const int row = threadIdx.x >> 2, kk = threadIdx.x & 3;
      float v = parts[row * 4 + kk];
#pragma unroll
      for (int w = 1; w < MW; ++w) v += parts[(size_t)(w * BE + row) * 4 + kk];
      const int r = base + row;
      if (r < n && kk < K) {
        const float sd = a.std[kk];
        a.dmu[r * K + kk] = -v / (sd * sd);
        dstd += -2.0f * dls[threadIdx.x] * v / sd;
      }
    }
    __syncthreads();  // (C) s2 of the tile in LDS
    // ---- gW3 += delta^T s2: rows = outputs (j < 4), k step = rows 4 s + g
#pragma unroll 4
    for (int s = 0; s < BE / 4; ++s) {
      const int row = 4 * s + g;
      const float av = j < 4 ? dls[row * 4 + j] : 0.0f;
#pragma unroll
      for (int t = 0; t < TW; ++t) gw3[t] = mf(av, s1s[row * HP + 16 * (wave * TW + t) + j], gw3[t]);
    }
    __syncthreads();  // (D) every wave is done with the tile's LDS
  }
  // ---- the workgroup's partial row [gW1 | gW3 | dstd]
  float* pr = a.part + (size_t)blockIdx.x * (size_t)row_floats;
#pragma unroll
  for (int t = 0; t < TW; ++t) store_gw1_gw3<H, DT>(pr, H * D, 16 * (wave * TW + t), D, K, g, j, gw1[t], gw3[t]);
  // dstd: waves 0 and 1 hold it, output kk = lane & 3 (fixed butterfly over the lanes of one output, then the waves)
  if (wave < 2) {
    float v = dstd;
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) v += __shfl_xor(v, off);
    if (lane < 4) red[wave * 4 + lane] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4 && (int)threadIdx.x < K) pr[H * D + K * H + threadIdx.x] = red[threadIdx.x] + red[4 + threadIdx.x];
}

// grads = [gW1 (H d) | gW2 (H H) | gW3 (k H)], dstd [k]: element e is the fixed-order sum of its partials (the
// backward's partial rows [gW1 | gW3 | dstd]; mlp_wgrad's split partials for gW2).  As mlp_final: a lane owns 4
// consecutive elements, the 4 waves of a workgroup take every 4th partial row and are summed in wave order.
constexpr int LF_WAVES = 4;
__global__ __launch_bounds__(LF_WAVES * 64) void lcp_final(const float* __restrict__ bpart, int bwd_rows, int bwd_ld,
                                                          const float* __restrict__ wpart, int splits, int H, int D,
                                                          int K, float* __restrict__ grads, float* __restrict__ dstd) {
  __shared__ m4 sm[LF_WAVES * 64];
  const int n_small = H * D + K * H + K;
  const int q_small = (n_small + 3) / 4, q_total = q_small + H * H / 4;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane;
  const float* src = nullptr;
  int rows = 0, ldr = 0;
  if (q < q_small) {
    src = bpart + 4 * q;
    rows = bwd_rows;
    ldr = bwd_ld;
  } else if (q < q_total) {
    src = wpart + 4 * (size_t)(q - q_small);
    rows = splits;
    ldr = H * H;
  }
  sm[threadIdx.x] = partial_rows_sum<LF_WAVES>(src, rows, ldr, wv);
  __syncthreads();
  if (wv == 0 && src) {
    m4 t = sm[lane];
#pragma unroll
    for (int w = 1; w < LF_WAVES; ++w) t += sm[w * 64 + lane];
    if (q < q_small) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * q + r;
        if (e < H * D) grads[e] = t[r];
        else if (e < H * D + K * H) grads[H * H + e] = t[r];
        else if (e < n_small) dstd[e - H * D - K * H] = t[r];
      }
    } else {
      const int f = 4 * (q - q_small);
#pragma unroll
      for (int r = 0; r < 4; ++r) grads[H * D + f + r] = t[r];
    }
  }
}

static int grid_x(long long rows) {
  const long long t = (rows + BE - 1) / BE;
  return t < L_BLOCKS ? (t < 1 ? 1 : (int)t) : L_BLOCKS;
}

template <int H, int DT>
static hipError_t launch_fwd_t(const Args& a, hipStream_t s) {
  return launch_lds<lcp_fwd<H, DT>>(dim3(grid_x(a.rows)), dim3(MW * 64), fwd_lds_bytes(H, DT), s, a);
}

template <int H, int DT>
static hipError_t launch_bwd_t(const Args& a, int row, hipStream_t s) {
  return launch_lds<lcp_bwd<H, DT>>(dim3(grid_x(a.rows)), dim3(MW * 64), bwd_lds_bytes(H), s, a, row);
}

}  // namespace lcp

// scratch (floats) of either pass: the forward's per-workgroup sums; the backward's partial rows (d <= 32, k <= 4)
// and mlp_wgrad's split partials
int64_t lcp_scratch_floats(long long rows, int hidden) {
  const int64_t bwd = (int64_t)lcp::grid_x(rows) * lcp::bwd_row(hidden, 32, 4);
  return bwd + (int64_t)mlp_wgrad_splits(rows, hidden, 1) * hidden * hidden;
}

static lcp::Args lcp_args(const float* mu, long long ld_mu, const float* act, long long ld_act, const float* std,
                          const float* h1, const float* z2, const float* w1, const float* w2, const float* w3,
                          long long rows, int d, int k, float slope) {
  lcp::Args a = {};
  a.mu = mu, a.act = act, a.std = std, a.h1 = h1, a.z2 = z2, a.w1 = w1, a.w2 = w2, a.w3 = w3;
  a.rows = (int)rows, a.ld_mu = (int)ld_mu, a.ld_act = (int)ld_act, a.d = d, a.k = k, a.slope = slope;
  return a;
}

hipError_t launch_lcp_forward(const float* mu, long long ld_mu, const float* act, long long ld_act, const float* std,
                              const float* h1, const float* z2, const float* w1, const float* w2, const float* w3,
                              long long rows, int hidden, int d, int k, float slope, float* g, float* v1, float* v2,
                              float* scratch, float* penalty, hipStream_t s) {
  lcp::Args a = lcp_args(mu, ld_mu, act, ld_act, std, h1, z2, w1, w2, w3, rows, d, k, slope);
  a.g = g, a.v1 = v1, a.v2 = v2, a.part = scratch;
  hipError_t e;
  if (hidden == 256) e = d <= 16 ? lcp::launch_fwd_t<256, 1>(a, s) : lcp::launch_fwd_t<256, 2>(a, s);
  else e = d <= 16 ? lcp::launch_fwd_t<128, 1>(a, s) : lcp::launch_fwd_t<128, 2>(a, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lcp::lcp_penalty, dim3(1), dim3(64), 0, s, (const float*)scratch, lcp::grid_x(rows), (int)rows,
                     penalty);
  return hipGetLastError();
}

hipError_t launch_lcp_backward(const float* mu, long long ld_mu, const float* act, long long ld_act, const float* std,
                               const float* h1, const float* z2, const float* w1, const float* w2, const float* w3,
                               long long rows, int hidden, int d, int k, float slope, const float* g, const float* v1,
                               const float* v2, const float* g_pen, float* s1, float* scratch, float* dmu, float* dstd,
                               float* grads, hipStream_t s) {
  lcp::Args a = lcp_args(mu, ld_mu, act, ld_act, std, h1, z2, w1, w2, w3, rows, d, k, slope);
  a.g = const_cast<float*>(g), a.v1 = const_cast<float*>(v1), a.v2 = const_cast<float*>(v2);
  a.s1 = s1, a.g_pen = g_pen, a.dmu = dmu, a.part = scratch;
  const int row = lcp::bwd_row(hidden, d, k);
  const int blocks = lcp::grid_x(rows);
  hipError_t e;
  if (hidden == 256) e = d <= 16 ? lcp::launch_bwd_t<256, 1>(a, row, s) : lcp::launch_bwd_t<256, 2>(a, row, s);
  else e = d <= 16 ? lcp::launch_bwd_t<128, 1>(a, row, s) : lcp::launch_bwd_t<128, 2>(a, row, s);
  if (e != hipSuccess) return e;
  // gW2 = v2^T s1: mlp_wgrad with (gz2, h1) := (v2, s1)
  gr_mlp_args m = {};
  m.rows = rows, m.nets = 1, m.hidden = hidden, m.slope = slope;
  m.net[0].gz2 = const_cast<float*>(v2);
  m.net[0].h1 = s1;
  m.net[0].d = d, m.net[0].k = k;
  float* wpart = scratch + (size_t)blocks * lcp::bwd_row(hidden, 32, 4);
  e = launch_mlp_wgrad(m, wpart, s);
  if (e != hipSuccess) return e;
  const int q_total = (hidden * d + k * hidden + k + 3) / 4 + hidden * hidden / 4;
  hipLaunchKernelGGL(lcp::lcp_final, dim3((q_total + 63) / 64), dim3(lcp::LF_WAVES * 64), 0, s,
                     (const float*)scratch, blocks, row, (const float*)wpart, mlp_wgrad_splits(rows, hidden, 1), hidden,
                     d, k, grads, dstd);
  return hipGetLastError();
}

}  // namespace gr
