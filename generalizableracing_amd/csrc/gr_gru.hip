// gr_gru.hip — the GRU memory of ActorCriticRecurrent (one layer, torch.nn.GRU's parameters and gate order r, z, n)
// as fp32-MFMA kernels: one rollout step (gr_gru_step), the masked sequence over a mini-batch in one launch
// (gr_gru_seq_forward) and its BPTT (gr_gru_seq_backward), include/gr.h.
//
//   a_r = W_ir x + b_ir + W_hr h' + b_hr        r = sigmoid(a_r)
//   a_z = W_iz x + b_iz + W_hz h' + b_hz        z = sigmoid(a_z)
//   hn  = W_hn h' + b_hn                        n = tanh(W_in x + b_in + r hn)
//   h_t = (1 - z) n + z h'                      h' = h_{t-1} (1 - done[t-1])  (t = 0: h0 as given)
//
// gru_fwd : a workgroup owns GE = 16 envs and walks them through the T steps.  Wave w owns hidden units 16 w .. + 15
//           (R / 16 waves) and all three of their gates, so the gate arithmetic is lane-local: A = the W rows of the
//           units (streamed from L2 every step: 3R x R fp32 does not fit the LDS), B = x_t^T and h'^T (the tile's h
//           lives in LDS across the steps, double buffered: one barrier per step), C rows = units, column = env.
//           The rollout step is this kernel with T = 1 and out = h, so the two share their per-step arithmetic.
// gru_bwd : the serial part of BPTT, the same tiling run backwards; it carries dh in registers, writes the gate
//           gradients [da_r | da_z | da_n | da_hn] per (t, env) and streams W_hh's columns for dh' = z dh + W_hh^T da.
// gru_wgrad / gru_final : gW_ih = sum da_i^T x, gW_hh = sum da_h^T h', the biases their column sums, over row splits
//           into partial rows, summed in a fixed order (partial_rows_sum).  No atomics: bit-reproducible.
// The wide family (gr_gru_wide_*: d <= 256, and the input gradient) runs the same gru_fwd and gru_bwd (their input loop
// and their arithmetic do not depend on d's range) and adds
// gru_gi      : the sequence's input projection hoisted out of the serial loop, gi [T B][3R] = x W_ih^T, as the very
//           MFMA chain gru_fwd's input loop runs (same operands, same k order, from zero), written into the gates
//           buffer's own r, z, n slots; gru_fwd<R, true> then starts its accumulators from them.  The same bits as the
//           in-loop form (which the rollout step keeps: it has no serial loop to hoist from), one device-wide GEMM
//           instead of 3R x d more weights streamed per step per workgroup.
// gru_wgrad_x : gW_ih's columns past gru_wgrad's four tiles, the same row splits and partial rows;
// gru_gx      : gx [T B][d] = da_i [T B][3R] W_ih [3R][d], one fixed-order MFMA chain over the 3R gate units per
//           output, so a row's gx does not depend on the rows around it.
// The MFMA fragment convention and helpers: gr_mfma.h.
#include <hip/hip_runtime.h>

#include "../../include/gr.h"
#include "gr_kernels.h"
#include "gr_mfma.h"

namespace gr {
namespace gru {

constexpr int GE = 16;        // envs per workgroup tile (one MFMA column tile)
constexpr int WG_WAVES = 4;   // gru_wgrad: waves per workgroup, one 16-row tile of the 3R gate units each
constexpr int GF_WAVES = 4;   // gru_final

// fast activations on v_exp_f32 / v_rcp_f32 (no libm call chain in the serial loop)
__device__ __forceinline__ float sigmoid_fast(float a) { return __builtin_amdgcn_rcpf(1.0f + __expf(-a)); }
__device__ __forceinline__ float tanh_fast(float a) {
  const float e = __expf(-2.0f * fabsf(a));
  return copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), a);
}

struct FwdArgs {
  const float* x;  // element (t, b, k) at x[t ldx_t + b ldx_b + k]
  long long ldx_t, ldx_b;
  const float* h0;             // [B][R]
  const unsigned char* dones;  // (t, b) at dones[t ld_dones + b]; null: no mask
  long long ld_dones;
  const float *w_ih, *w_hh, *b_ih, *b_hh;
  float* out;         // [T][B][R] (T == 1: may be h0 itself)
  float* gates;       // [T][B][4R]: r, z, n, hn; null: not saved
  float* h_prev_out;  // [B][R]: a copy of h0; null: none
  int T, B, D;
};

// GI: the input part of a_r, a_z, a_n was computed by gru_gi and lies in the step's gates row (its r, z, n slots)
template <int R, bool GI = false>
__global__ __launch_bounds__(R * 4) void gru_fwd(FwdArgs a) {
  constexpr int Q = R / 16, HP = R + 4, NTH = R * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int B = a.B, D = a.D, T = a.T;
  const int DQ = (D + 15) >> 4;
  extern __shared__ float lds[];  // [2][GE][HP]: the tile's masked h, double buffered
  const int base = blockIdx.x * GE;
  const int u0 = 16 * wave;  // the wave's units
  for (int i = threadIdx.x; i < GE * (R / 4); i += NTH) {
    const int row = i / (R / 4), c4 = 4 * (i % (R / 4));
    const int b = base + row;
    const m4 v = ld4(a.h0 + (size_t)(b < B ? b : B - 1) * R + c4);
    st4(lds + row * HP + c4, v);
    if (a.h_prev_out && b < B) st4(a.h_prev_out + (size_t)b * R + c4, v);
  }
  const int b = base + j;  // the lane's env: column j of the B operands and of the C tiles
  const int bb = b < B ? b : B - 1;
  const int uc = u0 + 4 * g;  // the lane's units uc .. uc + 3 in the C tiles
  const m4 bir = ld4(a.b_ih + uc), biz = ld4(a.b_ih + R + uc), bin = ld4(a.b_ih + 2 * R + uc);
  const m4 bhr = ld4(a.b_hh + uc), bhz = ld4(a.b_hh + R + uc), bhn = ld4(a.b_hh + 2 * R + uc);
  const float* wih = a.w_ih;
  const float* whh = a.w_hh;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    // (the weights are streamed every step: without this the loads are hoisted out of the loop into registers
    // the kernel does not have)
    asm volatile("" : "+s"(wih), "+s"(whh));
    const float* hb = lds + (t & 1) * GE * HP;
    float* hw = lds + ((t + 1) & 1) * GE * HP;
    m4 ar = zero4(), az = zero4(), ani = zero4(), anh = zero4();
    // ---- input part: k = input 16 q + 4 g + r (inputs past D: 0)
    if constexpr (GI) {
      // (the lane's own slots of the row: read here, overwritten with the gates below)
      const float* gp = a.gates + ((size_t)t * B + bb) * (4 * R) + uc;
      ar = ld4(gp), az = ld4(gp + R), ani = ld4(gp + 2 * R);
    } else {
      const float* xr = a.x + (size_t)t * a.ldx_t + (size_t)bb * a.ldx_b;
      for (int q = 0; q < DQ; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * q + 4 * g + r;
          const bool ok = k < D;
          const int kk = ok ? k : 0;
          const float xv = ok ? xr[kk] : 0.0f;
          const float wr = wih[(size_t)(u0 + j) * D + kk];
          const float wz = wih[(size_t)(R + u0 + j) * D + kk];
          const float wn = wih[(size_t)(2 * R + u0 + j) * D + kk];
          ar = mf(ok ? wr : 0.0f, xv, ar);
          az = mf(ok ? wz : 0.0f, xv, az);
          ani = mf(ok ? wn : 0.0f, xv, ani);
        }
      }
    }
    // ---- hidden part: k step 4 q + r = unit 16 q + 4 g + r of h'
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const m4 hv = ld4(hb + j * HP + 16 * q + 4 * g);
      const m4 wr = ld4(whh + (size_t)(u0 + j) * R + 16 * q + 4 * g);
      const m4 wz = ld4(whh + (size_t)(R + u0 + j) * R + 16 * q + 4 * g);
      const m4 wn = ld4(whh + (size_t)(2 * R + u0 + j) * R + 16 * q + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ar = mf(wr[r], hv[r], ar);
        az = mf(wz[r], hv[r], az);
        anh = mf(wn[r], hv[r], anh);
      }
    }
    // ---- the gates of units uc + q of env j
    const m4 hp = ld4(hb + j * HP + uc);
    m4 rv, zv, nv, hn, hnew;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rv[q] = sigmoid_fast(ar[q] + bir[q] + bhr[q]);
      zv[q] = sigmoid_fast(az[q] + biz[q] + bhz[q]);
      hn[q] = anh[q] + bhn[q];
      nv[q] = tanh_fast(ani[q] + bin[q] + rv[q] * hn[q]);
      hnew[q] = (1.0f - zv[q]) * nv[q] + zv[q] * hp[q];
    }
    // the next step's h' (a finished env restarts from 0)
    float keep = 1.0f;
    if (a.dones && t + 1 < T) keep = a.dones[(size_t)t * a.ld_dones + bb] ? 0.0f : 1.0f;
    st4(hw + j * HP + uc, hnew * keep);
    if (b < B) {
      const size_t row = (size_t)t * B + b;
      st4(a.out + row * R + uc, hnew);
      if (a.gates) {
        float* gr_ = a.gates + row * (4 * R) + uc;
        st4(gr_, rv);
        st4(gr_ + R, zv);
        st4(gr_ + 2 * R, nv);
        st4(gr_ + 3 * R, hn);
      }
    }
    __syncthreads();  // the step's h' complete; every wave is done reading the other buffer
  }
}

constexpr int GI_CT = 4;     // gru_gi: 16-row column tiles per workgroup
constexpr int GI_WAVES = 4;  // one 16-row tile of W_ih's 3R rows per wave

// gi = x W_ih^T into the gates buffer: element (row, m < 3R) at gates[row 4R + m].  blockIdx.x: GI_CT tiles of 16 rows
// (t, b), blockIdx.y: 64 of the 3R gate units.  A = W_ih row m0 + j, B = x^T (column j = the row), k = input
// 16 q + 4 g + r, inputs past D: 0 -- gru_fwd's input loop operand for operand, so each output is the same chain.
template <int R>
__global__ __launch_bounds__(GI_WAVES * 64) void gru_gi(FwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int B = a.B, D = a.D;
  const int DQ = (D + 15) >> 4;
  const int rows = a.T * B;
  const int m0 = 16 * (blockIdx.y * GI_WAVES + wave);  // < 3R
  const int row0 = blockIdx.x * (16 * GI_CT);
  const float* xr[GI_CT];
#pragma unroll
  for (int c = 0; c < GI_CT; ++c) {
    const int row = row0 + 16 * c + j;
    const int rr = row < rows ? row : rows - 1;
    const int t = rr / B, bq = rr - t * B;
    xr[c] = a.x + (size_t)t * a.ldx_t + (size_t)bq * a.ldx_b;
  }
  const float* wr = a.w_ih + (size_t)(m0 + j) * D;
  m4 acc[GI_CT];
#pragma unroll
  for (int c = 0; c < GI_CT; ++c) acc[c] = zero4();
  for (int q = 0; q < DQ; ++q) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * q + 4 * g + r;
      const bool ok = k < D;
      const int kk = ok ? k : 0;
      const float w = wr[kk];
      const float wv = ok ? w : 0.0f;
#pragma unroll
      for (int c = 0; c < GI_CT; ++c) {
        const float xv = xr[c][kk];
        acc[c] = mf(wv, ok ? xv : 0.0f, acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < GI_CT; ++c) {
    const int row = row0 + 16 * c + j;
    if (row < rows) st4(a.gates + (size_t)row * (4 * R) + m0 + 4 * g, acc[c]);
  }
}

struct BwdArgs {
  const float* gout;   // [T][B][R]
  const float* h0;     // [B][R]
  const float* out;    // [T][B][R]
  const float* gates;  // [T][B][4R]
  const unsigned char* dones;
  long long ld_dones;
  const float* w_hh;
  float* ga;  // [T][B][4R]: da_r, da_z, da_n, da_hn
  int T, B;
};

template <int R>
__global__ __launch_bounds__(R * 4) void gru_bwd(BwdArgs a) {
  constexpr int Q = R / 16, GP = 3 * R + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int B = a.B, T = a.T;
  extern __shared__ float lds[];  // [2][GE][GP]: the step's da_r, da_z, da_hn, double buffered
  const int base = blockIdx.x * GE;
  const int u0 = 16 * wave;
  const int b = base + j;
  const int bb = b < B ? b : B - 1;
  const int uc = u0 + 4 * g;
  const float* whh = a.w_hh;
  m4 dh = zero4();  // the carried gradient of h_t, units uc + q of env j
  for (int t = T - 1; t >= 0; --t) {
    asm volatile("" : "+s"(whh));  // (as gru_fwd: streamed every step)
    float* db = lds + (t & 1) * GE * GP;
    const size_t row = (size_t)t * B + bb;
    dh += ld4(a.gout + row * R + uc);
    const float* gr_ = a.gates + row * (4 * R) + uc;
    const m4 rv = ld4(gr_), zv = ld4(gr_ + R), nv = ld4(gr_ + 2 * R), hn = ld4(gr_ + 3 * R);
    float keep = 1.0f;  // of done[t - 1]: h' = keep out[t - 1]
    m4 hp;
    if (t == 0) {
      hp = ld4(a.h0 + (size_t)bb * R + uc);
    } else {
      if (a.dones) keep = a.dones[(size_t)(t - 1) * a.ld_dones + bb] ? 0.0f : 1.0f;
      hp = ld4(a.out + (row - B) * R + uc) * keep;
    }
    m4 dar, daz, dan, dahn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float dn = dh[q] * (1.0f - zv[q]);
      const float dz = dh[q] * (hp[q] - nv[q]);
      dan[q] = dn * (1.0f - nv[q] * nv[q]);
      daz[q] = dz * zv[q] * (1.0f - zv[q]);
      dar[q] = dan[q] * hn[q] * rv[q] * (1.0f - rv[q]);
      dahn[q] = dan[q] * rv[q];
    }
    st4(db + j * GP + uc, dar);
    st4(db + j * GP + R + uc, daz);
    st4(db + j * GP + 2 * R + uc, dahn);
    if (b < B) {
      float* o = a.ga + ((size_t)t * B + b) * (4 * R) + uc;
      st4(o, dar);
      st4(o + R, daz);
      st4(o + 2 * R, dan);
      st4(o + 3 * R, dahn);
    }
    __syncthreads();  // the step's da complete; every wave is done reading the other buffer
    if (t == 0) break;  // (no gradient for h0)
    // ---- dh' = z dh + W_hh^T da: A row j = unit u0 + j of h', k = gate unit 16 q + 4 g + r (a column of W_hh)
    // (the three gates are contiguous in the LDS row: gate unit v = 16 kq + 4 g + r over kq < 3 R / 16; two
    // accumulators take the even and the odd kq; unrolled by 4 kq only: the whole chain's loads in flight spilled)
    m4 acc0 = zero4(), acc1 = zero4();
#pragma unroll 2
    for (int kq = 0; kq < 3 * Q; kq += 2) {
      const int v = 16 * kq + 4 * g;
      const m4 d0 = ld4(db + j * GP + v), d1 = ld4(db + j * GP + v + 16);
      float w0[4], w1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        w0[r] = whh[(size_t)(v + r) * R + u0 + j];
        w1[r] = whh[(size_t)(v + 16 + r) * R + u0 + j];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc0 = mf(w0[r], d0[r], acc0);
        acc1 = mf(w1[r], d1[r], acc1);
      }
    }
    dh = (dh * zv + (acc0 + acc1)) * keep;
  }
}

// floats of a partial row = of the flat gradient: [gW_ih (3R D) | gW_hh (3R R) | gb_ih (3R) | gb_hh (3R)]
__host__ __device__ constexpr long long grad_floats(int r, int d) { return 3LL * r * (d + r + 2); }

struct WgArgs {
  const float* ga;  // [T B][4R]
  const float* x;
  long long ldx_t, ldx_b;
  const float* h0;
  const float* out;
  const unsigned char* dones;
  long long ld_dones;
  float* part;  // [splits][grad_floats]
  int T, B, D, rows_per_split;  // rows_per_split: a multiple of 4
};

// blockIdx.x: 4 tiles of 16 gate units (one per wave), blockIdx.y: the split's rows.  The contraction runs over the
// rows (t, b): k = g is row s + g.  A = the gate gradients of the tile's units (the n gate's hidden part: da_hn),
// B = h' (R / 16 column tiles) and x (up to 4 column tiles).
template <int R>
__global__ __launch_bounds__(WG_WAVES * 64) void gru_wgrad(WgArgs a) {
  constexpr int NT = R / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int B = a.B, D = a.D;
  const int DQ = (D + 15) >> 4;
  const int m0 = 16 * (blockIdx.x * WG_WAVES + wave);  // < 3R
  const bool n_gate = m0 >= 2 * R;
  const int rows = a.T * B;
  const int lo = blockIdx.y * a.rows_per_split;
  const int hi = lo + a.rows_per_split < rows ? lo + a.rows_per_split : rows;
  m4 ah[NT], ai[4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) ah[nt] = zero4();
#pragma unroll
  for (int q = 0; q < 4; ++q) ai[q] = zero4();
  float sbi = 0.0f, sbh = 0.0f;
  for (int s = lo; s < hi; s += 4) {
    const int row = s + g;
    const bool ok = row < hi;
    const int rr = ok ? row : lo;
    const int t = rr / B, bq = rr - t * B;
    const float* gr_ = a.ga + (size_t)rr * (4 * R);
    const float gi = gr_[m0 + j];
    const float gh = gr_[(n_gate ? m0 + R : m0) + j];
    const float avi = ok ? gi : 0.0f, avh = ok ? gh : 0.0f;
    sbi += avi;
    sbh += avh;
    // h' of the row: h0 (t = 0) or the masked out[t - 1]
    const float* hp = t == 0 ? a.h0 + (size_t)bq * R : a.out + ((size_t)(t - 1) * B + bq) * R;
    float keep = 1.0f;
    if (t > 0 && a.dones) keep = a.dones[(size_t)(t - 1) * a.ld_dones + bq] ? 0.0f : 1.0f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) ah[nt] = mf(avh, hp[16 * nt + j] * keep, ah[nt]);
    const float* xr = a.x + (size_t)t * a.ldx_t + (size_t)bq * a.ldx_b;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < DQ) {
        const int k = 16 * q + j;
        const float xv = k < D ? xr[k < D ? k : 0] : 0.0f;
        ai[q] = mf(avi, xv, ai[q]);
      }
  }
  // ---- the split's partial row: C rows = units m0 + 4 g + q, column j of tile nt
  float* pr = a.part + (size_t)blockIdx.y * (size_t)grad_floats(R, D);
  float* pih = pr;
  float* phh = pr + (size_t)3 * R * D;
  float* pbi = phh + (size_t)3 * R * R;
  float* pbh = pbi + 3 * R;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + 4 * g + q;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) phh[(size_t)m * R + 16 * nt + j] = ah[nt][q];
#pragma unroll
    for (int dq = 0; dq < 4; ++dq)
      if (16 * dq + j < D) pih[(size_t)m * D + 16 * dq + j] = ai[dq][q];
  }
  // the biases: the lane's sum over its rows, then over the 4 row groups g (fixed butterfly order)
  sbi += __shfl_xor(sbi, 16);
  sbi += __shfl_xor(sbi, 32);
  sbh += __shfl_xor(sbh, 16);
  sbh += __shfl_xor(sbh, 32);
  if (g == 0) {
    pbi[m0 + j] = sbi;
    pbh[m0 + j] = sbh;
  }
}

// gW_ih's columns 64 (blockIdx.z + 1) .. + 63 (the wide family, d > 64): gru_wgrad's input part on the next four
// column tiles, into the same partial rows (gru_wgrad wrote the first four, gW_hh and the biases)
template <int R>
__global__ __launch_bounds__(WG_WAVES * 64) void gru_wgrad_x(WgArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int B = a.B, D = a.D;
  const int k0 = 64 * (blockIdx.z + 1);                // < D
  const int m0 = 16 * (blockIdx.x * WG_WAVES + wave);  // < 3R
  const int rows = a.T * B;
  const int lo = blockIdx.y * a.rows_per_split;
  const int hi = lo + a.rows_per_split < rows ? lo + a.rows_per_split : rows;
  m4 ai[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) ai[q] = zero4();
  for (int s = lo; s < hi; s += 4) {
    const int row = s + g;
    const bool ok = row < hi;
    const int rr = ok ? row : lo;
    const int t = rr / B, bq = rr - t * B;
    const float gi = a.ga[(size_t)rr * (4 * R) + m0 + j];
    const float avi = ok ? gi : 0.0f;
    const float* xr = a.x + (size_t)t * a.ldx_t + (size_t)bq * a.ldx_b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + 16 * q + j;
      const float xv = k < D ? xr[k < D ? k : 0] : 0.0f;
      ai[q] = mf(avi, xv, ai[q]);
    }
  }
  float* pih = a.part + (size_t)blockIdx.y * (size_t)grad_floats(R, D);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + 4 * g + q;
#pragma unroll
    for (int dq = 0; dq < 4; ++dq)
      if (k0 + 16 * dq + j < D) pih[(size_t)m * D + k0 + 16 * dq + j] = ai[dq][q];
  }
}

struct GxArgs {
  const float* ga;    // [rows][4R]: da_r, da_z, da_n first
  const float* w_ih;  // [3R][D]
  float* gx;          // row (t, b), input k at gx[t ld_t + b ld_b + k]
  long long ld_t, ld_b;
  int rows, B, D;
};

constexpr int GX_RT = 4;     // 16-row tiles per workgroup
constexpr int GX_WAVES = 4;  // wave w owns the column tiles w, w + 4, w + 8, w + 12 of all GX_RT row tiles

// gx = da_i W_ih: A = da_i (row j of a row tile, k order: a float4 of 4 consecutive gate units feeds 4 k steps),
// B = W_ih[gate unit][input 16 ct + j], C rows = rows 4 g + r of the tile, column = the input.  Every output is one
// chain over the gate units 0 .. 3R - 1 in this order whatever the launch holds.
template <int R>
__global__ __launch_bounds__(GX_WAVES * 64) void gru_gx(GxArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int D = a.D, rows = a.rows;
  const int DQ = (D + 15) >> 4;
  const int row0 = blockIdx.x * (16 * GX_RT);
  const float* ap[GX_RT];
#pragma unroll
  for (int rt = 0; rt < GX_RT; ++rt) {
    const int r = row0 + 16 * rt + j;
    ap[rt] = a.ga + (size_t)(r < rows ? r : rows - 1) * (4 * R) + 4 * g;
  }
  int col[4];
  bool cok[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 16 * (wave + GX_WAVES * c) + j;
    cok[c] = k < D;
    col[c] = cok[c] ? k : 0;
  }
  m4 acc[GX_RT][4];
#pragma unroll
  for (int rt = 0; rt < GX_RT; ++rt)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[rt][c] = zero4();
  const float* wih = a.w_ih;
#pragma unroll 2
  for (int q = 0; q < 3 * R / 16; ++q) {
    m4 av[GX_RT];
#pragma unroll
    for (int rt = 0; rt < GX_RT; ++rt) av[rt] = ld4(ap[rt] + 16 * q);
    const float* wq = wih + (size_t)(16 * q + 4 * g) * D;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (wave + GX_WAVES * c >= DQ) continue;  // (wave-uniform)
      float w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = wq[(size_t)r * D + col[c]];
        w[r] = cok[c] ? v : 0.0f;
      }
#pragma unroll
      for (int rt = 0; rt < GX_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][c] = mf(av[rt][r], w[r], acc[rt][c]);
    }
  }
#pragma unroll
  for (int rt = 0; rt < GX_RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 16 * rt + 4 * g + r;
      if (row >= rows) continue;
      const int t = row / a.B, b = row - t * a.B;
      float* o = a.gx + (size_t)t * a.ld_t + (size_t)b * a.ld_b;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (cok[c]) o[col[c]] = acc[rt][c][r];
    }
}

// grads[e] = the fixed-order sum of the splits' partial rows: a lane owns 4 consecutive elements, the 4 waves take
// every 4th partial row and are summed in wave order (as lcp_final)
__global__ __launch_bounds__(GF_WAVES * 64) void gru_final(const float* __restrict__ part, int splits, long long ld,
                                                          float* __restrict__ grads) {
  __shared__ m4 sm[GF_WAVES * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * 64 + lane;
  const bool in = 4 * q < ld;
  sm[threadIdx.x] = partial_rows_sum<GF_WAVES>(in ? part + 4 * q : nullptr, splits, (int)ld, wv);
  __syncthreads();
  if (wv == 0 && in) {
    m4 t = sm[lane];
#pragma unroll
    for (int w = 1; w < GF_WAVES; ++w) t += sm[w * 64 + lane];
    st4(grads + 4 * q, t);
  }
}

static int tiles(long long b) { return (int)((b + GE - 1) / GE); }

// the row splits of gru_wgrad: about 512 workgroups, at least 64 rows each
static void wgrad_split(long long rows, int r, int* rows_per_split, int* splits) {
  const int xblocks = 3 * r / (16 * WG_WAVES);
  long long target = 512 / xblocks;
  const long long cap = (rows + 63) / 64;
  if (target > cap) target = cap;
  if (target < 1) target = 1;
  long long rps = (rows + target - 1) / target;
  rps = (rps + 3) & ~3LL;
  *rows_per_split = (int)rps;
  *splits = (int)((rows + rps - 1) / rps);
}

template <int R>
static hipError_t launch_fwd_t(const FwdArgs& a, bool hoist, hipStream_t s) {
  if (!hoist) return launch_lds<gru_fwd<R>>(dim3(tiles(a.B)), dim3(R * 4), (size_t)4 * 2 * GE * (R + 4), s, a);
  const int rows = a.T * a.B;
  hipLaunchKernelGGL(gru_gi<R>, dim3((rows + 16 * GI_CT - 1) / (16 * GI_CT), 3 * R / (16 * GI_WAVES)),
                     dim3(GI_WAVES * 64), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_lds<gru_fwd<R, true>>(dim3(tiles(a.B)), dim3(R * 4), (size_t)4 * 2 * GE * (R + 4), s, a);
}

template <int R>
static hipError_t launch_bwd_t(const BwdArgs& a, const WgArgs& w, int splits, float* grads, const GxArgs* gx,
                               hipStream_t s) {
  hipError_t e = launch_lds<gru_bwd<R>>(dim3(tiles(a.B)), dim3(R * 4), (size_t)4 * 2 * GE * (3 * R + 4), s, a);
  if (e != hipSuccess) return e;
  if (gx) {  // (the wide family only)
    hipLaunchKernelGGL(gru_gx<R>, dim3((gx->rows + 16 * GX_RT - 1) / (16 * GX_RT)), dim3(GX_WAVES * 64), 0, s, *gx);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gru_wgrad<R>, dim3(3 * R / (16 * WG_WAVES), splits), dim3(WG_WAVES * 64), 0, s, w);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (w.D > 64) {  // (the wide family only)
    hipLaunchKernelGGL(gru_wgrad_x<R>, dim3(3 * R / (16 * WG_WAVES), splits, (w.D - 1) / 64),
                       dim3(WG_WAVES * 64), 0, s, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const long long ld = grad_floats(R, w.D);
  hipLaunchKernelGGL(gru_final, dim3((unsigned)((ld / 4 + 63) / 64)), dim3(GF_WAVES * 64), 0, s,
                     (const float*)w.part, splits, ld, grads);
  return hipGetLastError();
}

}  // namespace gru

// scratch (floats) of gr_gru_seq_backward: the gate gradients [T B][4R], then gru_wgrad's partial rows (d <= 64)
int64_t gru_scratch_floats(long long t, long long b, int r) {
  int rps, splits;
  gru::wgrad_split(t * b, r, &rps, &splits);
  return t * b * 4 * r + (int64_t)splits * gru::grad_floats(r, 64);
}

// the same of gr_gru_wide_seq_backward (d <= 256)
int64_t gru_wide_scratch_floats(long long t, long long b, int d, int r) {
  int rps, splits;
  gru::wgrad_split(t * b, r, &rps, &splits);
  return t * b * 4 * r + (int64_t)splits * gru::grad_floats(r, d);
}

hipError_t launch_gru_forward(const float* x, long long ldx_t, long long ldx_b, const float* h0,
                              const unsigned char* dones, long long ld_dones, const float* w_ih, const float* w_hh,
                              const float* b_ih, const float* b_hh, int t, long long b, int d, int r, float* out,
                              float* gates, float* h_prev_out, bool hoist, hipStream_t s) {
  gru::FwdArgs a = {};
  a.x = x, a.ldx_t = ldx_t, a.ldx_b = ldx_b, a.h0 = h0, a.dones = dones, a.ld_dones = ld_dones;
  a.w_ih = w_ih, a.w_hh = w_hh, a.b_ih = b_ih, a.b_hh = b_hh;
  a.out = out, a.gates = gates, a.h_prev_out = h_prev_out;
  a.T = t, a.B = (int)b, a.D = d;
  hoist = hoist && gates && t > 1;  // (gi lives in the gates buffer; one step has no serial loop to hoist from)
  switch (r) {
    case 64: return gru::launch_fwd_t<64>(a, hoist, s);
    case 128: return gru::launch_fwd_t<128>(a, hoist, s);
    case 192: return gru::launch_fwd_t<192>(a, hoist, s);
    default: return gru::launch_fwd_t<256>(a, hoist, s);
  }
}

hipError_t launch_gru_backward(const float* gout, const float* x, long long ldx_t, long long ldx_b, const float* h0,
                               const unsigned char* dones, long long ld_dones, const float* w_hh, const float* out,
                               const float* gates, int t, long long b, int d, int r, float* scratch, float* grads,
                               const float* w_ih, float* gx, long long ldgx_t, long long ldgx_b, hipStream_t s) {
  gru::BwdArgs a = {};
  a.gout = gout, a.h0 = h0, a.out = out, a.gates = gates, a.dones = dones, a.ld_dones = ld_dones, a.w_hh = w_hh;
  a.ga = scratch, a.T = t, a.B = (int)b;
  gru::WgArgs w = {};
  int splits;
  gru::wgrad_split(t * b, r, &w.rows_per_split, &splits);
  w.ga = scratch, w.x = x, w.ldx_t = ldx_t, w.ldx_b = ldx_b, w.h0 = h0, w.out = out, w.dones = dones;
  w.ld_dones = ld_dones, w.part = scratch + (size_t)t * b * 4 * r, w.T = t, w.B = (int)b, w.D = d;
  gru::GxArgs x_ = {};
  x_.ga = scratch, x_.w_ih = w_ih, x_.gx = gx, x_.ld_t = ldgx_t, x_.ld_b = ldgx_b;
  x_.rows = (int)(t * b), x_.B = (int)b, x_.D = d;
  const gru::GxArgs* gp = gx ? &x_ : nullptr;
  switch (r) {
    case 64: return gru::launch_bwd_t<64>(a, w, splits, grads, gp, s);
    case 128: return gru::launch_bwd_t<128>(a, w, splits, grads, gp, s);
    case 192: return gru::launch_bwd_t<192>(a, w, splits, grads, gp, s);
    default: return gru::launch_bwd_t<256>(a, w, splits, grads, gp, s);
  }
}

}  // namespace gr
