// gr_mfma.h — what the whole-network fp32-MFMA kernels of the update's MLPs (gr_mlp.hip) and of PPOLCP's penalty
// chain over the same network (gr_lcp.hip) share: the fragment helpers, the tile geometry, the launcher, the W2-column
// operand load, the partial-row stores of the backward passes and the fixed-order sum over partial rows.  Every sum
// here has a fixed order (the update is bit-reproducible): both files take it from this one statement.  Included by
// those two sources only (it defines device functions).
//
// MFMA fragment convention (v_mfma_f32_16x16x4_f32): lane l = 16 g + j holds A[row j][k = g] and B[k = g][col j];
// the C tile holds rows 4 g + r of column j in register r.  "k order": k step 4 q + r of a contraction over H
// units is unit 16 q + 4 g + r, so a float4 of 4 consecutive units feeds 4 k steps.
#pragma once
#include <hip/hip_runtime.h>

namespace gr {

typedef float m4 __attribute__((ext_vector_type(4)));

constexpr int MW = 8;        // waves per workgroup (2 per SIMD)
// (32-row tiles where the W2 columns take 128 registers: with 64-row tiles the accumulators spilled)
constexpr int BC = 2;        // 16-row column tiles per workgroup tile of the passes that hold W2 columns
constexpr int BE = 16 * BC;  // rows per such tile

__device__ __forceinline__ m4 mf(float a, float b, m4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ m4 ld4(const float* p) { return *reinterpret_cast<const m4*>(p); }
__device__ __forceinline__ void st4(float* p, m4 v) { *reinterpret_cast<m4*>(p) = v; }
__device__ __forceinline__ float lrelu(float z, float s) { return z > 0.0f ? z : z * s; }
__device__ __forceinline__ float lrelu_d(float z, float s) { return z > 0.0f ? 1.0f : s; }
__device__ __forceinline__ m4 zero4() { return (m4){0.0f, 0.0f, 0.0f, 0.0f}; }

// Launches Kernel with `lds` bytes of dynamic LDS; the first launch of each kernel raises its limit (the once-only
// flag is per Kernel: one instantiation each).
template <auto Kernel, typename... Args>
static hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    attr = true;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return hipGetLastError();
}

// A operands of the passes that run the hidden layer backwards (mlp_bwd, lcp_fwd), for the lane's hidden unit i of
// h1 (row j of a 16-unit tile): gh1^T = W2^T gz2^T -> k step 4 q + r is z2 unit 16 q + 4 g + r: W2[16 q + 4 g + r][i];
// gh2^T = W3^T gy^T -> k = output g
template <int H>
__device__ __forceinline__ void load_w2_column(const float* __restrict__ W2, const float* __restrict__ W3, int K, int i,
                                               int g, float (&w2c)[H / 4], float& w3a) {
#pragma unroll
  for (int q = 0; q < H / 16; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) w2c[4 * q + r] = W2[(size_t)(16 * q + 4 * g + r) * H + i];
  w3a = g < K ? W3[(size_t)g * H + i] : 0.0f;
}

// The small weight gradients of the 16-unit tile at u0 into the workgroup's partial row pr: gW1 [H][D] at 0 (C rows =
// units u0 + 4 g + q, col = input 16 dt + j) and gW3 [k][H] at o_w3 (C rows = outputs 4 g + q: g == 0, q < k;
// col = unit u0 + j)
template <int H, int DT>
__device__ __forceinline__ void store_gw1_gw3(float* pr, int o_w3, int u0, int D, int K, int g, int j,
                                              const m4 (&gw1)[DT], m4 gw3) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (16 * dt + j < D) pr[(size_t)(u0 + 4 * g + q) * D + 16 * dt + j] = gw1[dt][q];
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < K) pr[o_w3 + q * H + u0 + j] = gw3[q];
  }
}

// The bias gradients into the MLP backward's partial row [gW1 (H D) | gb1 (H) | gb2 (H) | gW3 (k H) | gb3 (k)]: each
// lane's sums over its rows are summed over the 16 lanes j of its g group (fixed butterfly order); gb1 / gb2 of the
// wave's units 16 (wave TW + t) + 4 g + q, gb3 (wave 0's lanes, output g)
template <int H, int TW>
__device__ __forceinline__ void store_bias_sums(float* pr, int D, int K, int wave, int g, int j, float (&gb1)[TW][4],
                                                float (&gb2)[TW][4], float gb3) {
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v1 = gb1[t][q], v2 = gb2[t][q];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        v1 += __shfl_xor(v1, off);
        v2 += __shfl_xor(v2, off);
      }
      gb1[t][q] = v1;
      gb2[t][q] = v2;
    }
  if (j == 0) {
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pr[H * D + 16 * (wave * TW + t) + 4 * g + q] = gb1[t][q];
        pr[H * D + H + 16 * (wave * TW + t) + 4 * g + q] = gb2[t][q];
      }
  }
  if (wave == 0) {
    float v = gb3;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
    if (j == 0 && g < K) pr[H * D + 2 * H + K * H + g] = v;
  }
}

// The lane's float4 summed over `rows` partial rows (stride ldr floats) in a fixed order: wave wv of WAVES takes
// rows wv, wv + WAVES, ..., 8 loads in flight per lane into two accumulators, then the tail; the caller sums the
// waves' results in wave order.  src null: 0.
template <int WAVES>
__device__ __forceinline__ m4 partial_rows_sum(const float* src, int rows, int ldr, int wv) {
  m4 acc0 = zero4(), acc1 = zero4();
  if (src) {
    int b = wv;
    for (; b + 7 * WAVES < rows; b += 8 * WAVES) {
      m4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld4(src + (size_t)(b + u * WAVES) * ldr);
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        acc0 += v[u];
        acc1 += v[u + 1];
      }
    }
    for (; b < rows; b += WAVES) acc0 += ld4(src + (size_t)b * ldr);
  }
  return acc0 + acc1;
}

}  // namespace gr
