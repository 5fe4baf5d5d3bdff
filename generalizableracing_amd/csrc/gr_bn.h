// gr_bn.h — what the BatchNorm + activation op (gr_bn.hip) and the vision stem's first block (gr_stem.hip) share:
// the block geometry, the activation and its derivative, the fixed-order fp64 block / final reductions, and the
// run-time activation as a template argument.  Included by those two sources only (it defines device functions).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/gr.h"
#include "gr_kernels.h"

namespace gr {

constexpr int BN_THREADS = 256;
#ifndef GR_BN_MAX_BLOCKS
#define GR_BN_MAX_BLOCKS 1024
#endif
constexpr int BN_MAX_BLOCKS = GR_BN_MAX_BLOCKS;  // blocks per pass (partial rows of the fixed-order reductions)

__host__ __device__ inline int bn_blocks(long long m, int c) {
  const long long q = m * (c / 4);
  long long b = (q + BN_THREADS * 8 - 1) / (BN_THREADS * 8);  // ~8 float4 per thread at least
  if (b < 1) b = 1;
  return (int)(b < BN_MAX_BLOCKS ? b : BN_MAX_BLOCKS);
}

template <int ACT>
__device__ __forceinline__ float bn_act(float z, float slope) {
  if constexpr (ACT == GR_POLICY_ACT_ELU) return z > 0.0f ? z : expm1f(z);
  return z > 0.0f ? z : z * slope;
}
// d act / d z, from z (torch's leaky_relu_backward tests the input; ELU's uses the output y = expm1(z))
template <int ACT>
__device__ __forceinline__ float bn_dact(float z, float slope) {
  if constexpr (ACT == GR_POLICY_ACT_ELU) return z > 0.0f ? 1.0f : expm1f(z) + 1.0f;
  return z > 0.0f ? 1.0f : slope;
}

__device__ __forceinline__ float4 ld4f(const float* p, long long q) { return reinterpret_cast<const float4*>(p)[q]; }
__device__ __forceinline__ float comp(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// block reduction of 8 per-thread sums (two quantities x 4 channels) over the threads of each channel group,
// in fp64, then one row of partials per block: part[block][2][C]
__device__ void bn_block_partials(const float a[8], int c, double* part) {
  __shared__ double red[BN_THREADS * 8];
  const int t = threadIdx.x, c4 = c / 4;
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k * BN_THREADS + t] = (double)a[k];
  __syncthreads();
  // thread (quantity s, channel ch) sums the threads t' with t' % c4 == ch / 4 in index order
  for (int j = t; j < 2 * c; j += BN_THREADS) {
    const int s = j / c, ch = j % c, g = ch / 4, k = ch % 4;
    double acc = 0.0;
    for (int u = g; u < BN_THREADS; u += c4) acc += red[(s * 4 + k) * BN_THREADS + u];
    part[(size_t)blockIdx.x * 2 * c + j] = acc;
  }
}

// sums over the blocks' partials of `npairs` quantities (part[block][npairs]), in a fixed order: thread
// (pair j, lane k) of the BN_FINAL_THREADS sums the partials b = k (mod T), T = BN_FINAL_THREADS / npairs
// threads per pair, 32 (then 8) loads in flight at a time (the partials come from L2 / HBM: one load at a time left
// a 1 024-block reduction latency-bound at ~70 us), then lane 0 of each pair adds the T lane sums in order.
// Thread index = k * npairs + j: consecutive threads read consecutive pairs of one partial row (coalesced; with
// j = t / T a wave's load touched 16 rows, and the final took ~30 us for 1 024 rows of 32 pairs)
constexpr int BN_FINAL_THREADS = 1024;
__device__ void bn_final_sums(const double* __restrict__ part, int npairs, int blocks, double* out, int stride = 0) {
  __shared__ double red[BN_FINAL_THREADS];
  if (stride == 0) stride = npairs;  // (the partial rows' length, when the pairs are a slice of a longer row)
  const int T = BN_FINAL_THREADS / npairs, j = threadIdx.x % npairs, k = threadIdx.x / npairs;
  double acc = 0.0;
  if (k < T) {
    int b = k;
    // 32 loads in flight: the partials were just written by blocks on every XCD, so each round trip is a
    // far-memory latency (8 at a time left the final at ~29 us for 1 024 partial rows, profiles/round05_*)
    for (; b + 31 * T < blocks; b += 32 * T) {
      double v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = part[(size_t)(b + u * T) * stride + j];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += v[u];
    }
    for (; b + 7 * T < blocks; b += 8 * T) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(b + u * T) * stride + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; b < blocks; b += T) acc += part[(size_t)b * stride + j];
    red[j * T + k] = acc;
  }
  __syncthreads();
  if (j < npairs && k == 0) {
    double s = 0.0;
    for (int u = 0; u < T; ++u) s += red[j * T + u];
    out[j] = s;
  }
  __syncthreads();
}

// ---- host side
// a run-time choice as a template argument: f(std::integral_constant) for the activation, f(std::bool_constant) for a
// flag.  Every launcher of a kernel templated on them goes through these (the results of both branches: one type)
template <int V>
using int_c = std::integral_constant<int, V>;
template <class F>
inline auto pick_act(int act, F&& f) {
  return act == GR_POLICY_ACT_ELU ? f(int_c<GR_POLICY_ACT_ELU>{}) : f(int_c<GR_POLICY_ACT_LRELU>{});
}
template <class F>
inline auto pick_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

// the single-block finals of gr_bn.hip, which the stem's passes end in too (their partial rows have its layout)
void launch_bn_stats_final(const float* shift, long long m, int c, int blocks, float eps, const double* part,
                           float* stats, hipStream_t s);
void launch_bn_bwd_final(int c, int blocks, const double* part, float* gw, float* gb, float* sums, hipStream_t s);

}  // namespace gr
