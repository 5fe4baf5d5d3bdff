// gr_bn.hip — training-mode BatchNorm fused with its activation, on channels-last rows [M][C] (gfx950).
//
// The vision stem (VisionActorCritic, standalone/rsl_rl/ext/modules/vision_actor_critic.py:43-144, here
// rsl_rl/vision_actor_critic.py) runs Conv -> BatchNorm2d -> LeakyReLU three times on [batch*H*W, C]
// matrices with millions of rows and C = 16 / 32 / 64.  PyTorch spends 13 full passes over each such
// matrix per forward + backward (statistics, transform, activation, activation backward, BN backward
// reduce and element passes) and saves both the BN output and the activation output.  Here:
//   forward:  one statistics pass (read x) + one apply pass (read x, write y = act(bn(x)));
//   backward: one reduce pass (read gy, x) + one element pass (read gy, x, write gx);
// the activation's derivative is recomputed from x, so only x is kept for the backward.
//
// Layout: a thread owns one float4 (4 channels) of a row per item and walks the rows with a stride that
// is a multiple of C / 4, so its channel group is fixed (C / 4 must be a power of two dividing 256: C in
// {4, 8, 16, 32, 64}).  Per-channel sums: fp32 per thread over its items, shifted by the channel's value in
// row 0 (no cancellation in E[x^2] - E[x]^2), then fp64 across the block and across blocks in a fixed
// order — deterministic, no atomics, graph-capturable.  (The block geometry and the reductions: gr_bn.h, shared with
// the stem's first block from the image, gr_stem.hip.)
#include "gr_bn.h"

namespace gr {

// ---- forward: shifted channel sums of x
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial(const float* __restrict__ x, long long m, int c,
                                                               double* __restrict__ part) {
  const int c4 = c / 4;
  const long long q0 = (long long)blockIdx.x * BN_THREADS + threadIdx.x, stride = (long long)gridDim.x * BN_THREADS;
  const long long nq = m * c4;
  const float4 sh = ld4f(x, threadIdx.x & (c4 - 1));  // row 0 of this thread's channel group
  float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (long long q = q0; q < nq; q += stride) {
    const float4 v = ld4f(x, q);
    const float d[4] = {v.x - sh.x, v.y - sh.y, v.z - sh.z, v.w - sh.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] += d[k];
      a[4 + k] += d[k] * d[k];
    }
  }
  bn_block_partials(a, c, part);
}

// stats[0][c] mean, [1][c] invstd = 1 / sqrt(var + eps), [2][c] biased var, [3][c] unbiased var
// shift[c]: the per-channel shift of the partial sums (row 0 of x)
__global__ __launch_bounds__(BN_FINAL_THREADS) void bn_stats_final(const float* __restrict__ shift, long long m, int c, int blocks,
                                                             float eps, const double* __restrict__ part,
                                                             float* __restrict__ stats) {
  __shared__ double sums[128];
  bn_final_sums(part, 2 * c, blocks, sums);
  const int ch = threadIdx.x;
  if (ch >= c) return;
  const double md = (double)m, d1 = sums[ch] / md;
  double var = sums[c + ch] / md - d1 * d1;
  var = var > 0.0 ? var : 0.0;
  const float varf = (float)var;
  stats[ch] = (float)((double)shift[ch] + d1);
  stats[c + ch] = 1.0f / sqrtf(varf + eps);
  stats[2 * c + ch] = varf;
  stats[3 * c + ch] = m > 1 ? (float)(var * md / (md - 1.0)) : varf;
}

// ---- forward: y = act((x - mean) * invstd * w + b)
template <int ACT>
__global__ __launch_bounds__(BN_THREADS) void bn_apply(const float* __restrict__ x, long long m, int c,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       const float* __restrict__ stats, float slope, float* __restrict__ y) {
  const int c4 = c / 4, g = threadIdx.x & (c4 - 1);
  const float4 mu = ld4f(stats, g), is = ld4f(stats + c, g), wv = ld4f(w, g), bv = ld4f(b, g);
  const long long nq = m * c4, stride = (long long)gridDim.x * BN_THREADS;
  for (long long q = (long long)blockIdx.x * BN_THREADS + threadIdx.x; q < nq; q += stride) {
    const float4 v = ld4f(x, q);
    float4 o;
    o.x = bn_act<ACT>((v.x - mu.x) * is.x * wv.x + bv.x, slope);
    o.y = bn_act<ACT>((v.y - mu.y) * is.y * wv.y + bv.y, slope);
    o.z = bn_act<ACT>((v.z - mu.z) * is.z * wv.z + bv.z, slope);
    o.w = bn_act<ACT>((v.w - mu.w) * is.w * wv.w + bv.w, slope);
    reinterpret_cast<float4*>(y)[q] = o;
  }
}

// ---- backward: per channel sum(gz), sum(gz * xhat), gz = gy * act'(z)
template <int ACT>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_partial(const float* __restrict__ x, const float* __restrict__ gy,
                                                             long long m, int c, const float* __restrict__ w,
                                                             const float* __restrict__ b, const float* __restrict__ stats,
                                                             float slope, double* __restrict__ part) {
  const int c4 = c / 4, g = threadIdx.x & (c4 - 1);
  const float4 mu = ld4f(stats, g), is = ld4f(stats + c, g), wv = ld4f(w, g), bv = ld4f(b, g);
  const long long nq = m * c4, stride = (long long)gridDim.x * BN_THREADS;
  float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (long long q = (long long)blockIdx.x * BN_THREADS + threadIdx.x; q < nq; q += stride) {
    const float4 v = ld4f(x, q), dy = ld4f(gy, q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = (comp(v, k) - comp(mu, k)) * comp(is, k);
      const float gz = comp(dy, k) * bn_dact<ACT>(xh * comp(wv, k) + comp(bv, k), slope);
      a[k] += gz;
      a[4 + k] += gz * xh;
    }
  }
  bn_block_partials(a, c, part);
}

// sums[0][c] = sum gz (= grad bias), sums[1][c] = sum gz * xhat (= grad weight)
__global__ __launch_bounds__(BN_FINAL_THREADS) void bn_bwd_final(int c, int blocks, const double* __restrict__ part,
                                                           float* __restrict__ gw, float* __restrict__ gb,
                                                           float* __restrict__ sums) {
  __shared__ double tot[128];
  bn_final_sums(part, 2 * c, blocks, tot);
  const int ch = threadIdx.x;
  if (ch >= c) return;
  sums[ch] = (float)tot[ch];
  sums[c + ch] = (float)tot[c + ch];
  gb[ch] = (float)tot[ch];
  gw[ch] = (float)tot[c + ch];
}

// gx = (gz - sum(gz) / M - xhat * sum(gz xhat) / M) * invstd * w
template <int ACT>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_elemt(const float* __restrict__ x, const float* __restrict__ gy,
                                                           long long m, int c, const float* __restrict__ w,
                                                           const float* __restrict__ b, const float* __restrict__ stats,
                                                           const float* __restrict__ sums, float slope,
                                                           float* __restrict__ gx) {
  const int c4 = c / 4, g = threadIdx.x & (c4 - 1);
  const float4 mu = ld4f(stats, g), is = ld4f(stats + c, g), wv = ld4f(w, g), bv = ld4f(b, g);
  const float inv_m = 1.0f / (float)m;
  const float4 s1 = ld4f(sums, g), s2 = ld4f(sums + c, g);
  const float mg[4] = {s1.x * inv_m, s1.y * inv_m, s1.z * inv_m, s1.w * inv_m};
  const float mgx[4] = {s2.x * inv_m, s2.y * inv_m, s2.z * inv_m, s2.w * inv_m};
  const long long nq = m * c4, stride = (long long)gridDim.x * BN_THREADS;
  for (long long q = (long long)blockIdx.x * BN_THREADS + threadIdx.x; q < nq; q += stride) {
    const float4 v = ld4f(x, q), dy = ld4f(gy, q);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = (comp(v, k) - comp(mu, k)) * comp(is, k);
      const float gz = comp(dy, k) * bn_dact<ACT>(xh * comp(wv, k) + comp(bv, k), slope);
      o[k] = (gz - mg[k] - xh * mgx[k]) * (comp(is, k) * comp(wv, k));
    }
    reinterpret_cast<float4*>(gx)[q] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

int bn_scratch_doubles(long long m, int c) { return bn_blocks(m, c) * 2 * c + 2 * c; }

// the running-statistics update of `uses` training-mode forwards over the same rows (F.batch_norm's, as
// fused_bn._update_running made it with torch's ops: r = r * keep, then r + momentum * batch stat, per forward), and
// num_batches_tracked + count: one launch instead of five per BatchNorm and forward
__global__ void bn_running_update(float* __restrict__ rm, float* __restrict__ rv, long long* __restrict__ nbt,
                                  const float* __restrict__ stats, int c, float keep, float momentum, int uses,
                                  int count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < c) {
    const float mean = stats[j], var = stats[3 * c + j];
    float a = rm[j], v = rv[j];
    for (int u = 0; u < uses; ++u) {
      a = __fmaf_rn(momentum, mean, a * keep);
      v = __fmaf_rn(momentum, var, v * keep);
    }
    rm[j] = a;
    rv[j] = v;
  }
  if (j == 0 && nbt) nbt[0] += count;
}

hipError_t launch_bn_running_update(float* rm, float* rv, long long* nbt, const float* stats, int c, float keep,
                                    float momentum, int uses, int count, hipStream_t s) {
  hipLaunchKernelGGL(bn_running_update, dim3((c + 63) / 64), dim3(64), 0, s, rm, rv, nbt, stats, c, keep, momentum,
                     uses, count);
  return hipGetLastError();
}

void launch_bn_stats_final(const float* shift, long long m, int c, int blocks, float eps, const double* part,
                           float* stats, hipStream_t s) {
  hipLaunchKernelGGL(bn_stats_final, dim3(1), dim3(BN_FINAL_THREADS), 0, s, shift, m, c, blocks, eps, part, stats);
}
void launch_bn_bwd_final(int c, int blocks, const double* part, float* gw, float* gb, float* sums, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_final, dim3(1), dim3(BN_FINAL_THREADS), 0, s, c, blocks, part, gw, gb, sums);
}

hipError_t launch_bn_stats(const float* x, long long m, int c, float eps, float* stats, double* part, hipStream_t s) {
  const int nb = bn_blocks(m, c);
  hipLaunchKernelGGL(bn_stats_partial, dim3(nb), dim3(BN_THREADS), 0, s, x, m, c, part);
  launch_bn_stats_final(x, m, c, nb, eps, part, stats, s);  // shift: row 0 of x
  return hipGetLastError();
}

hipError_t launch_bn_forward(const float* x, long long m, int c, const float* w, const float* b, float eps, int act,
                             float slope, float* y, float* stats, double* part, hipStream_t s) {
  const int nb = bn_blocks(m, c);
  hipLaunchKernelGGL(bn_stats_partial, dim3(nb), dim3(BN_THREADS), 0, s, x, m, c, part);
  launch_bn_stats_final(x, m, c, nb, eps, part, stats, s);  // shift: row 0 of x
  pick_act(act, [&](auto a) {
    hipLaunchKernelGGL(bn_apply<decltype(a)::value>, dim3(nb), dim3(BN_THREADS), 0, s, x, m, c, w, b, stats, slope, y);
  });
  return hipGetLastError();
}

hipError_t launch_bn_backward(const float* x, const float* gy, long long m, int c, const float* w, const float* b,
                              const float* stats, int act, float slope, float* gx, float* gw, float* gb, double* part,
                              hipStream_t s) {
  const int nb = bn_blocks(m, c);
  // the two channel sums live after the partials in the same workspace (as floats)
  float* sums = reinterpret_cast<float*>(part + (size_t)nb * 2 * c);
  pick_act(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    hipLaunchKernelGGL(bn_bwd_partial<ACT>, dim3(nb), dim3(BN_THREADS), 0, s, x, gy, m, c, w, b, stats, slope, part);
    launch_bn_bwd_final(c, nb, part, gw, gb, sums, s);
    hipLaunchKernelGGL(bn_bwd_elemt<ACT>, dim3(nb), dim3(BN_THREADS), 0, s, x, gy, m, c, w, b, stats, sums, slope, gx);
  });
  return hipGetLastError();
}

}  // namespace gr
