// gr_offline.hip — the offline auxiliary-head stage (gr_offline_collect / gr_offline_pgd_step, include/gr.h).
//
// Reference: standalone/offline/data_collector.py:124-146 (the balanced collector: per env step the positive rows,
// then at most as many zero-label rows, both in row order, until the dataset is full; there nonzero(), boolean-index
// slices and .cpu().numpy() copies every step) and standalone/offline/train.py:11-31,84-123 (pgd_attack and the
// fine-tune loop of the Linear(192, 1) head under BCEWithLogitsLoss and Adam; there ~50 launches per 256-row batch).
//
//   collect_plan : one 1024-thread workgroup.  Pass 1 counts the positives; with the cursor that fixes how many
//                  positive (P) and zero-label (Q) rows this call keeps.  Pass 2 walks the rows in 1024-row chunks in
//                  order: a row's rank among its kind = the running base + the earlier waves' counts + the popcount of
//                  the wave's ballot below its lane; ranks < P (< Q) get the slot rank (P + rank) of the call's window
//                  -> scratch [header | source row of each slot].  Thread 0 advances the cursor.
//   collect_copy : one wave per slot copies d floats and the label byte (64-bit dataset offsets).
//   pgd_rows<T>  : one wave per row, lane l holds columns l + 64 t (t < T): the PGD iterations in registers (the dot
//                  product = per-lane sums over t, then a butterfly over the lanes: the same value in every lane), then
//                  the row's loss and gradient terms added to the wave's sums in row order.  The workgroup's 4 waves
//                  are summed in wave order -> one partial row [gw (d) | gb | loss] per workgroup.
//   pgd_final    : one workgroup: element e = the partial rows summed in a fixed order (lane l: rows l, l + 64, ..;
//                  then the butterfly), / rows, then torch.optim.Adam's update (the arithmetic of gr_update.hip's
//                  adam_update), the step count and the loss accumulator.
// No atomics, every sum in a fixed order: bit-reproducible.  Plain C++/HIP, wave64.
#include <hip/hip_runtime.h>

#include "../../include/gr.h"

namespace gr {
namespace offline {

constexpr int PLAN_THREADS = 1024;
constexpr int PLAN_WAVES = PLAN_THREADS / 64;
constexpr int HDR = 4;  // scratch header: slots of this call, positives among them, the cursor on entry (lo, hi)
constexpr int COPY_WAVES = 4;
constexpr int COPY_MAX_BLOCKS = 1024;
constexpr long long MAX_ROWS = 1LL << 30;  // (row indices and their strides stay inside int32)

__global__ __launch_bounds__(PLAN_THREADS) void collect_plan(const float* __restrict__ aux, long long ld_aux, int n,
                                                             long long capacity, long long* __restrict__ cursor,
                                                             int* __restrict__ scratch) {
  __shared__ int wp[PLAN_WAVES], wq[PLAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long w = cursor[0];
  // ---- pass 1: the positives of this step
  int cnt = 0;
  for (int i = tid; i < n; i += PLAN_THREADS) cnt += aux[(long long)i * ld_aux] != 0.0f ? 1 : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) wp[wave] = cnt;
  __syncthreads();
  int np = 0;
#pragma unroll
  for (int k = 0; k < PLAN_WAVES; ++k) np += wp[k];
  __syncthreads();  // wp is reused below; every thread has read cursor[0]
  // ---- how many of each kind are kept (data_collector.py:128-143)
  long long room = capacity - w;
  room = room < 0 ? 0 : room;
  long long sp = np;
  if (np > 0 && w + np >= capacity) sp = room;
  long long sq = (long long)n - np;
  sq = sq > sp ? sp : sq;
  if (w + sp + sq >= capacity) sq = capacity - (w + sp);
  sq = sq < 0 ? 0 : sq;
  const int P = (int)sp, Q = (int)sq;
  // ---- pass 2: ranks in row order -> the source row of every slot
  int basep = 0, baseq = 0;
  for (int c = 0; c < n && (basep < P || baseq < Q); c += PLAN_THREADS) {
    const int i = c + tid;
    const bool valid = i < n;
    const float a = valid ? aux[(long long)i * ld_aux] : 0.0f;
    const bool pos = valid && a != 0.0f, neg = valid && !(a != 0.0f);
    const unsigned long long bp = __ballot(pos), bq = __ballot(neg);
    if (lane == 0) {
      wp[wave] = __popcll(bp);
      wq[wave] = __popcll(bq);
    }
    __syncthreads();
    int prep = 0, preq = 0, totp = 0, totq = 0;
#pragma unroll
    for (int k = 0; k < PLAN_WAVES; ++k) {
      const int cp = wp[k], cq = wq[k];
      prep += k < wave ? cp : 0;
      preq += k < wave ? cq : 0;
      totp += cp;
      totq += cq;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (pos) {
      const int r = basep + prep + __popcll(bp & below);
      if (r < P) scratch[HDR + r] = i;
    }
    if (neg) {
      const int r = baseq + preq + __popcll(bq & below);
      if (r < Q) scratch[HDR + P + r] = i;
    }
    basep += totp;
    baseq += totq;
    __syncthreads();  // the next chunk overwrites wp / wq
  }
  if (tid == 0) {
    scratch[0] = P + Q;
    scratch[1] = P;
    scratch[2] = (int)(unsigned)((unsigned long long)w & 0xffffffffull);
    scratch[3] = (int)(unsigned)((unsigned long long)w >> 32);
    cursor[0] = w + P + Q;
    cursor[1] += P;
    cursor[2] += Q;
  }
}

__global__ __launch_bounds__(COPY_WAVES * 64) void collect_copy(const float* __restrict__ feat, long long ld_feat,
                                                                int d, float* __restrict__ features,
                                                                int8_t* __restrict__ supervision,
                                                                const int* __restrict__ scratch) {
  const int S = scratch[0], P = scratch[1];
  const long long w = (long long)(((unsigned long long)(unsigned)scratch[3] << 32) | (unsigned)scratch[2]);
  const int lane = threadIdx.x & 63;
  const int total = gridDim.x * COPY_WAVES;
  for (int s = blockIdx.x * COPY_WAVES + (threadIdx.x >> 6); s < S; s += total) {
    const float* __restrict__ in = feat + (long long)scratch[HDR + s] * ld_feat;
    float* __restrict__ out = features + (w + s) * (long long)d;
    for (int j = lane; j < d; j += 64) out[j] = in[j];
    if (lane == 0) supervision[w + s] = s < P ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ PGD fine-tune step
constexpr int PGD_WAVES = 4;
constexpr int PGD_MAX_BLOCKS = 256;
constexpr int FIN_THREADS = 1024;

static int pgd_blocks(long long rows) {
  const long long t = (rows + PGD_WAVES - 1) / PGD_WAVES;
  return t < PGD_MAX_BLOCKS ? (t < 1 ? 1 : (int)t) : PGD_MAX_BLOCKS;
}
// floats of a workgroup's partial row [gw (d) | gb | loss], padded to 4
__host__ __device__ constexpr int pgd_row(int d) { return (d + 2 + 3) & ~3; }

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

template <int T>
__global__ __launch_bounds__(PGD_WAVES * 64) void pgd_rows(const float* __restrict__ features,
                                                          const int8_t* __restrict__ supervision,
                                                          const long long* __restrict__ index, int rows, int d,
                                                          const float* __restrict__ wb, float epsilon, float alpha,
                                                          int iters, float* __restrict__ partial,
                                                          float* __restrict__ x_adv) {
  constexpr int W = 64 * T;
  __shared__ float red[PGD_WAVES][W + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wv[T], sw[T], gw[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int j = lane + 64 * t;
    wv[t] = j < d ? wb[j] : 0.0f;
    sw[t] = sgn(wv[t]);
    gw[t] = 0.0f;
  }
  const float bias = wb[d];
  float gb = 0.0f, ls = 0.0f;
  const int total = gridDim.x * PGD_WAVES;
  for (int r = blockIdx.x * PGD_WAVES + wave; r < rows; r += total) {
    const long long src = index ? index[r] : (long long)r;
    const float* __restrict__ xr = features + src * (long long)d;
    const float y = (float)supervision[src];
    float x0[T], x[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int j = lane + 64 * t;
      x0[t] = j < d ? xr[j] : 0.0f;  // (columns past d: x = 0, w = 0: they stay 0 and add nothing)
      x[t] = iters > 0 ? x0[t] : clampf(x0[t], 0.0f, 1.0f);  // (no iteration: only the feature clamp)
    }
    float z = 0.0f;
    for (int it = 0; it <= iters; ++it) {
      // z = w.x + b on the current x (the last pass: the final x)
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < T; ++t) acc += wv[t] * x[t];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
      z = acc + bias;
      if (it == iters) break;
      const float sg = sgn(sigmoidf(z) - y);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float xa = x[t] + alpha * (sg * sw[t]);
        const float p = clampf(xa - x0[t], -epsilon, epsilon);
        x[t] = clampf(x0[t] + p, 0.0f, 1.0f);
      }
    }
    const float g = sigmoidf(z) - y;
    // BCEWithLogits: softplus(z) - y z = max(z, 0) - y z + log1p(exp(-|z|))
    ls += (fmaxf(z, 0.0f) - y * z) + log1pf(expf(-fabsf(z)));
    gb += g;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      gw[t] += g * x[t];
      const int j = lane + 64 * t;
      if (x_adv && j < d) x_adv[(long long)r * d + j] = x[t];
    }
  }
  // ---- the workgroup's partial row: the waves in order
#pragma unroll
  for (int t = 0; t < T; ++t) red[wave][lane + 64 * t] = gw[t];
  if (lane == 0) {
    red[wave][W] = gb;
    red[wave][W + 1] = ls;
  }
  __syncthreads();
  float* __restrict__ pr = partial + (size_t)blockIdx.x * pgd_row(d);
  for (int e = threadIdx.x; e < d + 2; e += PGD_WAVES * 64) {
    const int c = e < d ? e : W + (e - d);
    float v = red[0][c];
#pragma unroll
    for (int k = 1; k < PGD_WAVES; ++k) v += red[k][c];
    pr[e] = v;
  }
}

// element e of [gw | gb | loss]: its partial rows in a fixed order, / rows; Adam on wb [d + 1] (torch's lerp,
// addcmul, addcdiv: gr_update.hip adam_update), step += 1, loss_acc += loss * rows
__global__ __launch_bounds__(FIN_THREADS) void pgd_final(const float* __restrict__ partial, int blocks, int rows, int d,
                                                         float* __restrict__ wb, float* __restrict__ exp_avg,
                                                         float* __restrict__ exp_avg_sq, float* __restrict__ step,
                                                         double lr, double beta1, double beta2, float eps,
                                                         double* __restrict__ loss_acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld = pgd_row(d);
  const float t = step[0] + 1.0f;
  __syncthreads();  // every thread has read the count before thread 0 stores it
  for (int e = wave; e < d + 2; e += FIN_THREADS / 64) {
    float v = 0.0f;
    for (int b = lane; b < blocks; b += 64) v += partial[(size_t)b * ld + e];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    if (lane != 0) continue;
    const float gr = v / (float)rows;
    if (e == d + 1) {
      loss_acc[0] += (double)gr * (double)rows;
      continue;
    }
    const float step_size = (float)(lr / (1.0 - pow(beta1, (double)t)));
    const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)t));
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
    float m = exp_avg[e], s = exp_avg_sq[e];
    m = m + w1 * (gr - m);
    s = s * b2;
    s = s + (w2 * gr) * gr;
    exp_avg[e] = m;
    exp_avg_sq[e] = s;
    const float denom = sqrtf(s) / bc2s + eps;
    wb[e] = wb[e] + (-step_size) * (m / denom);
  }
  if (threadIdx.x == 0) step[0] = t;
}

template <int T>
static void launch_rows(int blocks, hipStream_t s, const float* features, const int8_t* supervision,
                        const long long* index, int rows, int d, const float* wb, float epsilon, float alpha, int iters,
                        float* partial, float* x_adv) {
  hipLaunchKernelGGL((pgd_rows<T>), dim3(blocks), dim3(PGD_WAVES * 64), 0, s, features, supervision, index, rows, d, wb,
                     epsilon, alpha, iters, partial, x_adv);
}

}  // namespace offline
}  // namespace gr

using namespace gr::offline;

extern "C" {

int64_t gr_offline_scratch_ints(int64_t n) {
  if (n < 0 || n > MAX_ROWS) return GR_ERR_ARG;
  return n + HDR;
}

int gr_offline_collect(const float* feat, int64_t ld_feat, const float* aux, int64_t ld_aux, int64_t n, int32_t d,
                       float* features, int8_t* supervision, int64_t capacity, int64_t* cursor, int32_t* scratch,
                       void* stream) {
  if (n < 0 || n > MAX_ROWS || d < 1 || ld_feat < d || ld_aux < 1 || capacity < 1) return GR_ERR_ARG;
  if (!feat || !aux || !features || !supervision || !cursor || !scratch) return GR_ERR_ARG;
  if (n == 0) return GR_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(collect_plan, dim3(1), dim3(PLAN_THREADS), 0, s, aux, (long long)ld_aux, (int)n,
                     (long long)capacity, (long long*)cursor, (int*)scratch);
  if (hipGetLastError() != hipSuccess) return GR_ERR_HIP;
  const int64_t want = (n + COPY_WAVES - 1) / COPY_WAVES;
  const int blocks = want < COPY_MAX_BLOCKS ? (int)want : COPY_MAX_BLOCKS;
  hipLaunchKernelGGL(collect_copy, dim3(blocks), dim3(COPY_WAVES * 64), 0, s, feat, (long long)ld_feat, (int)d,
                     features, supervision, (const int*)scratch);
  return hipGetLastError() == hipSuccess ? GR_OK : GR_ERR_HIP;
}

int64_t gr_offline_pgd_partials(int64_t rows, int32_t d) {
  if (rows < 1 || rows > MAX_ROWS || d < 1 || d > GR_OFFLINE_PGD_MAX_D) return GR_ERR_ARG;
  return (int64_t)pgd_blocks(rows) * pgd_row(d);
}

int gr_offline_pgd_step(const float* features, const int8_t* supervision, const int64_t* index, int64_t rows,
                        int32_t d, float* wb, float* exp_avg, float* exp_avg_sq, float* step, float epsilon,
                        float alpha, int32_t iters, double lr, double beta1, double beta2, float eps, float* partial,
                        double* loss_acc, float* x_adv, void* stream) {
  if (rows < 1 || rows > MAX_ROWS || d < 1 || d > GR_OFFLINE_PGD_MAX_D || iters < 0) return GR_ERR_ARG;
  if (!features || !supervision || !wb || !exp_avg || !exp_avg_sq || !step || !partial || !loss_acc)
    return GR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = pgd_blocks(rows);
  const long long* idx = (const long long*)index;
  const int tiles = (d + 63) / 64;
#define GR_PGD_ROWS(T) \
  launch_rows<T>(blocks, s, features, supervision, idx, (int)rows, (int)d, wb, epsilon, alpha, (int)iters, partial, x_adv)
  if (tiles <= 1) GR_PGD_ROWS(1);
  else if (tiles == 2) GR_PGD_ROWS(2);
  else if (tiles == 3) GR_PGD_ROWS(3);
  else if (tiles == 4) GR_PGD_ROWS(4);
  else if (tiles <= 8) GR_PGD_ROWS(8);
  else GR_PGD_ROWS(16);
#undef GR_PGD_ROWS
  if (hipGetLastError() != hipSuccess) return GR_ERR_HIP;
  hipLaunchKernelGGL(pgd_final, dim3(1), dim3(FIN_THREADS), 0, s, (const float*)partial, blocks, (int)rows, (int)d, wb,
                     exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, loss_acc);
  return hipGetLastError() == hipSuccess ? GR_OK : GR_ERR_HIP;
}

}  // extern "C"
