// pm_pool_head.h -- the f32 kernels the linear probe (pm_probe.hip) and the end-to-end fine-tune (pm_finetune.hip) share: the two-stage
// mean over the patch rows through fc_norm (models_vit.py:46-48) and the Linear head's forward.  Fixed summation order, no float
// atomics.  Everything has internal linkage: each of the two translation units holds its own copy of what it launches.
//
//   pool_partial_kernel   the one HBM-bound pass: x [B, N, D] is read once, kPoolRows patch rows per workgroup as 16-byte loads, four
//                         rows in flight.
//   pool_norm_kernel      one workgroup per sample adds the partial rows in ascending order, divides by N - 1 and applies LayerNorm.
//                         <true> also leaves the pooled row and mean / rstd for the backward; feat has the bits of <false>.
//   linear_kernel         logits = in W^T + bias: one wave per (sample, class), 16 classes per wave.
#pragma once
#include "pm_common.h"

namespace {

constexpr int kPoolThreads = 256;
constexpr int kMaxD = 2048;     // two 16-byte vectors per lane in pool_norm_kernel
constexpr int kPoolRows = 32;   // patch rows per first-stage workgroup

inline int pool_splits(int N) { return (N - 1 + kPoolRows - 1) / kPoolRows; }
// the partial rows of pool_partial_kernel (pm_pool_norm_workspace)
inline size_t pool_workspace_bytes(int B, int N, int D) { return (size_t)B * pool_splits(N) * D * sizeof(float); }

// workgroup (b, s): partial[b][s][:] = sum of rows 1 + s kPoolRows ... of sample b, ascending
__global__ __launch_bounds__(kPoolThreads) void pool_partial_kernel(const float* __restrict__ x, int N, int D, int S,
                                                                    float* __restrict__ partial) {
  const int b = blockIdx.x / S, s = blockIdx.x % S;
  const int n0 = 1 + s * kPoolRows;
  const int n1 = n0 + kPoolRows < N ? n0 + kPoolRows : N;
  const float* base = x + (long)b * N * D;
  float* out = partial + (long)blockIdx.x * D;
  for (int c = threadIdx.x * 4; c < D; c += kPoolThreads * 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int n = n0;
    for (; n + 3 < n1; n += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(base + (long)(n + u) * D + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += v[u];
    }
    for (; n < n1; ++n) acc += *reinterpret_cast<const f32x4*>(base + (long)n * D + c);
    *reinterpret_cast<f32x4*>(out + c) = acc;
  }
}

// workgroup b: pooled = (partial rows in ascending order) / (N - 1), then LayerNorm over D.  kTrain: pooled / mean_out / rstd_out are
// stored too (they are not touched otherwise)
template <bool kTrain>
__global__ __launch_bounds__(kPoolThreads) void pool_norm_kernel(const float* __restrict__ partial, int N, int D, int S,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float eps, float* __restrict__ feat, float* __restrict__ pooled,
                                                                 float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  __shared__ float red[kPoolThreads / PM_WAVE];
  const int b = blockIdx.x;
  const float* rows = partial + (long)b * S * D;
  const float den = (float)(N - 1);
  f32x4 v[2];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (threadIdx.x + j * kPoolThreads) * 4;
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < D) {
      for (int s = 0; s < S; ++s) v[j] += *reinterpret_cast<const f32x4*>(rows + (long)s * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[j][e] = v[j][e] / den;
        sum += v[j][e];
      }
    }
  }
  const float mean = block_sum(sum, red) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (threadIdx.x + j * kPoolThreads) * 4;
    if (c < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[j][e] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(block_sum(q, red) / (float)D + eps);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (threadIdx.x + j * kPoolThreads) * 4;
    if (c < D) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (v[j][e] - mean) * rstd * g[e] + bt[e];
      *reinterpret_cast<f32x4*>(feat + (long)b * D + c) = y;
      if constexpr (kTrain) *reinterpret_cast<f32x4*>(pooled + (long)b * D + c) = v[j];
    }
  }
  if constexpr (kTrain) {
    if (threadIdx.x == 0) {
      mean_out[b] = mean;
      rstd_out[b] = rstd;
    }
  }
}

// logits[b][c] = sum_d in[b][d] W[c][d] + bias[c]; workgroup (class strip of 64, b), wave w owns 16 classes
__global__ __launch_bounds__(kPoolThreads) void linear_kernel(const float* __restrict__ in, const float* __restrict__ W,
                                                              const float* __restrict__ bias, int D, int C, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const float* xr = in + (long)b * D;
  for (int i = 0; i < 16; ++i) {
    const int c = blockIdx.x * 64 + wave * 16 + i;
    if (c >= C) return;  // (wave-uniform; no barrier below)
    const float* wr = W + (long)c * D;
    float acc = 0.f;
    for (int k = lane * 4; k < D; k += 64 * 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xr + k), w = *reinterpret_cast<const f32x4*>(wr + k);
      acc += a[0] * w[0];
      acc += a[1] * w[1];
      acc += a[2] * w[2];
      acc += a[3] * w[3];
    }
    acc = wave_sum(acc);
    if (lane == 0) logits[(long)b * C + c] = acc + bias[c];
  }
}

}  // namespace
