// pm_probe.hip -- the MAE linear-probe protocol beside the frozen encoder (include/polypmae.h: pm_pool_norm_fwd, pm_probe_head_fwd,
// pm_probe_ce, pm_probe_head_bwd, pm_lars_step).
//
// The reference scores a pre-trained encoder with main_linprobe.py: the features of the frozen ViT (the cls token, or with
// --global_pool the mean of the patch tokens through fc_norm, models_vit.py:46-48) go through BatchNorm1d(affine=False, eps=1e-6)
// and one Linear (main_linprobe.py:244), the loss is torch.nn.CrossEntropyLoss(), the optimiser is LARS (util/lars.py) over the
// Linear's two tensors, and engine_finetune.evaluate reports acc@1 / acc@5.  Everything here is f32 with a fixed summation order
// (no float atomics: two-stage sums with fixed trees), takes its stream, allocates nothing and checks its shapes on the host
// before the first launch.
//
//   pool_partial_kernel / pool_norm_kernel<false>, linear_kernel     pm_pool_head.h, shared with pm_finetune.hip: the global_pool
//                                            feature, and logits = xhat W^T + bias.
//   bn_kernel                                64 feature columns x 16 row groups per workgroup: batch mean, biased variance (two
//                                            passes: the deviations from the mean), xhat, the running statistics of
//                                            torch.nn.BatchNorm1d (momentum, unbiased variance), the int64 counter.
//   ce_rows_kernel / ce_finish_kernel        one wave per sample: log-sum-exp, the row's loss, dlogits x s / B, the number of
//                                            classes strictly above the target's logit; then one workgroup adds up the rows.
//   head_dw_kernel / head_dbias_kernel       dW += dlogits^T xhat, dbias += sum_b dlogits: 4 row groups per column, combined as
//                                            (r0 + r1) + (r2 + r3), ONE addition into what dW / dbias held (accum_iter).
//   lars_norms_kernel / lars_update_kernel   util/lars.py:22-47 over a segment table: |p|^2 and |g + wd p|^2 in f64, kLarsRows
//                                            partial rows per segment by a map that depends on the segment's length alone, then
//                                            q, mu = m mu + q dp, p -= lr mu.  lr / wd / m / trust coefficient are read from a
//                                            device record, so a captured step replays with a new lr.
#include <math.h>

#include "pm_pool_head.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PM_WAVE;
constexpr int kLarsRows = 32;    // partial rows per segment
constexpr int kLarsBatch = 32;   // segments per launch (they travel as kernel arguments)
constexpr int kLarsMaxBlocks = 256;

// ------------------------------------------------------------------------------------------------ BatchNorm1d(affine=False)
// 64 columns x 16 row groups; row group g owns rows g, g + 16, ...; the groups are combined in the order 0..15
__global__ __launch_bounds__(1024) void bn_kernel(const float* __restrict__ feat, int B, int D, float* __restrict__ running_mean,
                                                  float* __restrict__ running_var, long long* __restrict__ tracked, int training,
                                                  float momentum, float eps, float* __restrict__ xhat) {
  __shared__ float red[16][64];
  __shared__ float s_mean[64], s_rstd[64];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const bool live = d < D;
  if (training) {
    red[rg][lane] = live ? strided_sum<4>(feat + d, D, rg, 16, B) : 0.f;
    __syncthreads();
    if (rg == 0) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) t += red[g][lane];
      s_mean[lane] = t / (float)B;
    }
    __syncthreads();
    const float mean = s_mean[lane];
    float q = 0.f;
    if (live) {
      for (int b = rg; b < B; b += 16) {
        const float dv = feat[(long)b * D + d] - mean;
        q += dv * dv;
      }
    }
    red[rg][lane] = q;
    __syncthreads();
    if (rg == 0) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) t += red[g][lane];
      s_rstd[lane] = rsqrtf(t / (float)B + eps);
      if (live) {  // torch.nn.BatchNorm1d: running = (1 - momentum) running + momentum new, the variance unbiased
        running_mean[d] = (1.0f - momentum) * running_mean[d] + momentum * mean;
        running_var[d] = (1.0f - momentum) * running_var[d] + momentum * (t / (float)(B - 1));
      }
    }
    __syncthreads();
  } else {
    if (rg == 0) {
      s_mean[lane] = live ? running_mean[d] : 0.f;
      s_rstd[lane] = live ? rsqrtf(running_var[d] + eps) : 0.f;
    }
    __syncthreads();
  }
  if (live) {
    const float mean = s_mean[lane], rstd = s_rstd[lane];
    for (int b = rg; b < B; b += 16) xhat[(long)b * D + d] = (feat[(long)b * D + d] - mean) * rstd;
  }
  if (training && blockIdx.x == 0 && threadIdx.x == 0) *tracked += 1;
}

// ------------------------------------------------------------------------------------------------ cross-entropy + accuracy
// one wave per row.  row_hits: bit 0 correct at 1, bit 1 correct at k.  A target outside [0, C) poisons the loss with NaN, counts
// as wrong and gets a zero gradient row (torch raises there).
__global__ __launch_bounds__(kThreads) void ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ target, int B,
                                                           int C, int topk, const float* __restrict__ scale, float* __restrict__ dlogits,
                                                           float* __restrict__ row_loss, int* __restrict__ row_hits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kWaves + wave;
  if (row >= B) return;  // (wave-uniform; no barrier below)
  const float* z = logits + (long)row * C;
  const long long t = target[row];
  const bool valid = t >= 0 && t < (long long)C;
  const float zt = valid ? z[t] : 0.f;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
  m = wave_max(m);
  float se = 0.f;
  int above = 0;
  for (int c = lane; c < C; c += 64) {
    se += expf(z[c] - m);
    above += z[c] > zt ? 1 : 0;
  }
  se = wave_sum(se);
  above = wave_sum_int(above);
  if (lane == 0) {
    row_loss[row] = valid ? (m + logf(se)) - zt : NAN;
    row_hits[row] = valid ? ((above < 1 ? 1 : 0) | (above < topk ? 2 : 0)) : 0;
  }
  if (dlogits) {
    const float g = scale[0] / (float)B;
    const float rse = 1.0f / se;
    for (int c = lane; c < C; c += 64) {
      const float p = expf(z[c] - m) * rse;
      dlogits[(long)row * C + c] = valid ? (p - (c == (int)t ? 1.0f : 0.f)) * g : 0.f;
    }
  }
}

// loss = (rows in a fixed order) / B; the two counters (integers: any order)
__global__ __launch_bounds__(kThreads) void ce_finish_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_hits, int B,
                                                             float* __restrict__ loss, long long* __restrict__ correct) {
  __shared__ float red[kWaves];
  __shared__ int hits[2][kWaves];
  float s = 0.f;
  int h1 = 0, hk = 0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    s += row_loss[b];
    h1 += row_hits[b] & 1;
    hk += (row_hits[b] >> 1) & 1;
  }
  const float total = block_sum(s, red);
  h1 = wave_sum_int(h1);
  hk = wave_sum_int(hk);
  if ((threadIdx.x & 63) == 0) {
    hits[0][threadIdx.x >> 6] = h1;
    hits[1][threadIdx.x >> 6] = hk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = total / (float)B;
    correct[0] = (long long)(hits[0][0] + hits[0][1] + hits[0][2] + hits[0][3]);
    correct[1] = (long long)(hits[1][0] + hits[1][1] + hits[1][2] + hits[1][3]);
  }
}

// ------------------------------------------------------------------------------------------------ head backward
// workgroup (column strip of 64, class c): 4 row groups, group g owns rows g, g + 4, ...
__global__ __launch_bounds__(kThreads) void head_dw_kernel(const float* __restrict__ dlogits, const float* __restrict__ xhat, int B, int D,
                                                           int C, float* __restrict__ dW) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane, c = blockIdx.y;
  float acc = 0.f;
  if (d < D) {
    for (int b = rg; b < B; b += 4) acc += dlogits[(long)b * C + c] * xhat[(long)b * D + d];
  }
  red[rg][lane] = acc;
  __syncthreads();
  if (rg == 0 && d < D) dW[(long)c * D + d] += (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(kThreads) void head_dbias_kernel(const float* __restrict__ dlogits, int B, int C, float* __restrict__ dbias) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  dbias[c] += strided_sum<4>(dlogits + c, C, 0, 1, B);
}

// ------------------------------------------------------------------------------------------------ LARS
struct LarsBatch {
  float* p[kLarsBatch];
  const float* g[kLarsBatch];
  float* mu[kLarsBatch];
  long n[kLarsBatch];
  int is_matrix[kLarsBatch];
};

// workgroup (r, s): row r of segment s holds [sum p^2, sum (g + wd p)^2] over the elements r kThreads + t + k kLarsRows kThreads
__global__ __launch_bounds__(kThreads) void lars_norms_kernel(const LarsBatch b, const float* __restrict__ hyper, double* __restrict__ rows) {
  __shared__ double red[2][kWaves];
  const int s = blockIdx.y, r = blockIdx.x;
  if (!b.is_matrix[s]) return;  // (uniform over the workgroup)
  const float wd = hyper[1];
  const float* __restrict__ p = b.p[s];
  const float* __restrict__ g = b.g[s];
  double pp = 0.0, uu = 0.0;
  for (long i = (long)r * kThreads + threadIdx.x; i < b.n[s]; i += (long)kLarsRows * kThreads) {
    const float pv = p[i];
    const float dp = g[i] + wd * pv;
    pp += (double)pv * (double)pv;
    uu += (double)dp * (double)dp;
  }
  pp = wave_sum_f64(pp);
  uu = wave_sum_f64(uu);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = pp;
    red[1][wave] = uu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* row = rows + ((long)s * kLarsRows + r) * 2;
    row[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    row[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

__global__ __launch_bounds__(kThreads) void lars_update_kernel(const LarsBatch b, const float* __restrict__ hyper,
                                                               const double* __restrict__ rows) {
  __shared__ float s_q;
  const int s = blockIdx.y;
  const float lr = hyper[0], wd = hyper[1], mom = hyper[2], tc = hyper[3];
  const bool matrix = b.is_matrix[s] != 0;
  if (threadIdx.x == 0) {
    float q = 1.0f;
    if (matrix) {
      double pp = 0.0, uu = 0.0;
      for (int r = 0; r < kLarsRows; ++r) {
        pp += rows[((long)s * kLarsRows + r) * 2];
        uu += rows[((long)s * kLarsRows + r) * 2 + 1];
      }
      // torch.where(param_norm > 0, torch.where(update_norm > 0, tc param_norm / update_norm, 1), 1)
      if (pp > 0.0 && uu > 0.0) q = (float)((double)tc * sqrt(pp) / sqrt(uu));
    }
    s_q = q;
  }
  __syncthreads();
  const float q = s_q;
  float* __restrict__ p = b.p[s];
  const float* __restrict__ g = b.g[s];
  float* __restrict__ mu = b.mu[s];
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < b.n[s]; i += (long)gridDim.x * kThreads) {
    const float pv = p[i];
    float dp = g[i];
    if (matrix) dp = (dp + wd * pv) * q;
    const float m = mom * mu[i] + dp;
    mu[i] = m;
    p[i] = pv - lr * m;
  }
}

}  // namespace

extern "C" int pm_pool_norm_workspace(int B, int N, int D, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (B <= 0 || N < 2 || D <= 0 || (D & 3) || D > kMaxD || (long)B * pool_splits(N) > (1L << 30)) return PM_ESHAPE;
  *bytes = pool_workspace_bytes(B, N, D);
  return PM_OK;
}

extern "C" int pm_pool_norm_fwd(const float* x, int B, int N, int D, const float* gamma, const float* beta, float eps, float* feat,
                                void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !gamma || !beta || !feat || !workspace) return PM_EINVAL;
  size_t need = 0;
  const int st = pm_pool_norm_workspace(B, N, D, &need);
  if (st != PM_OK) return st;
  if (!(eps >= 0.f)) return PM_EINVAL;
  if (ws_bytes < need) return PM_EINVAL;
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)feat | (uintptr_t)workspace) & 15) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  const int S = pool_splits(N);
  hipLaunchKernelGGL(pool_partial_kernel, dim3(B * S), dim3(kPoolThreads), 0, q, x, N, D, S, (float*)workspace);
  hipLaunchKernelGGL(pool_norm_kernel<false>, dim3(B), dim3(kPoolThreads), 0, q, (const float*)workspace, N, D, S, gamma, beta, eps, feat,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr);
  return pm_check_launch();
}

extern "C" int pm_probe_head_fwd(const float* feat, int B, int D, int C, const float* W, const float* bias, float* running_mean,
                                 float* running_var, long long* num_batches_tracked, int training, float momentum, float eps,
                                 float* xhat, float* logits, void* stream) {
  if (!feat || !W || !bias || !running_mean || !running_var || !xhat || !logits) return PM_EINVAL;
  if (training && !num_batches_tracked) return PM_EINVAL;
  if (B <= 0 || B > 65535 || D <= 0 || (D & 3) || C <= 0 || C > (1 << 20)) return PM_ESHAPE;
  if (training && B < 2) return PM_ESHAPE;  // torch: "Expected more than 1 value per channel when training"
  if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return PM_EINVAL;
  if (((uintptr_t)W | (uintptr_t)xhat) & 15) return PM_EALIGN;
  if (((uintptr_t)feat | (uintptr_t)bias | (uintptr_t)running_mean | (uintptr_t)running_var | (uintptr_t)logits) & 3) return PM_EALIGN;
  if ((uintptr_t)num_batches_tracked & 7) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  hipLaunchKernelGGL(bn_kernel, dim3((D + 63) / 64), dim3(1024), 0, q, feat, B, D, running_mean, running_var, num_batches_tracked,
                     training ? 1 : 0, momentum, eps, xhat);
  hipLaunchKernelGGL(linear_kernel, dim3((C + 63) / 64, B), dim3(kPoolThreads), 0, q, (const float*)xhat, W, bias, D, C, logits);
  return pm_check_launch();
}

extern "C" int pm_probe_ce_workspace(int B, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (B <= 0 || B > (1 << 24)) return PM_ESHAPE;
  *bytes = (size_t)B * (sizeof(float) + sizeof(int));
  return PM_OK;
}

extern "C" int pm_probe_ce(const float* logits, const long long* target, int B, int C, const float* scale, float* loss, float* dlogits,
                           long long* correct, void* workspace, size_t ws_bytes, void* stream) {
  if (!logits || !target || !loss || !correct || !workspace) return PM_EINVAL;
  if (dlogits && !scale) return PM_EINVAL;
  size_t need = 0;
  const int st = pm_probe_ce_workspace(B, &need);
  if (st != PM_OK) return st;
  if (C <= 0 || C > (1 << 20)) return PM_ESHAPE;
  if (ws_bytes < need) return PM_EINVAL;
  if (((uintptr_t)logits | (uintptr_t)scale | (uintptr_t)loss | (uintptr_t)dlogits | (uintptr_t)workspace) & 3) return PM_EALIGN;
  if (((uintptr_t)target | (uintptr_t)correct) & 7) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  float* row_loss = (float*)workspace;
  int* row_hits = (int*)(row_loss + B);
  hipLaunchKernelGGL(ce_rows_kernel, dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, q, logits, target, B, C, C < 5 ? C : 5, scale,
                     dlogits, row_loss, row_hits);
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(kThreads), 0, q, (const float*)row_loss, (const int*)row_hits, B, loss, correct);
  return pm_check_launch();
}

extern "C" int pm_probe_head_bwd(const float* dlogits, const float* xhat, int B, int D, int C, float* dW, float* dbias, void* stream) {
  if (!dlogits || !xhat || !dW || !dbias) return PM_EINVAL;
  if (B <= 0 || D <= 0 || C <= 0 || C > 65535) return PM_ESHAPE;
  if (((uintptr_t)dlogits | (uintptr_t)xhat | (uintptr_t)dW | (uintptr_t)dbias) & 3) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  hipLaunchKernelGGL(head_dw_kernel, dim3((D + 63) / 64, C), dim3(kThreads), 0, q, dlogits, xhat, B, D, C, dW);
  hipLaunchKernelGGL(head_dbias_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, q, dlogits, B, C, dbias);
  return pm_check_launch();
}

extern "C" int pm_lars_workspace(int n_segs, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (n_segs <= 0 || n_segs > (1 << 16)) return PM_ESHAPE;
  *bytes = (size_t)n_segs * kLarsRows * 2 * sizeof(double);
  return PM_OK;
}

// Everything is checked before the first enqueue, so a refusal leaves the stream untouched.
extern "C" int pm_lars_step(const pm_lars_segment* segs, int n_segs, const float* hyper, void* workspace, size_t ws_bytes, void* stream) {
  if (!segs || !hyper || !workspace) return PM_EINVAL;
  size_t need = 0;
  const int st = pm_lars_workspace(n_segs, &need);
  if (st != PM_OK) return st;
  if (ws_bytes < need) return PM_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)hyper & 3)) return PM_EALIGN;
  for (int i = 0; i < n_segs; ++i) {
    if (!segs[i].p || !segs[i].g || !segs[i].mu) return PM_EINVAL;
    if (segs[i].n <= 0 || segs[i].n > (1L << 40)) return PM_ESHAPE;
    if (((uintptr_t)segs[i].p | (uintptr_t)segs[i].g | (uintptr_t)segs[i].mu) & 3) return PM_EALIGN;
  }
  hipStream_t q = pm_stream(stream);
  double* rows = (double*)workspace;
  for (int first = 0; first < n_segs; first += kLarsBatch) {
    LarsBatch b;
    const int live = n_segs - first < kLarsBatch ? n_segs - first : kLarsBatch;
    long longest = 1;
    bool any_matrix = false;
    for (int i = 0; i < kLarsBatch; ++i) {
      const bool on = i < live;
      b.p[i] = on ? segs[first + i].p : nullptr;
      b.g[i] = on ? segs[first + i].g : nullptr;
      b.mu[i] = on ? segs[first + i].mu : nullptr;
      b.n[i] = on ? segs[first + i].n : 0;
      b.is_matrix[i] = on && segs[first + i].is_matrix ? 1 : 0;
      if (on && b.n[i] > longest) longest = b.n[i];
      any_matrix = any_matrix || b.is_matrix[i];
    }
    double* batch_rows = rows + (long)first * kLarsRows * 2;
    if (any_matrix) {
      hipLaunchKernelGGL(lars_norms_kernel, dim3(kLarsRows, live), dim3(kThreads), 0, q, b, hyper, batch_rows);
    }
    hipLaunchKernelGGL(lars_update_kernel, dim3(cap_grid(longest, kThreads * 4, kLarsMaxBlocks), live), dim3(kThreads), 0, q, b, hyper,
                       (const double*)batch_rows);
  }
  return pm_check_launch();
}
