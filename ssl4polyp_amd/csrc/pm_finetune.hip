// pm_finetune.hip -- the ring of f32 kernels the MAE end-to-end fine-tune recipe (mae/main_finetune.py + engine_finetune.py) puts
// around the block stack (include/polypmae.h: pm_mix_batch, pm_soft_ce, pm_pool_norm_fwd_train, pm_pool_norm_bwd, pm_linear_head_fwd,
// pm_linear_head_dfeat).
//
// The reference mixes every training batch with timm's Mixup (mode "batch": Mixup or CutMix of sample b with sample B - 1 - b),
// scores it with SoftTargetCrossEntropy over the mixed, smoothed one-hot targets, and trains the whole ViT of models_vit.py: with
// global_pool the mean of the patch rows through fc_norm, then one plain Linear.  Conventions as in pm_probe.hip: f32 throughout,
// fixed summation order (no float atomics), the stream passed in, nothing allocated, every refusal before the first launch.
//
//   mix_kernel                    one thread owns the same 4 elements of BOTH members of a pair, so the in-place update has no hazard.
//                                 lam / 1 - lam / the box come from a device record (a captured step follows new draws).  Mixup:
//                                 fl(fl(lam a) + fl((1 - lam) b)) -- two products and one sum, never an FMA (v_mul_f32 / v_add_f32 by
//                                 name: hipcc contracts every other spelling, __fmul_rn included) = torch's three-op sequence bit
//                                 for bit.  CutMix: the pair swaps its old values inside the box; nothing is loaded or written
//                                 outside it.  Vectors are aligned to the flat sample, not to the box: xl may be anything.
//   soft_ce_rows / soft_ce_finish one wave per sample: log-sum-exp, loss_b = sum_c t_c (lse - z_c) with the target row
//                                 t = lam onehot(y_b) + (1 - lam) onehot(y_partner) built on the fly (the two weights ADD when the
//                                 classes coincide), dlogits = (softmax - t) s / B; then one workgroup adds up the rows.
//   pool_partial / pool_norm<true>, linear_kernel   pm_pool_head.h, shared with pm_probe.hip: the two-stage pool + fc_norm that also
//                                 leaves the pooled row and mean / rstd for the backward, and logits = feat W^T + bias.
//   pool_bwd_row / _fill / _pgrad LayerNorm backward on the pooled row, / (N - 1), into a [B, D] row; ONE coalesced pass writes
//                                 that row to every patch row of dx (f32) and dx_act (16-byte stores), zeros to the cls row;
//                                 dgamma / dbeta: one thread per column, samples in ascending order, one addition into the prior.
//   dfeat_kernel                  dfeat = dlogits W: 8 samples x 4 columns per thread, classes in ascending order; W is read once
//                                 per 8 samples.
#include <math.h>

#include "pm_pool_head.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PM_WAVE;
constexpr int kMaxBlocks = 2048;
constexpr int kDfeatRows = 8;
constexpr int kDfeatDepth = 16;
constexpr int kPgradDepth = 16;

// one rounding each: an instruction the compiler cannot fuse with its neighbour
__device__ __forceinline__ float mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float add_rn(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// ------------------------------------------------------------------------------------------------ Mixup / CutMix in place
// V consecutive elements of the flat sample [C, H, W] per thread (V = 4: 16-byte accesses, E % 4 == 0; V = 1 otherwise).
// blockIdx.y: the pair (b, B - 1 - b).
template <int V>
__global__ __launch_bounds__(kThreads) void mix_kernel(float* __restrict__ x, int B, long E, int H, int W,
                                                       const pm_mix_record* __restrict__ rec) {
  const float lam = rec->lam, oml = rec->one_minus_lam;
  const int cut = rec->use_cutmix;
  if (!cut && lam == 1.0f && oml == 0.0f) return;  // the identity draw writes nothing
  const int b = blockIdx.y;
  float* __restrict__ xa = x + (long)b * E;
  float* __restrict__ xb = x + (long)(B - 1 - b) * E;
  const long step = (long)gridDim.x * kThreads * V;
  if (!cut) {
    for (long e = ((long)blockIdx.x * kThreads + threadIdx.x) * V; e < E; e += step) {
      if constexpr (V == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xa + e), p = *reinterpret_cast<const f32x4*>(xb + e);
        f32x4 na, np;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          na[k] = add_rn(mul_rn(a[k], lam), mul_rn(p[k], oml));
          np[k] = add_rn(mul_rn(p[k], lam), mul_rn(a[k], oml));
        }
        *reinterpret_cast<f32x4*>(xa + e) = na;
        *reinterpret_cast<f32x4*>(xb + e) = np;
      } else {
        const float a = xa[e], p = xb[e];
        xa[e] = add_rn(mul_rn(a, lam), mul_rn(p, oml));
        xb[e] = add_rn(mul_rn(p, lam), mul_rn(a, oml));
      }
    }
    return;
  }
  // the box, clipped to the image whatever the record holds
  const int yl = max(rec->yl, 0), yh = min(rec->yh, H), xl = max(rec->xl, 0), xh = min(rec->xh, W);
  if (yl >= yh || xl >= xh) return;
  const unsigned HW = (unsigned)H * (unsigned)W;
  for (long e = ((long)blockIdx.x * kThreads + threadIdx.x) * V; e < E; e += step) {   // (E < 2^31: checked on the host)
    const int rem = (int)((unsigned)e % HW);
    int y = rem / W, xx = rem - y * W;
    bool in[V];
    int n_in = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      in[k] = y >= yl && y < yh && xx >= xl && xx < xh;
      n_in += in[k] ? 1 : 0;
      if (++xx == W) {
        xx = 0;
        if (++y == H) y = 0;   // (the next channel's first row)
      }
    }
    if (n_in == 0) continue;
    if constexpr (V == 4) {
      if (n_in == 4) {  // both old values are in registers before either store
        const f32x4 a = *reinterpret_cast<const f32x4*>(xa + e), p = *reinterpret_cast<const f32x4*>(xb + e);
        *reinterpret_cast<f32x4*>(xa + e) = p;
        *reinterpret_cast<f32x4*>(xb + e) = a;
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (in[k]) {
        const float a = xa[e + k], p = xb[e + k];
        xa[e + k] = p;
        xb[e + k] = a;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ soft-target cross-entropy
// one wave per row; the row's target is lam onehot(y_row; on, off) + (1 - lam) onehot(y_{B-1-row}; on, off).  A target outside
// [0, C) (of the row or of its partner) poisons the loss with NaN and gives the row a zero gradient.
__global__ __launch_bounds__(kThreads) void soft_ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                                int B, int C, const pm_mix_record* __restrict__ rec, float on, float off,
                                                                const float* __restrict__ scale, float* __restrict__ dlogits,
                                                                float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kWaves + wave;
  if (row >= B) return;  // (wave-uniform; no barrier below)
  const float lam = rec ? rec->lam : 1.0f, oml = rec ? rec->one_minus_lam : 0.0f;
  const float* z = logits + (long)row * C;
  const long long ta = target[row], tb = target[B - 1 - row];
  const bool valid = ta >= 0 && ta < (long long)C && tb >= 0 && tb < (long long)C;
  const int ya = valid ? (int)ta : -1, yb = valid ? (int)tb : -1;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
  m = wave_max(m);
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(z[c] - m);
  se = wave_sum(se);
  const float lse = m + logf(se);
  const float rse = 1.0f / se;
  const float g = (dlogits && scale) ? scale[0] / (float)B : 0.f;
  float acc = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float t = lam * (c == ya ? on : off) + oml * (c == yb ? on : off);
    acc += t * (lse - z[c]);
    if (dlogits) {
      const float p = expf(z[c] - m) * rse;
      dlogits[(long)row * C + c] = valid ? (p - t) * g : 0.f;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) row_loss[row] = valid ? acc : NAN;
}

__global__ __launch_bounds__(kThreads) void soft_ce_finish_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ loss) {
  __shared__ float red[kWaves];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += kThreads) s += row_loss[b];
  const float total = block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = total / (float)B;
}

// ------------------------------------------------------------------------------------------------ pool + fc_norm, backward
// workgroup b: row[b][d] = rstd (gg_d - c1 - xhat_d c2) / (N - 1), gg = dfeat gamma, c1 = mean_d gg, c2 = mean_d gg xhat
__global__ __launch_bounds__(kThreads) void pool_bwd_row_kernel(const float* __restrict__ dfeat, const float* __restrict__ pooled,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, int N, int D, float* __restrict__ row) {
  __shared__ float red[kWaves];
  const int b = blockIdx.x;
  const float mu = mean[b], rs = rstd[b];
  f32x4 gg[2], xh[2];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (threadIdx.x + j * kThreads) * 4;
    gg[j] = xh[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < D) {
      const f32x4 df = *reinterpret_cast<const f32x4*>(dfeat + (long)b * D + c), g = *reinterpret_cast<const f32x4*>(gamma + c);
      const f32x4 p = *reinterpret_cast<const f32x4*>(pooled + (long)b * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gg[j][e] = df[e] * g[e];
        xh[j][e] = (p[e] - mu) * rs;
        s1 += gg[j][e];
        s2 += gg[j][e] * xh[j][e];
      }
    }
  }
  const float c1 = block_sum(s1, red) / (float)D;
  const float c2 = block_sum(s2, red) / (float)D;
  const float den = (float)(N - 1);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (threadIdx.x + j * kThreads) * 4;
    if (c < D) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = rs * (gg[j][e] - c1 - xh[j][e] * c2) / den;
      *reinterpret_cast<f32x4*>(row + (long)b * D + c) = o;
    }
  }
}

// blockIdx.y: the sample; the sample's N D elements as one flat array, V per thread: row 0 zeros, every other row a copy of row[b]
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void pool_bwd_fill_kernel(const float* __restrict__ row, int N, int D, float* __restrict__ dx,
                                                                 T* __restrict__ dx_act) {
  const int b = blockIdx.y;
  const unsigned total = (unsigned)N * (unsigned)D;
  const float* __restrict__ r = row + (long)b * D;
  float* __restrict__ out = dx + (long)b * total;
  T* __restrict__ out_act = dx_act ? dx_act + (long)b * total : nullptr;
  const unsigned step = gridDim.x * kThreads * V;
  for (unsigned i = (blockIdx.x * kThreads + threadIdx.x) * V; i < total; i += step) {
    const unsigned col = i % (unsigned)D;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (i >= (unsigned)D) {
      lo = *reinterpret_cast<const f32x4*>(r + col);
      if constexpr (V == 8) hi = *reinterpret_cast<const f32x4*>(r + col + 4);
    }
    *reinterpret_cast<f32x4*>(out + i) = lo;
    if constexpr (V == 8) {
      *reinterpret_cast<f32x4*>(out + i + 4) = hi;
      if (out_act) store8_16<T>(out_act + i, lo, hi);
    } else {
      if (out_act) store4<T>(out_act + i, lo);
    }
  }
}

// one thread per column, the samples in ascending order, kPgradDepth loads in flight; ONE addition into what dgamma / dbeta held
__global__ __launch_bounds__(64) void pool_bwd_pgrad_kernel(const float* __restrict__ dfeat, const float* __restrict__ pooled,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd, int B, int D,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  float sg = 0.f, sb = 0.f;
  int b = 0;
  for (; b + kPgradDepth - 1 < B; b += kPgradDepth) {
    float df[kPgradDepth], p[kPgradDepth], mu[kPgradDepth], rs[kPgradDepth];
#pragma unroll
    for (int u = 0; u < kPgradDepth; ++u) {
      df[u] = dfeat[(long)(b + u) * D + d];
      p[u] = pooled[(long)(b + u) * D + d];
      mu[u] = mean[b + u];
      rs[u] = rstd[b + u];
    }
#pragma unroll
    for (int u = 0; u < kPgradDepth; ++u) {
      sg += df[u] * ((p[u] - mu[u]) * rs[u]);
      sb += df[u];
    }
  }
  for (; b < B; ++b) {
    const float df = dfeat[(long)b * D + d];
    sg += df * ((pooled[(long)b * D + d] - mean[b]) * rstd[b]);
    sb += df;
  }
  if (dgamma) dgamma[d] += sg;
  if (dbeta) dbeta[d] += sb;
}

// ------------------------------------------------------------------------------------------------ the plain Linear head, backward
// dfeat[b][d] = sum_c dlogits[b][c] W[c][d], c ascending.  Workgroup (64 vectors of 4 columns, kDfeatRows samples): one 16-byte load
// of W per class serves kDfeatRows samples; the dlogits of a class are uniform over the workgroup.
__global__ __launch_bounds__(64) void dfeat_kernel(const float* __restrict__ dlogits, const float* __restrict__ W, int B, int D, int C,
                                                   float* __restrict__ dfeat) {
  const int d = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int b0 = blockIdx.y * kDfeatRows;
  if (d >= D) return;
  const float* dl[kDfeatRows];
#pragma unroll
  for (int r = 0; r < kDfeatRows; ++r) dl[r] = dlogits + (long)min(b0 + r, B - 1) * C;
  f32x4 acc[kDfeatRows];
#pragma unroll
  for (int r = 0; r < kDfeatRows; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  int c = 0;
  for (; c + kDfeatDepth - 1 < C; c += kDfeatDepth) {  // kDfeatDepth rows of W in flight (L2 latency, not bandwidth, bounds this loop)
    f32x4 w[kDfeatDepth];
#pragma unroll
    for (int u = 0; u < kDfeatDepth; ++u) w[u] = *reinterpret_cast<const f32x4*>(W + (long)(c + u) * D + d);
#pragma unroll
    for (int u = 0; u < kDfeatDepth; ++u) {
#pragma unroll
      for (int r = 0; r < kDfeatRows; ++r) acc[r] += w[u] * dl[r][c + u];
    }
  }
  for (; c < C; ++c) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(W + (long)c * D + d);
#pragma unroll
    for (int r = 0; r < kDfeatRows; ++r) acc[r] += w * dl[r][c];
  }
#pragma unroll
  for (int r = 0; r < kDfeatRows; ++r) {
    if (b0 + r < B) *reinterpret_cast<f32x4*>(dfeat + (long)(b0 + r) * D + d) = acc[r];
  }
}

int pool_shape_ok(int B, int N, int D) {
  return !(B <= 0 || B > 65535 || N < 2 || D <= 0 || (D & 3) || D > kMaxD || (long)B * pool_splits(N) > (1L << 30) ||
           (long)N * D > (1L << 30));
}

}  // namespace

extern "C" int pm_mix_batch(float* x, int B, int C, int H, int W, const pm_mix_record* rec, int enabled, void* stream) {
  if (!x || !rec) return PM_EINVAL;
  if (B <= 0 || (B & 1) || B > 2 * 65535 || C <= 0 || H <= 0 || W <= 0) return PM_ESHAPE;  // timm asserts an even batch
  const long E = (long)C * H * W;
  if ((long)H * W > (1L << 30) || E >= (1L << 31)) return PM_ESHAPE;
  if (((uintptr_t)x & 15) || ((uintptr_t)rec & 3)) return PM_EALIGN;
  if (!enabled) return PM_OK;  // the host drew lam == 1 without a box: nothing to launch
  hipStream_t q = pm_stream(stream);
  const int pairs = B / 2;
  if ((E & 3) == 0) {
    const int gx = cap_grid(E / 4, kThreads, (kMaxBlocks + pairs - 1) / pairs);
    hipLaunchKernelGGL(mix_kernel<4>, dim3(gx, pairs), dim3(kThreads), 0, q, x, B, E, H, W, rec);
  } else {
    const int gx = cap_grid(E, kThreads, (kMaxBlocks + pairs - 1) / pairs);
    hipLaunchKernelGGL(mix_kernel<1>, dim3(gx, pairs), dim3(kThreads), 0, q, x, B, E, H, W, rec);
  }
  return pm_check_launch();
}

extern "C" int pm_soft_ce_workspace(int B, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (B <= 0 || B > 65535) return PM_ESHAPE;
  *bytes = (size_t)B * sizeof(float);
  return PM_OK;
}

extern "C" int pm_soft_ce(const float* logits, const long long* target, int B, int C, const pm_mix_record* rec, float smoothing,
                          const float* scale, float* loss, float* dlogits, void* workspace, size_t ws_bytes, void* stream) {
  if (!logits || !target || !loss || !workspace) return PM_EINVAL;
  if (dlogits && !scale) return PM_EINVAL;
  size_t need = 0;
  const int st = pm_soft_ce_workspace(B, &need);
  if (st != PM_OK) return st;
  if (C <= 0 || C > (1 << 20)) return PM_ESHAPE;
  if (!(smoothing >= 0.f && smoothing <= 1.f)) return PM_EINVAL;
  if (ws_bytes < need) return PM_EINVAL;
  if (((uintptr_t)logits | (uintptr_t)rec | (uintptr_t)scale | (uintptr_t)loss | (uintptr_t)dlogits | (uintptr_t)workspace) & 3)
    return PM_EALIGN;
  if ((uintptr_t)target & 7) return PM_EALIGN;
  // timm's one_hot: off = smoothing / C, on = 1 - smoothing + off, in double, stored in f32 tensors
  const double off = (double)smoothing / (double)C;
  const double on = 1.0 - (double)smoothing + off;
  hipStream_t q = pm_stream(stream);
  float* row_loss = (float*)workspace;
  hipLaunchKernelGGL(soft_ce_rows_kernel, dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, q, logits, target, B, C, rec, (float)on,
                     (float)off, scale, dlogits, row_loss);
  hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(kThreads), 0, q, (const float*)row_loss, B, loss);
  return pm_check_launch();
}

extern "C" int pm_pool_norm_fwd_train(const float* x, int B, int N, int D, const float* gamma, const float* beta, float eps, float* feat,
                                      float* pooled, float* mean, float* rstd, void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !gamma || !beta || !feat || !pooled || !mean || !rstd || !workspace) return PM_EINVAL;
  if (!pool_shape_ok(B, N, D)) return PM_ESHAPE;
  if (!(eps >= 0.f)) return PM_EINVAL;
  if (ws_bytes < pool_workspace_bytes(B, N, D)) return PM_EINVAL;   // (= pm_pool_norm_workspace)
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)feat | (uintptr_t)pooled | (uintptr_t)workspace) & 15)
    return PM_EALIGN;
  if (((uintptr_t)mean | (uintptr_t)rstd) & 3) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  const int S = pool_splits(N);
  hipLaunchKernelGGL(pool_partial_kernel, dim3(B * S), dim3(kPoolThreads), 0, q, x, N, D, S, (float*)workspace);
  hipLaunchKernelGGL(pool_norm_kernel<true>, dim3(B), dim3(kPoolThreads), 0, q, (const float*)workspace, N, D, S, gamma, beta, eps, feat,
                     pooled, mean, rstd);
  return pm_check_launch();
}

extern "C" int pm_pool_norm_bwd_workspace(int B, int N, int D, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (!pool_shape_ok(B, N, D)) return PM_ESHAPE;
  *bytes = (size_t)B * D * sizeof(float);
  return PM_OK;
}

extern "C" int pm_pool_norm_bwd(const float* dfeat, const float* pooled, const float* mean, const float* rstd, const float* gamma, int B,
                                int N, int D, float* dx, void* dx_act, int act_dtype, float* dgamma, float* dbeta, void* workspace,
                                size_t ws_bytes, void* stream) {
  if (!dfeat || !pooled || !mean || !rstd || !gamma || !workspace) return PM_EINVAL;
  if (!dx && dx_act) return PM_EINVAL;
  size_t need = 0;
  const int st = pm_pool_norm_bwd_workspace(B, N, D, &need);
  if (st != PM_OK) return st;
  if (ws_bytes < need) return PM_EINVAL;
  if (act_dtype != PM_BF16 && act_dtype != PM_F16 && act_dtype != PM_F32) return PM_EINVAL;
  if (((uintptr_t)dfeat | (uintptr_t)pooled | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)dx_act | (uintptr_t)workspace) & 15)
    return PM_EALIGN;
  if (((uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)dgamma | (uintptr_t)dbeta) & 3) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  float* row = (float*)workspace;
  if (dx) {  // NULL: nothing below fc_norm trains
    hipLaunchKernelGGL(pool_bwd_row_kernel, dim3(B), dim3(kThreads), 0, q, dfeat, pooled, mean, rstd, gamma, N, D, row);
    const long total = (long)N * D;
    const int cap = (kMaxBlocks + B - 1) / B;
#define PM_POOL_FILL(T, V)                                                                                              \
  hipLaunchKernelGGL((pool_bwd_fill_kernel<T, V>), dim3(cap_grid(total / V, kThreads, cap), B), dim3(kThreads), 0, q, \
                     (const float*)row, N, D, dx, (T*)dx_act)
    if (act_dtype == PM_F32) PM_POOL_FILL(float, 4);
    else if (act_dtype == PM_BF16) { if (D & 7) PM_POOL_FILL(__bf16, 4); else PM_POOL_FILL(__bf16, 8); }
    else { if (D & 7) PM_POOL_FILL(_Float16, 4); else PM_POOL_FILL(_Float16, 8); }
#undef PM_POOL_FILL
  }
  if (dgamma || dbeta)
    hipLaunchKernelGGL(pool_bwd_pgrad_kernel, dim3((D + 63) / 64), dim3(64), 0, q, dfeat, pooled, mean, rstd, B, D, dgamma, dbeta);
  return pm_check_launch();
}

extern "C" int pm_linear_head_fwd(const float* feat, int B, int D, int C, const float* W, const float* bias, float* logits, void* stream) {
  if (!feat || !W || !bias || !logits) return PM_EINVAL;
  if (B <= 0 || B > 65535 || D <= 0 || (D & 3) || C <= 0 || C > 65535) return PM_ESHAPE;
  if (((uintptr_t)feat | (uintptr_t)W) & 15) return PM_EALIGN;
  if (((uintptr_t)bias | (uintptr_t)logits) & 3) return PM_EALIGN;
  hipLaunchKernelGGL(linear_kernel, dim3((C + 63) / 64, B), dim3(kPoolThreads), 0, pm_stream(stream), feat, W, bias, D, C, logits);
  return pm_check_launch();
}

extern "C" int pm_linear_head_dfeat(const float* dlogits, const float* W, int B, int D, int C, float* dfeat, void* stream) {
  if (!dlogits || !W || !dfeat) return PM_EINVAL;
  if (B <= 0 || B > 65535 || D <= 0 || (D & 3) || C <= 0 || C > 65535) return PM_ESHAPE;
  if (((uintptr_t)W | (uintptr_t)dfeat) & 15) return PM_EALIGN;
  if ((uintptr_t)dlogits & 3) return PM_EALIGN;
  hipLaunchKernelGGL(dfeat_kernel, dim3((D / 4 + 63) / 64, (B + kDfeatRows - 1) / kDfeatRows), dim3(64), 0, pm_stream(stream), dlogits, W,
                     B, D, C, dfeat);
  return pm_check_launch();
}
