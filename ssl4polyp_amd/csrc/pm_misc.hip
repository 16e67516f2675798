// pm_misc.hip -- the HBM-bound kernels around the GEMMs: patch im2col (+ kept-patch gather), token
// assembly (cls / pos-embed), bias-gradient column sums, casts, fused AdamW (the classifier head: pm_head.hip).
// Reference ops replaced are named per kernel.  All are streaming kernels: 16-B vector accesses,
// one wave64 per token row where a row is the unit, grid capped and grid-strided.
#include "pm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// column sums: out[n] += sum_m x[m][n]   (bias gradients)
// ---------------------------------------------------------------------------------------------
// first stage (pm_common.h block_colsum_tail): wave w of row split blockIdx.y takes rows 4 blockIdx.y + w, + 4 gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, long ldx, float* __restrict__ out,
                                                     float* __restrict__ partials, int M, int N) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 256 + lane * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (n < N) {
    for (long m = (long)blockIdx.y * 4 + wave; m < M; m += (long)gridDim.y * 4) acc += load4<T>(x + m * ldx + n);
  }
  block_colsum_tail(acc, out, partials, N);
}

// ---------------------------------------------------------------------------------------------
// im2col of the k = s = p patch-embedding conv, optionally gathering only kept patches
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ imgs, const int* __restrict__ ids_keep,
                                                     T* __restrict__ cols, long ldcols, int C, int img, int p, int keep) {
  const int b = blockIdx.x / keep, j = blockIdx.x % keep;
  const int grid = img / p;
  const int pid = ids_keep ? ids_keep[b * keep + j] : j;
  const int gy = pid / grid, gx = pid % grid;
  const float* src = imgs + (long)b * C * img * img + (long)gy * p * img + gx * p;
  T* dst = cols + (long)blockIdx.x * ldcols;
  const int PE = C * p * p;
  if ((p & 3) == 0) {  // 16-B reads of a patch row (p = 16: 64 B per row)
    const int p4 = p >> 2;
    const int nvec = C * p * p4;
    for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
      const int c = v / (p * p4), rem = v % (p * p4);
      const int py = rem / p4, px = (rem % p4) * 4;
      const f32x4 val = *reinterpret_cast<const f32x4*>(src + (long)c * img * img + (long)py * img + px);
      store4<T>(dst + (c * p + py) * p + px, val);
    }
  } else {             // p = 14 (ViT-H/14): a patch row starts on an 8-B boundary only; element-wise
    for (int e = threadIdx.x; e < PE; e += blockDim.x) {
      const int c = e / (p * p), rem = e % (p * p);
      const int py = rem / p, px = rem % p;
      dst[e] = from_f32<T>(src[(long)c * img * img + (long)py * img + px]);
    }
  }
  for (int e = PE + threadIdx.x; e < ldcols; e += blockDim.x) dst[e] = from_f32<T>(0.f);  // row padding (K of the GEMM)
}

// dst[r][c] = r < rows && c < cols ? src[r][c] : 0 over rows_pad x cols_pad, f32 -> act: a weight whose reduction dimension is not
// a multiple of the GEMM's k-step (588 = 3 x 14 x 14) laid out as the zero-padded operand the matrix-core kernels take
template <typename T>
__global__ __launch_bounds__(256) void pad_cast_kernel(const float* __restrict__ src, long lds, T* __restrict__ dst, long ldd, int rows,
                                                       int cols, int rows_pad, int cols_pad) {
  const long total = (long)rows_pad * cols_pad;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = i / cols_pad, c = i % cols_pad;
    const float v = (r < rows && c < cols) ? src[(long)r * lds + c] : 0.f;
    dst[(long)r * ldd + c] = from_f32<T>(v);
  }
}

// dst[r][c] (+)= src[r][c] over rows x cols: the valid part of a gradient computed in the padded layout
__global__ __launch_bounds__(256) void unpad_add_kernel(const float* __restrict__ src, long lds, float* __restrict__ dst, long ldd,
                                                        int rows, int cols, int accumulate) {
  const long total = (long)rows * cols;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = i / cols, c = i % cols;
    const float v = src[(long)r * lds + c];
    float* d = dst + (long)r * ldd + c;
    *d = accumulate ? *d + v : v;
  }
}

// ---------------------------------------------------------------------------------------------
// token assembly (cls + pos-embed) and its backward
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ emb, const float* __restrict__ cls,
                                                       const float* __restrict__ pos, const int* __restrict__ ids_keep,
                                                       float* __restrict__ x, int B, int keep, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (long)B * (keep + 1);
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const int b = row / (keep + 1), t = row % (keep + 1);
    const float* src;
    const float* pp;
    if (t == 0) {
      src = cls;
      pp = pos;
    } else {
      const int j = t - 1;
      const int pid = ids_keep ? ids_keep[b * keep + j] : j;
      src = emb + ((long)b * keep + j) * D;
      pp = pos + (long)(1 + pid) * D;
    }
    for (int c = lane * 4; c < D; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + c);
      const f32x4 q = *reinterpret_cast<const f32x4*>(pp + c);
      *reinterpret_cast<f32x4*>(x + row * D + c) = a + q;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void assemble_bwd_kernel(const float* __restrict__ dx, const int* __restrict__ ids_keep,
                                                           T* __restrict__ demb, float* __restrict__ dpos, int B, int keep,
                                                           int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (long)B * keep;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const int b = row / keep, j = row % keep;
    const float* src = dx + ((long)b * (keep + 1) + 1 + j) * D;
    const int pid = ids_keep ? ids_keep[b * keep + j] : j;
    for (int c = lane * 4; c < D; c += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
      store4<T>(demb + row * D + c, v);
      if (dpos) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dpos + (long)(1 + pid) * D + c + e, v[e]);
      }
    }
  }
}

// dcls[d] += sum_b dx[b, 0, d]   (also dpos[0] when the positional table is learnable; either pointer may be NULL, not both)
// The rows are one sample apart (600 KB): a thread that walks all B of them serially pays B dependent-latency loads at the
// very end of the backward pass, when nothing else runs (27 us at B = 64, 92 us at B = 256).  64 columns per block, the four
// waves take every fourth sample with four independent accumulators each, partials combined in wave order: fixed order,
// ~2 rounds of load latency.
__global__ __launch_bounds__(256) void cls_grad_kernel(const float* __restrict__ dx, float* __restrict__ dcls,
                                                       float* __restrict__ dpos0, int B, long sample_stride, int D) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (d < D) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int b = wave;
    for (; b + 12 < B; b += 16) {
      a0 += dx[(long)b * sample_stride + d];
      a1 += dx[(long)(b + 4) * sample_stride + d];
      a2 += dx[(long)(b + 8) * sample_stride + d];
      a3 += dx[(long)(b + 12) * sample_stride + d];
    }
    for (; b < B; b += 4) a0 += dx[(long)b * sample_stride + d];
    s = (a0 + a1) + (a2 + a3);
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && d < D) {
    const float t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    if (dcls) dcls[d] += t;
    if (dpos0) dpos0[d] += t;
  }
}

// ---------------------------------------------------------------------------------------------
// input tail: uint8 HWC frames -> normalised f32 NCHW  (torchvision ToTensor + Normalize, optional flips)
// ---------------------------------------------------------------------------------------------
// One thread = 4 consecutive output pixels of one row: 12 source bytes -> one f32x4 per channel plane.
// Arithmetic and its order are torchvision's: v = float(u8) / 255 ; (v - mean) / std, IEEE f32 division.
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const unsigned char* __restrict__ src,
                                                            const unsigned char* __restrict__ flags, float* __restrict__ dst,
                                                            int B, int H, int W, f32x4 mean, f32x4 stdv) {
  const int w4 = W >> 2;
  const long total = (long)B * H * w4;
  for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const int xq = id % w4;
    const int y = (id / w4) % H;
    const int b = id / ((long)w4 * H);
    const int f = flags ? flags[b] : 0;
    const int sy = (f & 2) ? H - 1 - y : y;
    const unsigned char* row = src + ((long)b * H + sy) * W * 3;
    float px[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = xq * 4 + i;
      const int sx = (f & 1) ? W - 1 - x : x;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = (float)row[sx * 3 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __fdiv_rn(__fdiv_rn(px[i][c], 255.0f) - mean[c], stdv[c]);
      *reinterpret_cast<f32x4*>(dst + (((long)b * 3 + c) * H + y) * W + xq * 4) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// cast
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ src, T* __restrict__ dst, long n) {
  const long nvec = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
    store4<T>(dst + 4 * i, *reinterpret_cast<const f32x4*>(src + 4 * i));
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[(nvec << 2) + threadIdx.x] = (T)src[(nvec << 2) + threadIdx.x];
}

// out = dy * gelu_erf'(pre): the backward of timm Mlp.act as a stand-alone elementwise pass (the training step gets it from the
// dfc2 GEMM's PM_EPI_DGELU epilogue; this is for callers that compose their own blocks from the registered ops)
template <typename T>
__global__ __launch_bounds__(256) void dgelu_kernel(const T* __restrict__ dy, const T* __restrict__ pre, T* __restrict__ out, long n) {
  const long nvec = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256)
    store4<T>(out + 4 * i, load4<T>(dy + 4 * i) * gelu_act_grad4<T>(load4<T>(pre + 4 * i)));
}

// ---------------------------------------------------------------------------------------------
// fused AdamW (torch.optim.AdamW update rule) + act-typed shadow refresh
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, T* __restrict__ shadow, long n, float lr,
                                                    float beta1, float beta2, float eps, float wd, float bc1, float rsqrt_bc2,
                                                    float gscale) {
  const long nvec = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    f32x4 pp = *reinterpret_cast<const f32x4*>(p + 4 * i);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
    f32x4 mm = *reinterpret_cast<const f32x4*>(m + 4 * i);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * gscale;
      pp[e] *= (1.0f - lr * wd);
      mm[e] = beta1 * mm[e] + (1.0f - beta1) * gr;
      vv[e] = beta2 * vv[e] + (1.0f - beta2) * gr * gr;
      const float denom = sqrtf(vv[e]) * rsqrt_bc2 + eps;
      pp[e] -= (lr / bc1) * (mm[e] / denom);
    }
    *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
    *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
    *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
    if (shadow) store4<T>(shadow + 4 * i, pp);
  }
}


// Device-resident hyper-parameters (hipGraph-replayable optimizer step): one 16-float record per param group
//   [0] lr [1] beta1 [2] beta2 [3] eps [4] weight_decay [5] grad_scale [6] step [7] bc1 [8] rsqrt_bc2
//   [9] skip (pm_loss_scale_update: this step's gradients hold inf / nan)  [10] 1 / loss scale (0 = no scaler: treated as 1)
constexpr int kHyperStride = 16;
__global__ void adamw_tick_kernel(float* __restrict__ hyper, int n_groups) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  float* h = hyper + (long)g * kHyperStride;
  if (h[9] != 0.f) return;  // a skipped step does not count (GradScaler.step: optimizer.step() is not called)
  const float step = h[6] + 1.0f;
  h[6] = step;
  h[7] = (float)(1.0 - pow((double)h[1], (double)step));
  h[8] = (float)(1.0 / sqrt(1.0 - pow((double)h[2], (double)step)));
}

// The same tick for the records a device-resident list names (per-parameter steps: a param group owns one record per cohort of
// parameters that share a step history, and only the cohorts with a gradient this step advance).  Same skip rule, same f64
// arithmetic: a cohort at step t holds the bits a group at step t holds.  An index outside [0, n_records) is ignored (the host
// refuses such a list before the launch; the list itself lives in device memory that later code could overwrite).
__global__ void adamw_tick_list_kernel(float* __restrict__ hyper, int n_records, const int* __restrict__ list, int n_list) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_list) return;
  const int r = list[i];
  if (r < 0 || r >= n_records) return;
  float* h = hyper + (long)r * kHyperStride;
  if (h[9] != 0.f) return;
  const float step = h[6] + 1.0f;
  h[6] = step;
  h[7] = (float)(1.0 - pow((double)h[1], (double)step));
  h[8] = (float)(1.0 / sqrt(1.0 - pow((double)h[2], (double)step)));
}

// The device-hyper-parameter update as a streaming kernel whose footprint the caller bounds (pm_adamw_grid): a workgroup walks
// chunks of kAdamwUnroll x 256 vectors, and a whole chunk is written as all of a lane's loads of p, g, m, v (64 VGPRs of payload)
// followed by the arithmetic and the stores, so that a grid of a few hundred workgroups keeps the ~10 MB in flight that HBM rate
// needs (256 workgroups run the ViT-B update as fast as 4096; 128 do not).  The compiler's own order -- the first vector's loads and
// stores, then the other thirteen loads in flight over the rest -- is left alone: fenced into sixteen loads up front the step was
// slower (docs/EXPERIMENT_LOG.md, "AdamW footprint").  There are no cross-element sums: every output is the per-element
// expression of adamw_kernel above, whatever the map.
constexpr int kAdamwUnroll = 4;
constexpr int kAdamwChunk = kAdamwUnroll * 256;  // vectors per workgroup and loop trip

struct AdamwHyper {
  float lr, beta1, beta2, eps, wd, gscale, bc1, rsqrt_bc2;
};

// p, g, m and v are touched once per step and not again before the next one: their loads and stores carry the non-temporal
// hint (the shadow, which the next forward reads, is stored normally).  Measured, not derived: the update alone runs at 5.4 instead
// of 4.8 TB/s with it, and the step beside it gains more than that difference.  The hint changes no value.
__device__ __forceinline__ f32x4 ld_stream(const float* a) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a)); }
__device__ __forceinline__ void st_stream(float* a, f32x4 x) { __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(a)); }

template <typename T>
__device__ __forceinline__ void adamw_dev_vec(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, T* __restrict__ shadow,
                                              long i, f32x4 pp, const f32x4 gg, f32x4 mm, f32x4 vv, const AdamwHyper& h) {
  const float lr = h.lr, beta1 = h.beta1, beta2 = h.beta2, eps = h.eps, wd = h.wd, gscale = h.gscale;
  const float bc1 = h.bc1, rsqrt_bc2 = h.rsqrt_bc2;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float gr = gg[e] * gscale;
    pp[e] *= (1.0f - lr * wd);
    mm[e] = beta1 * mm[e] + (1.0f - beta1) * gr;
    vv[e] = beta2 * vv[e] + (1.0f - beta2) * gr * gr;
    const float denom = sqrtf(vv[e]) * rsqrt_bc2 + eps;
    pp[e] -= (lr / bc1) * (mm[e] / denom);
  }
  st_stream(p + 4 * i, pp);
  st_stream(m + 4 * i, mm);
  st_stream(v + 4 * i, vv);
  if (shadow) store4<T>(shadow + 4 * i, pp);
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, T* __restrict__ shadow, long n,
                                                        const float* __restrict__ hyper) {
  if (hyper[9] != 0.f) return;  // non-finite gradients under loss scaling: the update is skipped, nothing is touched
  AdamwHyper h;
  h.lr = hyper[0], h.beta1 = hyper[1], h.beta2 = hyper[2], h.eps = hyper[3], h.wd = hyper[4];
  h.gscale = hyper[5] * (hyper[10] != 0.f ? hyper[10] : 1.0f);
  h.bc1 = hyper[7], h.rsqrt_bc2 = hyper[8];
  const long nvec = n >> 2;
  for (long c = (long)blockIdx.x * kAdamwChunk; c < nvec; c += (long)gridDim.x * kAdamwChunk) {
    const long i0 = c + threadIdx.x;
    if (c + kAdamwChunk <= nvec) {  // a whole chunk (uniform over the workgroup): all loads, then the arithmetic and the stores
      f32x4 pp[kAdamwUnroll], gg[kAdamwUnroll], mm[kAdamwUnroll], vv[kAdamwUnroll];
#pragma unroll
      for (int k = 0; k < kAdamwUnroll; ++k) {
        const long i = i0 + k * 256;
        pp[k] = ld_stream(p + 4 * i);
        gg[k] = ld_stream(g + 4 * i);
        mm[k] = ld_stream(m + 4 * i);
        vv[k] = ld_stream(v + 4 * i);
      }
#pragma unroll
      for (int k = 0; k < kAdamwUnroll; ++k) adamw_dev_vec<T>(p, m, v, shadow, i0 + k * 256, pp[k], gg[k], mm[k], vv[k], h);
    } else {  // the ragged last chunk of the range
      for (long i = i0; i < nvec; i += 256)
        adamw_dev_vec<T>(p, m, v, shadow, i, ld_stream(p + 4 * i), ld_stream(g + 4 * i),
                         ld_stream(m + 4 * i), ld_stream(v + 4 * i), h);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gradient statistics in one pass: out[0] += sum g^2, out[1] += #NaN, out[2] += #Inf
// (replaces the per-parameter host-synchronising loops of tc.py:1437-1454 and misc.py:387-400)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_stats_kernel(const float* __restrict__ g, long n, float* __restrict__ out) {
  __shared__ float red[3][4];
  float ss = 0.f, nn = 0.f, ni = 0.f;
  const long nvec = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ss += v[e] * v[e];
      nn += (v[e] != v[e]) ? 1.f : 0.f;
      ni += (fabsf(v[e]) == INFINITY) ? 1.f : 0.f;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = g[(nvec << 2) + threadIdx.x];
    ss += v * v;
    nn += (v != v) ? 1.f : 0.f;
    ni += (fabsf(v) == INFINITY) ? 1.f : 0.f;
  }
  ss = wave_sum(ss);
  nn = wave_sum(nn);
  ni = wave_sum(ni);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = ss;
    red[1][wave] = nn;
    red[2][wave] = ni;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    atomicAdd(out + k, (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]));
  }
}

// ---------------------------------------------------------------------------------------------
// dynamic loss scaling on the device (precision mode fp16): torch.cuda.amp.GradScaler's step() + update()
// (tc.py:4533-4546, engine_pretrain.py:65-72 through misc.py:252-282) without its host read-back of found_inf
//   state[0] scale  [1] growth tracker  [2] found_inf of the last step  [3] skipped steps  [4] steps  [5] 1 / scale used
// ---------------------------------------------------------------------------------------------
__global__ void loss_scale_update_kernel(float* __restrict__ state, const float* __restrict__ stats, float* __restrict__ hyper,
                                         int n_groups, float growth, float backoff, int interval) {
  const float scale = state[0];
  const float found = (stats[1] + stats[2]) > 0.f ? 1.f : 0.f;
  const float tracker = state[1];
  __syncthreads();
  for (int g = threadIdx.x; g < n_groups; g += blockDim.x) {
    hyper[(long)g * kHyperStride + 9] = found;
    hyper[(long)g * kHyperStride + 10] = 1.0f / scale;
  }
  if (threadIdx.x == 0) {
    state[2] = found;
    state[4] += 1.f;
    state[5] = 1.0f / scale;
    if (found != 0.f) {
      state[0] = scale * backoff;
      state[1] = 0.f;
      state[3] += 1.f;
    } else {
      const float t = tracker + 1.f;
      if (t >= (float)interval) {
        const float grown = scale * growth;
        state[0] = fabsf(grown) < INFINITY ? grown : scale;  // a growth that overflows keeps the scale (torch._amp_update_scale_)
        state[1] = 0.f;
      } else {
        state[1] = t;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Row gather / scatter for the classifier's top block (engine.py BlockStack.backward, sparse_top): with out_token "cls" the head's
// backward leaves a gradient in ONE row per sample, and the MLP branch of the last block (dfc2 + dGELU, dfc1, LayerNorm backward,
// proj dgrad and three of the four weight gradients) sees nothing but those rows until the attention backward spreads them again.
// ---------------------------------------------------------------------------------------------
// dst[r][:] = src[idx[r]][:], rows of `words` 32-bit words (source row pitch ld_words)
__global__ __launch_bounds__(256) void gather_rows_kernel(const unsigned int* __restrict__ src, long ld_words, const int* __restrict__ idx,
                                                          unsigned int* __restrict__ dst, int R, long words) {
  const long total = (long)R * words;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = i / words;
    const long w = i % words;
    dst[i] = src[(long)idx[r] * ld_words + w];
  }
}
// dst[m][:] = inv[m] >= 0 ? src[inv[m]][:] : 0 for all M rows of `vecs` 16-byte vectors
__global__ __launch_bounds__(256) void scatter_rows_zero_kernel(const u32x4* __restrict__ src, const int* __restrict__ inv,
                                                                u32x4* __restrict__ dst, int M, long vecs) {
  const long total = (long)M * vecs;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = i / vecs;
    const long v = i % vecs;
    const int r = inv[m];
    dst[i] = r >= 0 ? src[(long)r * vecs + v] : u32x4{0u, 0u, 0u, 0u};
  }
}

}  // namespace

extern "C" int pm_colsum_ws(const void* x, long ldx, int dtype, float* out, int M, int N, void* workspace, size_t ws_bytes,
                            void* stream) {
  if (!x || !out) return PM_EINVAL;
  if (M <= 0 || N <= 0 || (N & 3) || (ldx & 3)) return PM_ESHAPE;
  const int splits = cap_grid(M, 64, 128);
  const dim3 grid((N + 255) / 256, splits);
  float* partials = (workspace && ws_bytes >= (size_t)splits * N * sizeof(float)) ? reinterpret_cast<float*>(workspace) : nullptr;
  hipStream_t s = pm_stream(stream);
  PM_DISPATCH_ACT(dtype, T, hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, s, (const T*)x, ldx, out, partials, M, N));
  if (partials)
    hipLaunchKernelGGL(reduce_partial_rows<8>, dim3((N + 63) / 64), dim3(1024), 0, s, partials, (long)N, splits, N, out, (float*)nullptr,
                       (float*)nullptr);
  return pm_check_launch();
}

extern "C" int pm_colsum(const void* x, long ldx, int dtype, float* out, int M, int N, void* stream) {
  return pm_colsum_ws(x, ldx, dtype, out, M, N, nullptr, 0, stream);
}

extern "C" int pm_patch_im2col(const float* imgs, const int* ids_keep, void* cols, long ldcols, int out_dtype, int B, int C,
                               int img, int p, int keep, void* stream) {
  if (!imgs || !cols) return PM_EINVAL;
  if (B <= 0 || C <= 0 || img <= 0 || p <= 0 || keep <= 0 || (img % p)) return PM_ESHAPE;
  if (ldcols < (long)C * p * p) return PM_ESHAPE;
  if ((p & 3) == 0 && (ldcols & 3)) return PM_EALIGN;  // (vector stores)
  const int L = (img / p) * (img / p);
  if (keep > L || (!ids_keep && keep != L)) return PM_ESHAPE;
  const dim3 grid(B * keep);
  PM_DISPATCH_ACT(out_dtype, T, hipLaunchKernelGGL(im2col_kernel<T>, grid, dim3(256), 0, pm_stream(stream), imgs, ids_keep, (T*)cols,
                                                   ldcols, C, img, p, keep));
  return pm_check_launch();
}

extern "C" int pm_pad_cast(const float* src, long lds, void* dst, long ldd, int dst_dtype, int rows, int cols, int rows_pad,
                           int cols_pad, void* stream) {
  if (!src || !dst) return PM_EINVAL;
  if (rows <= 0 || cols <= 0 || rows_pad < rows || cols_pad < cols || lds < cols || ldd < cols_pad) return PM_ESHAPE;
  const long total = (long)rows_pad * cols_pad;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  PM_DISPATCH_ACT(dst_dtype, T, hipLaunchKernelGGL(pad_cast_kernel<T>, dim3(grid), dim3(256), 0, pm_stream(stream), src, lds, (T*)dst,
                                                   ldd, rows, cols, rows_pad, cols_pad));
  return pm_check_launch();
}

extern "C" int pm_unpad_add(const float* src, long lds, float* dst, long ldd, int rows, int cols, int accumulate, void* stream) {
  if (!src || !dst) return PM_EINVAL;
  if (rows <= 0 || cols <= 0 || lds < cols || ldd < cols) return PM_ESHAPE;
  const long total = (long)rows * cols;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(unpad_add_kernel, dim3(grid), dim3(256), 0, pm_stream(stream), src, lds, dst, ldd, rows, cols, accumulate ? 1 : 0);
  return pm_check_launch();
}

extern "C" int pm_assemble_tokens(const float* emb, const float* cls, const float* pos, const int* ids_keep, float* x,
                                  int B, int keep, int D, void* stream) {
  if (!emb || !cls || !pos || !x) return PM_EINVAL;
  if (B <= 0 || keep <= 0 || D <= 0 || (D & 3)) return PM_ESHAPE;
  hipLaunchKernelGGL(assemble_kernel, dim3(cap_grid((long)B * (keep + 1), 4, 4096)), dim3(256), 0, pm_stream(stream), emb,
                     cls, pos, ids_keep, x, B, keep, D);
  return pm_check_launch();
}

extern "C" int pm_assemble_tokens_bwd(const float* dx, const int* ids_keep, void* demb, int act_dtype, float* dcls,
                                      float* dpos, int B, int keep, int D, void* stream) {
  if (!dx || !demb) return PM_EINVAL;
  if (B <= 0 || keep <= 0 || D <= 0 || (D & 3)) return PM_ESHAPE;
  const dim3 grid(cap_grid((long)B * keep, 4, 4096));
  PM_DISPATCH_ACT(act_dtype, T, hipLaunchKernelGGL(assemble_bwd_kernel<T>, grid, dim3(256), 0, pm_stream(stream), dx, ids_keep,
                                                   (T*)demb, dpos, B, keep, D));
  if (dcls || dpos)  // dpos[0] gets the cls rows' sum whether or not the cls token itself is trained
    hipLaunchKernelGGL(cls_grad_kernel, dim3((D + 63) / 64), dim3(256), 0, pm_stream(stream), dx, dcls, dpos, B,
                       (long)(keep + 1) * D, D);
  return pm_check_launch();
}

extern "C" int pm_preprocess_u8(const unsigned char* src, const unsigned char* flip_flags, float* dst, int B, int H, int W,
                                float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b,
                                void* stream) {
  if (!src || !dst) return PM_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || (W & 3)) return PM_ESHAPE;
  if (((uintptr_t)dst & 15)) return PM_EALIGN;
  if (!(std_r > 0.f) || !(std_g > 0.f) || !(std_b > 0.f)) return PM_EINVAL;
  const long total = (long)B * H * (W >> 2);
  const dim3 grid(cap_grid(total, 256, 8192));
  hipLaunchKernelGGL(preprocess_u8_kernel, grid, dim3(256), 0, pm_stream(stream), src, flip_flags, dst, B, H, W,
                     f32x4{mean_r, mean_g, mean_b, 0.f}, f32x4{std_r, std_g, std_b, 1.f});
  return pm_check_launch();
}

extern "C" int pm_cast(const float* src, void* dst, int dst_dtype, long n, void* stream) {
  if (!src || !dst) return PM_EINVAL;
  if (n <= 0) return PM_ESHAPE;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return PM_EALIGN;
  const dim3 grid(cap_grid(n >> 2, 256, 4096));
  PM_DISPATCH_ACT(dst_dtype, T, hipLaunchKernelGGL(cast_kernel<T>, grid, dim3(256), 0, pm_stream(stream), src, (T*)dst, n));
  return pm_check_launch();
}

extern "C" int pm_gather_rows(const void* src, long ld_bytes, const int* idx, void* dst, int R, long row_bytes, void* stream) {
  if (!src || !idx || !dst) return PM_EINVAL;
  if (R <= 0 || row_bytes <= 0 || ld_bytes < row_bytes) return PM_ESHAPE;
  if ((row_bytes & 3) || (ld_bytes & 3) || ((uintptr_t)src & 3) || ((uintptr_t)dst & 3)) return PM_EALIGN;
  const long total = (long)R * (row_bytes >> 2);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(cap_grid(total, 256, 4096)), dim3(256), 0, pm_stream(stream), (const unsigned int*)src,
                     ld_bytes >> 2, idx, (unsigned int*)dst, R, row_bytes >> 2);
  return pm_check_launch();
}

extern "C" int pm_scatter_rows_zero(const void* src, const int* inv, void* dst, int M, long row_bytes, void* stream) {
  if (!src || !inv || !dst) return PM_EINVAL;
  if (M <= 0 || row_bytes <= 0) return PM_ESHAPE;
  if ((row_bytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return PM_EALIGN;
  const long total = (long)M * (row_bytes >> 4);
  hipLaunchKernelGGL(scatter_rows_zero_kernel, dim3(cap_grid(total, 256, 8192)), dim3(256), 0, pm_stream(stream), (const u32x4*)src, inv,
                     (u32x4*)dst, M, row_bytes >> 4);
  return pm_check_launch();
}

extern "C" int pm_dgelu(const void* dy, const void* pre, void* out, int dtype, long n, void* stream) {
  if (!dy || !pre || !out) return PM_EINVAL;
  if (n <= 0 || (n & 3)) return PM_ESHAPE;
  if (((uintptr_t)dy & 7) || ((uintptr_t)pre & 7) || ((uintptr_t)out & 7)) return PM_EALIGN;
  const dim3 grid(cap_grid(n >> 2, 256, 4096));
  PM_DISPATCH_ACT(dtype, T, hipLaunchKernelGGL(dgelu_kernel<T>, grid, dim3(256), 0, pm_stream(stream), (const T*)dy, (const T*)pre,
                                               (T*)out, n));
  return pm_check_launch();
}

// The AdamW kernels move p, g, m, v (and an f32 shadow) as 16-byte vectors and a 16-bit shadow as 8-byte ones.
static bool adamw_aligned(const void* p, const void* g, const void* m, const void* v, const void* shadow, int shadow_dtype) {
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return false;
  return !shadow || !((uintptr_t)shadow & (shadow_dtype == PM_F32 ? 15 : 7));
}

extern "C" int pm_adamw(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, long n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                        void* stream) {
  if (!p || !g || !m || !v) return PM_EINVAL;
  if (n <= 0 || (n & 3) || step < 1) return PM_ESHAPE;
  if (shadow && shadow_dtype != PM_BF16 && shadow_dtype != PM_F16 && shadow_dtype != PM_F32) return PM_EINVAL;
  if (!adamw_aligned(p, g, m, v, shadow, shadow_dtype)) return PM_EALIGN;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const dim3 grid(cap_grid(n >> 2, 256, 4096));
  if (!shadow) shadow_dtype = PM_BF16;
  PM_DISPATCH_ACT(shadow_dtype, T, hipLaunchKernelGGL(adamw_kernel<T>, grid, dim3(256), 0, pm_stream(stream), p, g, m, v, (T*)shadow, n,
                                                      lr, beta1, beta2, eps, weight_decay, (float)bc1, rsqrt_bc2, grad_scale));
  return pm_check_launch();
}


extern "C" int pm_adamw_tick(float* hyper, int n_groups, void* stream) {
  if (!hyper) return PM_EINVAL;
  if (n_groups <= 0) return PM_ESHAPE;
  hipLaunchKernelGGL(adamw_tick_kernel, dim3((n_groups + 63) / 64), dim3(64), 0, pm_stream(stream), hyper, n_groups);
  return pm_check_launch();
}

// Workgroups of one adamw_dev_kernel launch over n elements.  max_blocks = 0: the full grid (one workgroup per 256 vectors, at
// most 4096: fastest when the update runs alone); max_blocks > 0: one workgroup per chunk of kAdamwChunk vectors, at most
// max_blocks (the footprint an update beside other kernels is held to).
extern "C" int pm_adamw_grid(long n, int max_blocks) {
  if (n <= 0 || (n & 3) || max_blocks < 0) return PM_ESHAPE;
  return max_blocks == 0 ? cap_grid(n >> 2, 256, 4096) : cap_grid(n >> 2, kAdamwChunk, max_blocks);
}

static int adamw_dev_check(const float* p, const float* g, const float* m, const float* v, const void* shadow, int shadow_dtype,
                           long n, const float* hyper) {
  if (!p || !g || !m || !v || !hyper) return PM_EINVAL;
  if (n <= 0 || (n & 3)) return PM_ESHAPE;
  if (shadow && shadow_dtype != PM_BF16 && shadow_dtype != PM_F16 && shadow_dtype != PM_F32) return PM_EINVAL;
  if (!adamw_aligned(p, g, m, v, shadow, shadow_dtype)) return PM_EALIGN;
  return PM_OK;
}

static int adamw_dev_launch(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, long n, const float* hyper,
                            int max_blocks, void* stream) {
  const dim3 grid(pm_adamw_grid(n, max_blocks));
  if (!shadow) shadow_dtype = PM_BF16;
  PM_DISPATCH_ACT(shadow_dtype, T, hipLaunchKernelGGL(adamw_dev_kernel<T>, grid, dim3(256), 0, pm_stream(stream), p, g, m, v, (T*)shadow,
                                                      n, hyper));
  return pm_check_launch();
}

extern "C" int pm_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, long n,
                            const float* hyper, void* stream) {
  const int st = adamw_dev_check(p, g, m, v, shadow, shadow_dtype, n, hyper);
  if (st != PM_OK) return st;
  return adamw_dev_launch(p, g, m, v, shadow, shadow_dtype, n, hyper, 0, stream);
}

// The whole update in one call: [wait_event ->] tick -> per segment (launch [-> done_event]).  Everything is checked before the
// first enqueue, so a refusal leaves the stream untouched.
extern "C" int pm_adamw_segments(const pm_adamw_segment* segs, int n_segs, float* hyper, int n_groups, void* wait_event, void* stream,
                                 int max_blocks) {
  if (!segs || !hyper) return PM_EINVAL;
  if (n_segs <= 0 || n_groups <= 0 || max_blocks < 0) return PM_ESHAPE;
  for (int i = 0; i < n_segs; ++i) {
    const pm_adamw_segment& s = segs[i];
    const int st = adamw_dev_check(s.p, s.g, s.m, s.v, s.shadow, s.shadow_dtype, s.n, s.hyper);
    if (st != PM_OK) return st;
  }
  hipStream_t q = pm_stream(stream);
  if (wait_event && hipStreamWaitEvent(q, (hipEvent_t)wait_event, 0) != hipSuccess) return PM_ELAUNCH;
  int st = pm_adamw_tick(hyper, n_groups, stream);
  if (st != PM_OK) return st;
  for (int i = 0; i < n_segs; ++i) {
    const pm_adamw_segment& s = segs[i];
    st = adamw_dev_launch(s.p, s.g, s.m, s.v, s.shadow, s.shadow_dtype, s.n, s.hyper, max_blocks, stream);
    if (st != PM_OK) return st;
    if (s.done_event && hipEventRecord((hipEvent_t)s.done_event, q) != hipSuccess) return PM_ELAUNCH;
  }
  return PM_OK;
}

// `list` is what the kernel reads (device memory, fixed address: a captured step replays it); `list_host` is the caller's host
// copy of the same n_list indices, which is what can be checked here without a read-back: strictly ascending, inside [0, n_records).
static int tick_list_check(const float* hyper, int n_records, const int* list, const int* list_host, int n_list) {
  if (!hyper || !list || !list_host) return PM_EINVAL;
  if (n_records <= 0 || n_list <= 0 || n_list > n_records) return PM_ESHAPE;
  for (int i = 0; i < n_list; ++i) {
    if (list_host[i] < 0 || list_host[i] >= n_records) return PM_EINVAL;
    if (i && list_host[i] <= list_host[i - 1]) return PM_EINVAL;
  }
  if ((uintptr_t)list & 3) return PM_EALIGN;
  return PM_OK;
}

extern "C" int pm_adamw_tick_list(float* hyper, int n_records, const int* list, const int* list_host, int n_list, void* stream) {
  const int st = tick_list_check(hyper, n_records, list, list_host, n_list);
  if (st != PM_OK) return st;
  hipLaunchKernelGGL(adamw_tick_list_kernel, dim3((n_list + 63) / 64), dim3(64), 0, pm_stream(stream), hyper, n_records, list, n_list);
  return pm_check_launch();
}

// pm_adamw_segments with the tick over a list: every check of both before the first enqueue.
extern "C" int pm_adamw_segments_list(const pm_adamw_segment* segs, int n_segs, float* hyper, int n_records, const int* list,
                                      const int* list_host, int n_list, void* wait_event, void* stream, int max_blocks) {
  if (!segs || !hyper) return PM_EINVAL;
  if (n_segs <= 0 || max_blocks < 0) return PM_ESHAPE;
  int st = tick_list_check(hyper, n_records, list, list_host, n_list);
  if (st != PM_OK) return st;
  for (int i = 0; i < n_segs; ++i) {
    const pm_adamw_segment& s = segs[i];
    st = adamw_dev_check(s.p, s.g, s.m, s.v, s.shadow, s.shadow_dtype, s.n, s.hyper);
    if (st != PM_OK) return st;
    // a segment's record must be one of this array's, on a record boundary
    if (s.hyper < hyper || s.hyper >= hyper + (long)n_records * kHyperStride || (s.hyper - hyper) % kHyperStride) return PM_EINVAL;
  }
  hipStream_t q = pm_stream(stream);
  if (wait_event && hipStreamWaitEvent(q, (hipEvent_t)wait_event, 0) != hipSuccess) return PM_ELAUNCH;
  st = pm_adamw_tick_list(hyper, n_records, list, list_host, n_list, stream);
  if (st != PM_OK) return st;
  for (int i = 0; i < n_segs; ++i) {
    const pm_adamw_segment& s = segs[i];
    st = adamw_dev_launch(s.p, s.g, s.m, s.v, s.shadow, s.shadow_dtype, s.n, s.hyper, max_blocks, stream);
    if (st != PM_OK) return st;
    if (s.done_event && hipEventRecord((hipEvent_t)s.done_event, q) != hipSuccess) return PM_ELAUNCH;
  }
  return PM_OK;
}

extern "C" int pm_loss_scale_update(float* state, const float* stats, float* hyper, int n_groups, float growth_factor,
                                    float backoff_factor, int growth_interval, void* stream) {
  if (!state || !stats || !hyper) return PM_EINVAL;
  if (n_groups <= 0 || growth_interval <= 0 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f)) return PM_ESHAPE;
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, pm_stream(stream), state, stats, hyper, n_groups,
                     growth_factor, backoff_factor, growth_interval);
  return pm_check_launch();
}

extern "C" int pm_grad_stats(const float* g, long n, float* out, void* stream) {
  if (!g || !out) return PM_EINVAL;
  if (n <= 0) return PM_ESHAPE;
  if ((uintptr_t)g & 15) return PM_EALIGN;
  hipLaunchKernelGGL(grad_stats_kernel, dim3(cap_grid(n >> 2, 256, 1024)), dim3(256), 0, pm_stream(stream), g, n, out);
  return pm_check_launch();
}

extern "C" const char* pm_strerror(int status) {
  switch (status) {
    case PM_OK: return "ok";
    case PM_EINVAL: return "invalid argument (null pointer / unknown dtype or epilogue)";
    case PM_ESHAPE: return "unsupported shape";
    case PM_EARCH: return "no gfx950 device";
    case PM_ELAUNCH: return "kernel launch failed";
    case PM_EALIGN: return "pointer / leading dimension not 16-byte aligned";
    default: return "unknown status";
  }
}

// 3: pm_gemm_ex / pm_gemm_opts replace pm_tune, workspace queries, pm_vit_head_*, pm_supervised_loss_fwd, pm_scale
// 10: PM_F16 (precision mode fp16), pm_loss_scale_update, pm_dgelu
// 15: pm_gemm_plan; pm_gemm_opts.variant names shipped kernels only (anything else: PM_EINVAL)
// 16: pm_attention_plan; pm_gemm_colsum and PM_WS_GEMM_COLSUM are gone (pm_gemm_ws, then pm_colsum_ws)
extern "C" int pm_abi_version(void) { return 16; }

extern "C" size_t pm_workspace_bytes(int kind, int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  switch (kind) {
    case PM_WS_LAYERNORM_BWD: {  // one partial row triple per block, grid = min(ceil(M/4), 1024)
      long g = (M + 3) / 4;
      if (g > 1024) g = 1024;
      if (g < 64) g = 64;
      return (size_t)g * 3 * N * sizeof(float);
    }
    case PM_WS_COLSUM: return (size_t)cap_grid(M, 64, 128) * N * sizeof(float);
    case PM_WS_UNSHUFFLE_BWD: return (size_t)1024 * N * sizeof(float);  // partial rows of the mask-token gradient
    default: return 0;
  }
}
