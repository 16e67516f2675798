// pm_droppath.hip -- stochastic depth (timm 0.4.12 DropPath, mae/main_finetune.py:251 `drop_path_rate`) as per-sample scales of a
// block's two residual branches: x = x + s[b] * f(LN(x)) with s[b] in {0, 1 / keep} drawn per sample and branch.
// Three streaming kernels around the unchanged GEMM / LayerNorm / attention kernels:
//   drop_path_add         out[r,:] = x[r,:] + s[r / N] * y[r,:]            (forward: the residual add behind a branch's last GEMM)
//   drop_path_scale_cast  dy_act[r,:] = cast(s[r / N] * dy[r,:]), colsum += sum_r s[r / N] * dy[r,:]
//                                                                         (backward: what the branch's dgrad and weight gradients read,
//                                                                          and the bias gradient of the branch's last Linear)
//   drop_path_scales      noise -> scale table
// Compiled with -ffp-contract=off: the product is rounded before the sum, as torch's `x + y * s[:, None]` rounds it.  No float
// atomics; the column sum goes through partial rows and reduce_partial_rows (pm_common.h) in a fixed order.
#include "pm_common.h"

namespace {

constexpr int kAddUnroll = 4;   // 16-byte vectors a thread has in flight (x and y each)
constexpr int kCastRows = 4;    // rows a wave has in flight

// `y` and `out` carry no __restrict__: out may be y (in place on the buffer the GEMM wrote); a thread reads its vector before it
// writes it and no other thread touches it.
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* __restrict__ x, const float* y, float* out,
                                                            const float* __restrict__ scale, long total, int V, int N) {
  const long step = (long)gridDim.x * 256;
  for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += step * kAddUnroll) {
    f32x4 xv[kAddUnroll], yv[kAddUnroll];
    float s[kAddUnroll];
#pragma unroll
    for (int u = 0; u < kAddUnroll; ++u) {
      const long i = i0 + u * step;
      if (i < total) {
        xv[u] = *reinterpret_cast<const f32x4*>(x + 4 * i);
        yv[u] = *reinterpret_cast<const f32x4*>(y + 4 * i);
        s[u] = scale[(i / V) / N];
      }
    }
#pragma unroll
    for (int u = 0; u < kAddUnroll; ++u) {
      const long i = i0 + u * step;
      if (i < total) {
        const f32x4 p = yv[u] * s[u];   // rounded here (no contraction), then the sum
        *reinterpret_cast<f32x4*>(out + 4 * i) = xv[u] + p;
      }
    }
  }
}

// The first stage of colsum_kernel (pm_misc.hip) with the scale and the cast on the way: blockIdx.x = 256-column strip, blockIdx.y = row
// split; wave w of split y takes rows 4 y + w, + 4 gridDim.y, ..., kCastRows of them in flight.  kSum = false: no sums, no LDS.
template <typename T, bool kSum>
__global__ __launch_bounds__(256) void drop_path_scale_cast_kernel(const float* __restrict__ dy, const float* __restrict__ scale,
                                                                   T* __restrict__ dy_act, float* __restrict__ partials, int M, int N,
                                                                   int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 256 + lane * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (n < D) {
    const long step = (long)gridDim.y * 4;
    for (long m0 = (long)blockIdx.y * 4 + wave; m0 < M; m0 += step * kCastRows) {
      f32x4 v[kCastRows];
      float s[kCastRows];
#pragma unroll
      for (int u = 0; u < kCastRows; ++u) {
        const long m = m0 + u * step;
        if (m < M) {
          v[u] = *reinterpret_cast<const f32x4*>(dy + m * D + n);
          s[u] = scale[m / N];
        }
      }
#pragma unroll
      for (int u = 0; u < kCastRows; ++u) {
        const long m = m0 + u * step;
        if (m < M) {
          const f32x4 p = v[u] * s[u];
          store4<T>(dy_act + m * D + n, p);
          if (kSum) acc += p;
        }
      }
    }
  }
  if (kSum) block_colsum_tail(acc, nullptr, partials, D);   // (partials is never NULL here: no atomics)
}

__global__ __launch_bounds__(256) void drop_path_scales_kernel(const float* __restrict__ noise, const float* __restrict__ rates,
                                                               float* __restrict__ out, int depth, int B) {
  const long total = (long)depth * 2 * B;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const float keep = 1.0f - rates[i / (2 * (long)B)];
    const float t = keep + noise[i];                       // timm: random_tensor = keep_prob + rand; floor_() -> 1 iff >= 1
    out[i] = t >= 1.0f ? __fdiv_rn(1.0f, keep) : 0.f;      // x.div(keep_prob) by a scalar = x * fl32(1 / keep)
  }
}

int cast_splits(int M) { return cap_grid(M, 16, 512); }

}  // namespace

extern "C" int pm_drop_path_add(const float* x, const float* y, float* out, const float* scale, int M, int N, int D, void* stream) {
  if (!x || !y || !out || !scale) return PM_EINVAL;
  if (M <= 0 || N <= 0 || D <= 0 || (D & 3) || (M % N)) return PM_ESHAPE;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15) return PM_EALIGN;
  const long total = (long)M * (D >> 2);
  hipLaunchKernelGGL(drop_path_add_kernel, dim3(cap_grid(total, 256 * kAddUnroll, 4096)), dim3(256), 0, pm_stream(stream), x, y, out,
                     scale, total, D >> 2, N);
  return pm_check_launch();
}

extern "C" int pm_drop_path_workspace(int M, int D, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (M <= 0 || D <= 0 || (D & 3)) return PM_ESHAPE;
  *bytes = (size_t)cast_splits(M) * D * sizeof(float);
  return PM_OK;
}

extern "C" int pm_drop_path_scale_cast(const float* dy, const float* scale, void* dy_act, int act_dtype, float* colsum, int M, int N,
                                       int D, void* workspace, size_t ws_bytes, void* stream) {
  if (!dy || !scale || !dy_act) return PM_EINVAL;
  if (M <= 0 || N <= 0 || D <= 0 || (D & 3) || (M % N)) return PM_ESHAPE;
  if (((uintptr_t)dy | (uintptr_t)dy_act | (uintptr_t)workspace) & 15) return PM_EALIGN;
  const int splits = cast_splits(M);
  if (colsum && (!workspace || ws_bytes < (size_t)splits * D * sizeof(float))) return PM_EINVAL;
  float* partials = reinterpret_cast<float*>(workspace);
  const dim3 grid((D + 255) / 256, splits);
  hipStream_t s = pm_stream(stream);
  if (colsum) {
    PM_DISPATCH_ACT(act_dtype, T, hipLaunchKernelGGL((drop_path_scale_cast_kernel<T, true>), grid, dim3(256), 0, s, dy, scale,
                                                     (T*)dy_act, partials, M, N, D));
    hipLaunchKernelGGL(reduce_partial_rows<8>, dim3((D + 63) / 64), dim3(1024), 0, s, partials, (long)D, splits, D, colsum,
                       (float*)nullptr, (float*)nullptr);
  } else {
    PM_DISPATCH_ACT(act_dtype, T, hipLaunchKernelGGL((drop_path_scale_cast_kernel<T, false>), grid, dim3(256), 0, s, dy, scale,
                                                     (T*)dy_act, (float*)nullptr, M, N, D));
  }
  return pm_check_launch();
}

extern "C" int pm_drop_path_scales(const float* noise, const float* rates, float* out, int depth, int B, void* stream) {
  if (!noise || !rates || !out) return PM_EINVAL;
  if (depth <= 0 || B <= 0) return PM_ESHAPE;
  hipLaunchKernelGGL(drop_path_scales_kernel, dim3(cap_grid((long)depth * 2 * B, 256, 1024)), dim3(256), 0, pm_stream(stream), noise,
                     rates, out, depth, B);
  return pm_check_launch();
}
