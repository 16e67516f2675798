// pm_gradclip.hip -- per-group gradient norms and clipping by global norm on the device (include/polypmae.h: pm_grad_norms,
// pm_grad_clip).
//
// The reference computes one gradient norm per parameter group and the global one after scaler.unscale_
// (train_classification.py:4534-4544, _compute_grad_norm :1437-1454: a host read-back per parameter) and clips by global norm in
// its AMP helper (mae/util/misc.py:268-279: unscale_ -> torch.nn.utils.clip_grad_norm_ -> step).  Here the gradients stay where
// they are, scaled: one pass sums g^2 per group, and the clip coefficient is folded into slot [10] of the AdamW records -- the
// factor adamw_dev_kernel (pm_misc.hip) already multiplies every gradient by.  The update kernels are not touched.
//
// These sums decide the weights, so they are deterministic: no float atomics.  Every value is squared and accumulated in f64 (the
// product of two f32 values is exact in f64; 1e18^2 is far inside its range), by a fixed map of elements to lanes, and reduced by
// fixed trees:
//   grad_norms_partial_kernel  one launch per batch of kBatch segments.  The segments of a batch are cut into chunks of
//                              kChunk 16-byte vectors; workgroup b walks chunks [b per, (b + 1) per).  A lane keeps one f64 sum and
//                              two counters; whenever the group changes (uniform over the workgroup) the workgroup reduces them and
//                              lane 0 adds the result to ITS row of the workspace: [sum g^2, #NaN, #Inf] per group, f64.
//   grad_norms_reduce_kernel   one workgroup sums the rows in a fixed order: f64 [G] sums, and the f32 triple pm_loss_scale_update reads.
//   grad_clip_kernel           one lane: the norms of the gradient as the update consumes it, the coefficient of
//                              torch.nn.utils.clip_grad_norm_, the new slot [10], the f64 record.
// The grid is a function of the segment sizes alone, never of the stream or of capture: every mode gives the same bits.
#include <float.h>

#include "pm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PM_WAVE;
constexpr int kUnroll = 4;
constexpr int kChunk = kThreads * kUnroll;  // 16-byte vectors per chunk: 16 KiB of gradient
constexpr int kMaxBlocks = 1024;            // workgroups per launch
constexpr int kBatch = 64;                  // segments per launch (they travel as kernel arguments)
constexpr int kHyperStride = 16;            // floats per AdamW record (pm_misc.hip)
constexpr long kMaxChunks = 1L << 30;

struct GradBatch {
  const float* g[kBatch];
  long nvec[kBatch];
  int chunk0[kBatch + 1];  // first chunk of each segment; [n_segs] = chunks of the batch
  int group[kBatch];
  int n_segs;
};

// the workgroup's [sum, #NaN, #Inf] since the last flush, added to row[0..3) by lane 0; called under uniform control flow
__device__ __forceinline__ void flush_group(double& ss, unsigned& nn, unsigned& ni, double* __restrict__ row, double (*red)[kWaves]) {
  const double a = wave_sum_f64(ss), b = wave_sum_f64((double)nn), c = wave_sum_f64((double)ni);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
    red[2][wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) row[k] += (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  }
  __syncthreads();
  ss = 0.0, nn = 0u, ni = 0u;
}

__global__ __launch_bounds__(kThreads) void grad_norms_partial_kernel(const GradBatch b, int per, int n_groups,
                                                                      double* __restrict__ partials) {
  __shared__ double red[3][kWaves];
  double* row = partials + (long)blockIdx.x * n_groups * 3;
  if (threadIdx.x == 0) {  // (lane 0 alone reads and writes this row)
    for (int i = 0; i < n_groups * 3; ++i) row[i] = 0.0;
  }
  const int total = b.chunk0[b.n_segs];
  const int c_lo = blockIdx.x * per;
  const int c_hi = c_lo + per < total ? c_lo + per : total;
  double ss = 0.0;
  unsigned nn = 0u, ni = 0u;
  int s = 0, cur = -1;
  for (int c = c_lo; c < c_hi; ++c) {
    while (c >= b.chunk0[s + 1]) ++s;
    const int grp = b.group[s];
    if (grp != cur) {
      if (cur >= 0) flush_group(ss, nn, ni, row + cur * 3, red);
      cur = grp;
    }
    const float* __restrict__ g = b.g[s];
    const long nvec = b.nvec[s];
    const long i0 = (long)(c - b.chunk0[s]) * kChunk + threadIdx.x;
    f32x4 v[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const long i = i0 + k * kThreads;
      v[k] = i < nvec ? *reinterpret_cast<const f32x4*>(g + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = v[k][e];
        ss += (double)x * (double)x;
        nn += (x != x) ? 1u : 0u;
        ni += (fabsf(x) == INFINITY) ? 1u : 0u;
      }
    }
  }
  if (cur >= 0) flush_group(ss, nn, ni, row + cur * 3, red);
}

__global__ __launch_bounds__(kThreads) void grad_norms_reduce_kernel(const double* __restrict__ partials, int rows, int n_groups,
                                                                     double* __restrict__ sumsq, float* __restrict__ stats) {
  __shared__ double red[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int width = n_groups * 3;
  double tot[3] = {0.0, 0.0, 0.0};  // (lane 0's)
  for (int q = 0; q < width; ++q) {
    double a = 0.0;
    for (int r = threadIdx.x; r < rows; r += kThreads) a += partials[(long)r * width + q];
    a = wave_sum_f64(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double v = (red[0] + red[1]) + (red[2] + red[3]);
      if (q % 3 == 0) sumsq[q / 3] = v;
      tot[q % 3] += v;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[0] = (float)tot[0];
    stats[1] = (float)tot[1];
    stats[2] = (float)tot[2];
  }
}

// s_g = grad_scale x (1 / loss scale when `scaled` and slot [10] holds one): what adamw_dev_kernel multiplies group g's gradients
// by before this kernel touches [10].  record: [0, G) the groups' norms, [G] the total, [G + 1] coef, [G + 2] max_norm.
__global__ void grad_clip_kernel(const double* __restrict__ sumsq, float* __restrict__ hyper, int n_groups, double max_norm, int clip,
                                 int scaled, double* __restrict__ record) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double tot = 0.0;
  for (int g = 0; g < n_groups; ++g) {
    const float* h = hyper + (long)g * kHyperStride;
    const float base = (scaled && h[10] != 0.f) ? h[10] : 1.0f;
    const double s = (double)h[5] * (double)base;
    record[g] = sqrt(sumsq[g]) * s;
    tot += sumsq[g] * s * s;
  }
  const double total = sqrt(tot);
  double coef = 1.0;
  if (clip) {
    coef = max_norm / (total + 1e-6);   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
    if (coef > 1.0) coef = 1.0;         // (a NaN passes both comparisons, as it passes torch.clamp)
    if (coef < (double)FLT_MIN) coef = (double)FLT_MIN;
    for (int g = 0; g < n_groups; ++g) {
      float* h = hyper + (long)g * kHyperStride;
      const float base = (scaled && h[10] != 0.f) ? h[10] : 1.0f;
      float w = (float)((double)base * coef);
      if (w < FLT_MIN) w = FLT_MIN;     // never the 0 that means "no scaling"
      h[10] = w;
    }
  }
  record[n_groups] = total;
  record[n_groups + 1] = coef;
  record[n_groups + 2] = clip ? max_norm : (double)INFINITY;
}

// grad_clip_kernel over cohort records (per-parameter steps: a param group owns one AdamW record per cohort, pm_misc.hip).  sumsq
// has one sum per RECORD; group g's sum is the sum of its records' in ascending record order, and from there on this is
// grad_clip_kernel's arithmetic expression by expression: with n_records == n_groups and group_of[r] == r the bits are the same
// (0.0 + x == x for the sums this pass produces, which are never -0).  s_g is read from the group's first record: sync_hyper and
// pm_loss_scale_update write [5] and [10] alike into all records of a group.  A group without a record reports 0.
// An entry of group_of outside [0, n_groups) belongs to no group (the host refuses such a map before the launch).
__global__ void grad_clip_cohorts_kernel(const double* __restrict__ sumsq, float* __restrict__ hyper, int n_records,
                                         const int* __restrict__ group_of, int n_groups, double max_norm, int clip, int scaled,
                                         double* __restrict__ record) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double tot = 0.0;
  for (int g = 0; g < n_groups; ++g) {
    double gs = 0.0;
    int first = -1;
    for (int r = 0; r < n_records; ++r) {
      if (group_of[r] != g) continue;
      if (first < 0) first = r;
      gs += sumsq[r];
    }
    if (first < 0) {
      record[g] = 0.0;
      continue;
    }
    const float* h = hyper + (long)first * kHyperStride;
    const float base = (scaled && h[10] != 0.f) ? h[10] : 1.0f;
    const double s = (double)h[5] * (double)base;
    record[g] = sqrt(gs) * s;
    tot += gs * s * s;
  }
  const double total = sqrt(tot);
  double coef = 1.0;
  if (clip) {
    coef = max_norm / (total + 1e-6);
    if (coef > 1.0) coef = 1.0;
    if (coef < (double)FLT_MIN) coef = (double)FLT_MIN;
    for (int r = 0; r < n_records; ++r) {
      float* h = hyper + (long)r * kHyperStride;
      const float base = (scaled && h[10] != 0.f) ? h[10] : 1.0f;
      float w = (float)((double)base * coef);
      if (w < FLT_MIN) w = FLT_MIN;
      h[10] = w;
    }
  }
  record[n_groups] = total;
  record[n_groups + 1] = coef;
  record[n_groups + 2] = clip ? max_norm : (double)INFINITY;
}

// one row per workgroup of every launch: at most kMaxBlocks per batch of segments
size_t grad_ws_bytes(int n_segs, int n_groups) {
  const size_t batches = ((size_t)n_segs + kBatch - 1) / kBatch;
  return batches * kMaxBlocks * (size_t)n_groups * 3 * sizeof(double);
}

}  // namespace

extern "C" int pm_grad_norms_workspace(int n_segs, int n_groups, size_t* bytes) {
  if (!bytes) return PM_EINVAL;
  if (n_segs <= 0 || n_segs > (1 << 16) || n_groups <= 0 || n_groups > (1 << 16)) return PM_ESHAPE;
  *bytes = grad_ws_bytes(n_segs, n_groups);
  return PM_OK;
}

// Everything is checked before the first enqueue, so a refusal leaves the stream untouched.
extern "C" int pm_grad_norms(const pm_grad_segment* segs, int n_segs, int n_groups, void* workspace, size_t ws_bytes, double* sumsq,
                             float* stats, void* stream) {
  if (!segs || !workspace || !sumsq || !stats) return PM_EINVAL;
  if (n_segs <= 0 || n_segs > (1 << 16) || n_groups <= 0 || n_groups > (1 << 16)) return PM_ESHAPE;
  for (int i = 0; i < n_segs; ++i) {
    if (!segs[i].g) return PM_EINVAL;
    if (segs[i].n <= 0 || (segs[i].n & 3)) return PM_ESHAPE;
    if (segs[i].group < 0 || segs[i].group >= n_groups) return PM_EINVAL;
    if ((uintptr_t)segs[i].g & 15) return PM_EALIGN;
    if ((segs[i].n >> 2) / kChunk >= kMaxChunks / kBatch) return PM_ESHAPE;
  }
  if (ws_bytes < grad_ws_bytes(n_segs, n_groups)) return PM_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)sumsq & 7)) return PM_EALIGN;
  hipStream_t q = pm_stream(stream);
  double* partials = (double*)workspace;
  int rows = 0;
  for (int first = 0; first < n_segs; first += kBatch) {
    GradBatch b;
    b.n_segs = n_segs - first < kBatch ? n_segs - first : kBatch;
    int chunks = 0;
    for (int i = 0; i < kBatch; ++i) {
      const bool live = i < b.n_segs;
      b.g[i] = live ? segs[first + i].g : nullptr;
      b.nvec[i] = live ? segs[first + i].n >> 2 : 0;
      b.group[i] = live ? segs[first + i].group : 0;
      b.chunk0[i] = chunks;
      if (live) chunks += (int)((b.nvec[i] + kChunk - 1) / kChunk);
    }
    b.chunk0[kBatch] = chunks;  // (slots past n_segs hold the batch's total as well)
    const int per = (chunks + kMaxBlocks - 1) / kMaxBlocks;
    const int grid = (chunks + per - 1) / per;
    hipLaunchKernelGGL(grad_norms_partial_kernel, dim3(grid), dim3(kThreads), 0, q, b, per, n_groups,
                       partials + (long)rows * n_groups * 3);
    rows += grid;
  }
  hipLaunchKernelGGL(grad_norms_reduce_kernel, dim3(1), dim3(kThreads), 0, q, (const double*)partials, rows, n_groups, sumsq, stats);
  return pm_check_launch();
}

extern "C" int pm_grad_clip(const double* sumsq, float* hyper, int n_groups, double max_norm, int clip, int scaled, double* record,
                            void* stream) {
  if (!sumsq || !hyper || !record) return PM_EINVAL;
  if (n_groups <= 0) return PM_ESHAPE;
  if (clip && !(max_norm > 0.0)) return PM_EINVAL;
  if (((uintptr_t)sumsq & 7) || ((uintptr_t)record & 7)) return PM_EALIGN;
  hipLaunchKernelGGL(grad_clip_kernel, dim3(1), dim3(64), 0, pm_stream(stream), sumsq, hyper, n_groups, max_norm, clip, scaled, record);
  return pm_check_launch();
}

// `group_of` is what the kernel reads (device memory at a fixed address); `group_of_host` is the caller's host copy of the same
// n_records entries, checked here so that a refusal needs no read-back and leaves the stream untouched.
extern "C" int pm_grad_clip_cohorts(const double* sumsq, float* hyper, int n_records, const int* group_of, const int* group_of_host,
                                    int n_groups, double max_norm, int clip, int scaled, double* record, void* stream) {
  if (!sumsq || !hyper || !record || !group_of || !group_of_host) return PM_EINVAL;
  if (n_groups <= 0 || n_records <= 0 || n_records > (1 << 16) || n_groups > (1 << 16)) return PM_ESHAPE;
  if (clip && !(max_norm > 0.0)) return PM_EINVAL;
  for (int r = 0; r < n_records; ++r) {
    if (group_of_host[r] < 0 || group_of_host[r] >= n_groups) return PM_EINVAL;
  }
  if (((uintptr_t)sumsq & 7) || ((uintptr_t)record & 7) || ((uintptr_t)group_of & 3)) return PM_EALIGN;
  hipLaunchKernelGGL(grad_clip_cohorts_kernel, dim3(1), dim3(64), 0, pm_stream(stream), sumsq, hyper, n_records, group_of, n_groups,
                     max_norm, clip, scaled, record);
  return pm_check_launch();
}
