// pm_layernorm.hip -- LayerNorm forward / backward for the pre-LN ViT blocks (HBM-bound).
// Replaces nn.LayerNorm(eps=1e-6) of timm Block.norm1/norm2 and MaskedAutoencoderViT.norm/decoder_norm
// (reference models_mae.py:39-42,53-57,168,188).  One wave64 per row, the row lives in registers
// (D <= 1280, D % 4 == 0: 768 / 512 for ViT-B/16 and its MAE decoder, 1024 / 1280 for ViT-L / ViT-H; the number of f32x4 slots
// per lane is a template parameter), f32 statistics, two-pass variance.
// Algorithmic bytes per row: fwd 4D (x) + sizeof(act)*D (y); bwd sizeof(act)*D (dy) + 4D (x) + 4D (dres)
// + 4D (dx) + sizeof(act)*D (dx_act).
#include "pm_common.h"

namespace {

constexpr int kMaxD = 1280;  // 5 f32x4 slots per lane (ViT-H)

template <typename TOut, int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, TOut* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out, int M,
                                                     int D, float eps) {
  constexpr int kMaxVec = NV;  // f32x4 slots per lane for this D: D <= 256 * NV
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nvec = D >> 2;
  for (long row = (long)blockIdx.x * 4 + wave; row < M; row += (long)gridDim.x * 4) {
    const float* xr = x + row * ldx;
    f32x4 v[kMaxVec];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * c);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[i][e] - mean;
          q += d * d;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    TOut* yr = y + row * (long)D;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
        const f32x4 b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
        store4<TOut>(yr + 4 * c, o);
      }
    }
  }
}

// Backward.  One wave64 per row, rows gw, gw + W, gw + 2W, ... for wave gw of W = 4 * gridDim.x: which wave handles which row is a
// pure function of (M, grid), so the column sums are run-to-run deterministic.  One row is under arithmetic at a time while the
// next row's loads are in flight: the wave issues row r + W (x, dy, dres, mean, rstd) before the reductions and stores of row r,
// and dy stays in its 16-bit form until it is used.  What does not change from row to row lives in LDS, not in registers: gamma
// (read at each use) and the wave's three column accumulators (read-modify-write of the wave's own 16-byte-per-lane slots, no
// bank conflicts; 18 LDS instructions of 1 KB per row against 12 KB of HBM traffic).  That brings D <= 768 to at most 118 VGPRs
// and 39 KB of LDS per workgroup, i.e. 4 waves per SIMD, where two full f32 working sets and the accumulators took 182 VGPRs
// (2 waves); D = 1024 holds 3 and D = 1280 holds 2 (242 and 266 registers, 2 and 1 before).
// `dres` may alias `dx` row for row (so neither is `__restrict__`): a prefetched row is never the row being stored, and the loads
// of a row precede its own store by data dependence.  kRes: the launch has a residual (`dres` != NULL).  The launch bound is the
// minimum number of waves per SIMD the register allocator must leave room for.
template <typename TDy, typename TAct, int NV, bool kRes>
__global__ __launch_bounds__(256, NV <= 3 ? 4 : 1) void ln_bwd_kernel(const TDy* __restrict__ dy, const float* __restrict__ x, long ldx,
                                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                      const float* __restrict__ rstd, const float* dres, long lddres,
                                                                      float* dx, long lddx, TAct* __restrict__ dx_act,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                      float* __restrict__ dcolsum, float* __restrict__ partials,
                                                                      int M, int D) {
  __shared__ f32x4 gam[NV * 64];
  __shared__ f32x4 acc[3][4][NV * 64];  // [dgamma | dbeta | dcolsum][wave][column / 4]: each wave's column sums, touched by it alone
  constexpr int kMaxVec = NV;  // f32x4 slots per lane for this D (shadows the file-scope bound): D <= 256 * NV
  typedef TDy __attribute__((ext_vector_type(4))) Dy4;  // dy as loaded: 8 bytes per slot for the 16-bit types
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row addresses and mean / rstd stay scalar
  const int nvec = D >> 2;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int c = threadIdx.x; c < kMaxVec * 64; c += 256) gam[c] = (c < nvec) ? *reinterpret_cast<const f32x4*>(gamma + 4 * c) : z;
#pragma unroll
  for (int i = 0; i < kMaxVec; ++i) {
    acc[0][wave][lane + 64 * i] = z;
    acc[1][wave][lane + 64 * i] = z;
    acc[2][wave][lane + 64 * i] = z;
  }
  __syncthreads();
  const float invD = 1.0f / (float)D;
  const long stride = (long)gridDim.x * 4;
  long row = (long)blockIdx.x * 4 + wave;
  // the row in flight
  f32x4 nx[kMaxVec], ndr[kMaxVec];
  Dy4 ndy[kMaxVec];
  float nmu = 0.f, nrs = 0.f;
  auto fetch = [&](long r) {
    nmu = mean[r];
    nrs = rstd[r];
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (i < kMaxVec - 1 || c < nvec) {  // only the last slot can be ragged: D > 256 * (NV - 1)
        nx[i] = *reinterpret_cast<const f32x4*>(x + r * ldx + 4 * c);
        ndy[i] = *reinterpret_cast<const Dy4*>(dy + r * (long)D + 4 * c);
        if (kRes) ndr[i] = *reinterpret_cast<const f32x4*>(dres + r * lddres + 4 * c);
      }
    }
  };
  if (row < M) fetch(row);  // a wave without a row loads nothing
  while (row < M) {
    const float mu = nmu, rs = nrs;
    f32x4 xh[kMaxVec], dr[kMaxVec];
    Dy4 dv[kMaxVec];
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (i < kMaxVec - 1 || c < nvec) {  // only the last slot can be ragged: D > 256 * (NV - 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) xh[i][e] = (nx[i][e] - mu) * rs;
        dv[i] = ndy[i];
        if (kRes) dr[i] = ndr[i];
      }
    }
    const long next = row + stride;
    if (next < M) fetch(next);  // under this row's reductions and stores
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (i < kMaxVec - 1 || c < nvec) {  // only the last slot can be ragged: D > 256 * (NV - 1)
        const f32x4 g = gam[c];
        f32x4 ag = acc[0][wave][c], ab = acc[1][wave][c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = (float)dv[i][e];
          const float gg = d * g[e];
          s1 += gg;
          s2 += gg * xh[i][e];
          ag[e] = __builtin_fmaf(d, xh[i][e], ag[e]);  // fused in every slot (left to contraction, the guarded slot got mul + add)
          ab[e] += d;
        }
        acc[0][wave][c] = ag;
        acc[1][wave][c] = ab;
      }
      __builtin_amdgcn_sched_barrier(0);  // one slot's gamma and f32 dy live at a time
    }
    float c1 = s1, c2 = s2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // the two reductions interleaved
      c1 += __shfl_xor(c1, o, 64);
      c2 += __shfl_xor(c2, o, 64);
    }
    const float k1 = c1 * invD, k2 = c2 * invD;
#pragma unroll
    for (int i = 0; i < kMaxVec; ++i) {
      const int c = lane + 64 * i;
      if (i < kMaxVec - 1 || c < nvec) {  // only the last slot can be ragged: D > 256 * (NV - 1)
        const f32x4 g = gam[c];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rs * ((float)dv[i][e] * g[e] - k1 - xh[i][e] * k2);
        if (kRes) o += dr[i];
        *reinterpret_cast<f32x4*>(dx + row * lddx + 4 * c) = o;
        if (dx_act) store4<TAct>(dx_act + row * (long)D + 4 * c, o);
        acc[2][wave][c] += o;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    row = next;
  }
  // cross-wave reduction of the column partials, then one partial row (or one atomic per column) per block
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kMaxVec; ++i) {
    const int c = lane + 64 * i;
    if (wave < 3 && (i < kMaxVec - 1 || c < nvec)) {
      float* dst = wave == 0 ? dgamma : (wave == 1 ? dbeta : dcolsum);
      if (dst) {
        const f32x4 t = (acc[wave][0][c] + acc[wave][1][c]) + (acc[wave][2][c] + acc[wave][3][c]);
        if (partials) {  // two-stage: plain store of this block's partial row, summed by reduce_partial_rows
          *reinterpret_cast<f32x4*>(partials + ((long)blockIdx.x * 3 + wave) * D + 4 * c) = t;
        } else {         // no workspace: one atomic per column per block (contended when the grid is large)
#pragma unroll
          for (int e = 0; e < 4; ++e) atomicAdd(dst + 4 * c + e, t[e]);
        }
      }
    }
  }
}

// Most workgroups of one ln_bwd_kernel launch; the workspace the caller passes bounds it further.  Another bound is another (still
// deterministic) association of the column sums.
constexpr int kLnBwdBlocks = 1024;
}  // namespace

extern "C" int pm_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, void* y, int out_dtype,
                                float* mean, float* rstd, int M, int D, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !rstd) return PM_EINVAL;
  if (M <= 0 || D <= 0 || D > kMaxD || (D & 3) || (ldx & 3)) return PM_ESHAPE;
  const int grid = (M + 3) / 4 > 4096 ? 4096 : (M + 3) / 4;
#define PM_LN_FWD(TO, NV) \
  hipLaunchKernelGGL((ln_fwd_kernel<TO, NV>), dim3(grid), dim3(256), 0, pm_stream(stream), x, ldx, gamma, beta, (TO*)y, mean, rstd, M, D, eps)
  PM_DISPATCH_ACT(out_dtype, T, {
    if (D <= 1024) PM_LN_FWD(T, 4); else PM_LN_FWD(T, 5);
  });
#undef PM_LN_FWD
  return pm_check_launch();
}

extern "C" int pm_layernorm_bwd(const void* dy, int dy_dtype, const float* x, long ldx, const float* gamma,
                                const float* mean, const float* rstd, const float* dres, long lddres, float* dx,
                                long lddx, void* dx_act, int act_dtype, float* dgamma, float* dbeta, float* dcolsum,
                                int M, int D, void* workspace, size_t ws_bytes, void* stream) {
  if (!dy || !x || !gamma || !mean || !rstd || !dx) return PM_EINVAL;
  if (M <= 0 || D <= 0 || D > kMaxD || (D & 3) || (ldx & 3) || (lddx & 3) || (dres && (lddres & 3))) return PM_ESHAPE;
  if (dx_act && act_dtype != dy_dtype) return PM_EINVAL;
  int cap = 256;  // atomics fallback: keep the number of contending blocks low
  float* partials = nullptr;
  const bool want_sums = dgamma || dbeta || dcolsum;
  if (want_sums && workspace && ws_bytes >= (size_t)64 * 3 * D * sizeof(float)) {
    const size_t fit = ws_bytes / ((size_t)3 * D * sizeof(float));
    cap = kLnBwdBlocks;
    if ((size_t)cap > fit) cap = (int)fit;
    partials = reinterpret_cast<float*>(workspace);
  } else if (!want_sums) {
    cap = kLnBwdBlocks;
  }
  // the parent kernel's grid and row assignment (wave gw of 4 * grid takes rows gw, gw + 4 * grid, ...): with the fixed order inside
  // a wave, a workgroup and reduce_partial_rows, the column sums come out bit for bit as before the rows went in flight
  const int grid = (M + 3) / 4 < cap ? (M + 3) / 4 : cap;
  hipStream_t s = pm_stream(stream);
  const int nv = (D + 255) / 256;  // f32x4 slots per lane: 3 for D = 768, 2 for 512
#define PM_LN_BWD(TD, NV)                                                                                               \
  do {                                                                                                                   \
    auto kern = dres ? ln_bwd_kernel<TD, TD, NV, true> : ln_bwd_kernel<TD, TD, NV, false>;                               \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const TD*)dy, x, ldx, gamma, mean, rstd, dres, lddres, dx, lddx, \
                       (TD*)dx_act, dgamma, dbeta, dcolsum, partials, M, D);                                             \
  } while (0)
  PM_DISPATCH_ACT(dy_dtype, T, {
    if (nv == 1) PM_LN_BWD(T, 1); else if (nv == 2) PM_LN_BWD(T, 2); else if (nv == 3) PM_LN_BWD(T, 3);
    else if (nv == 4) PM_LN_BWD(T, 4); else PM_LN_BWD(T, 5);
  });
#undef PM_LN_BWD
  if (partials)  // dst_v[d] += sum over blocks of partials[b][v][d]
    hipLaunchKernelGGL(reduce_partial_rows<16>, dim3((D + 63) / 64, 3), dim3(1024), 0, s, partials, 3L * D, grid, D, dgamma, dbeta, dcolsum);
  return pm_check_launch();
}
