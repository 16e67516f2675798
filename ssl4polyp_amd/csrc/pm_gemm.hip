// pm_gemm.hip -- MFMA GEMM with fused epilogues for every Linear / conv-as-GEMM of the ViT path and for
// their dgrad / wgrad (reference: timm Attention.qkv/proj, Mlp.fc1/fc2, PatchEmbed.proj, decoder_embed,
// decoder_pred -- models_mae.py:33,39-41,48,53-58; autograd backward engine_pretrain.py:65, tc.py:4533).
//
//   acc[m,n] = sum_k X(m,k) * W(n,k)        X = "A" matrix (M side), W = "B" matrix (N side)
//
// 128x128 kernels -- tile: 128(m) x 128(n) x 128 BYTES of k (64 bf16 / 32 f32) per step, 256 threads = 4 wave64 in 2x2, each
// wave owns 64x64 = 2x2 accumulators of v_mfma_f32_32x32x16_bf16 (or 4x v_mfma_f32_32x32x2_f32 per 16-B
// fragment in f32 mode: exact f32 fma chain).  The W fragment is the MFMA's first operand, so the
// accumulator has n in registers (4 consecutive n per register quad) and m on the lane.
//
// Operand storage (either side independently):
//   k-normal  [R][K]: LDS image 128 rows x 128 B, 16-B chunk c of row r at c ^ ((r>>1)&7)  -> ds_read_b128,
//                     conflict-free for the 32x32x16 operand map (lane (r,h) reads chunk 2*kk+h of row r).
//   k-major   [K][R]: bf16: LDS image 64 k-rows x 256 B, chunk c of row k at c ^ ((k&3)<<2), fragments by
//                     ds_read_b64_tr_b16 (hardware transpose read); f32: 32 k-rows x 512 B, ds_read_b32.
//   -> forward: X k-normal, W k-normal;  dgrad: dY k-normal, W (as stored [out][in]) k-major;
//      wgrad: dY k-major (M side = out features), X k-major (N side = in features).
//
// Three GEMM kernels:
//   gemm_v3_kernel (below, "large-tile path"): the bf16 workhorse of the training step -- 256x256 / 192x256 / 256x128
//     block tiles, 8 waves, 4-slot LDS-DMA ring, ping-pong or software-pipelined k-loop, batched-load / 16-B-store
//     epilogues; forward, dgrad and split-K wgrad of every ViT-B shape go through it.
//   The two 128x128 kernels serve f32 mode and the small / odd shapes, and share LDS images and fragment readers:
//   gemm_glds_kernel (K % k-step == 0): global -> LDS by LDS-DMA (global_load_lds_dwordx4; the LDS
//     image is lane-linear, so the swizzle is applied to each lane's SOURCE address), double buffered, one
//     barrier per k-step, no staging registers and no ds_write; rows beyond M / N are clamped to the last
//     valid row (their results are never stored).  Optional split-K over blockIdx.y writes f32 partial slabs
//     that splitk_reduce_kernel sums in a fixed order (deterministic; used by wgrad where K = #tokens).
//     Epilogue: each wave stages its 64x64 accumulators through LDS and leaves as whole 16-B vectors along n
//     (bias / GELU / dGELU / residual applied on the way out) -> fully coalesced stores.
//   gemm_generic_kernel (any K % chunk == 0): register-staged, fully predicated loads (tiny / odd shapes).
// wgrad_group_kernel runs the ring kernel's tile body over the weight gradients of a whole transformer block in one launch.
//
// Host side: plan_gemm is a pure function of a call's layouts, types, epilogue, shapes, scratch size and pm_gemm_opts; it
// returns the refusal or the kernel family, ring configuration, tile, split-K and tile order (pm_gemm_plan exposes it, so "which
// kernel runs for this Linear" is checked on the CPU: tests/golden/gemm_plan.json).  gemm_dispatch validates the pointers, plans
// and launches what the plan says; pm_gemm_workspace_bytes is the same plan with unlimited scratch.  The ring configurations are
// one table (kRingCfgs) read by the plan and by the launcher: only what the heuristics can choose is instantiated, and
// pm_gemm_opts.variant, the one per-call override, can name nothing else.  No environment variable is read here; the thresholds
// are named constants beside their rules.  The variants that were measured and removed: docs/EXPERIMENT_LOG.md.
// Roofline: MFMA-bound; algorithmic FLOPs 2*M*N*K.
#include "pm_common.h"
#include <type_traits>

namespace {

constexpr int BM = 128, BN = 128, KB = 128;  // KB: bytes of k per row per step
constexpr int TILE_BYTES = 128 * KB;         // 16 KiB per side per buffer
constexpr int kThreads = 256;
constexpr int STAGE_ROW = 64 * 4 + 16;       // epilogue staging: 64 f32 per row + 16 B pad (bank spread)
constexpr int STAGE_BYTES = 64 * STAGE_ROW;  // per wave
constexpr int GLDS_LDS_BYTES = (4 * STAGE_BYTES > 4 * TILE_BYTES) ? 4 * STAGE_BYTES : 4 * TILE_BYTES;

struct GemmArgs {
  const void* X;
  const void* W;
  long ldx, ldw;
  const float* bias;
  void* C;
  long ldc;
  void* aux;
  const float* resid;
  int M, N, K;
  int epilogue;
  int c_dtype;
  int tiles_m, tiles_n;
  int split_k;       // >1: blockIdx.y = split, C = f32 slabs [split][M][ldc]
  int ksteps_split;  // k-steps per split
  float* xsum;         // grouped wgrad: xsum[m] += sum_k X(m, k) (= the bias gradient: column sums of dY), or NULL
  int xsum_store;      // xsum[m] = ... instead of += (partial row sums of a k-slice, reduced later)
  int col_major;       // tile index -> (tm, tn): 0 row by row, 1 column by column (grouped wgrad: see wgrad_group_kernel), >= 2: row by
                       // row inside bands of that many tile columns (wide-N GEMMs: see plan_gemm)
#ifdef PM_GEMM_STAMP
  unsigned long long* stamps;  // diagnostic build only: per-wave cycle sums of the k-loop segments
#endif
};

// Diagnostic build (-DPM_GEMM_STAMP, scratch/stamp_gemm.py): s_memtime stamps around the segments of the ping-pong
// k-loop.  The shipped library never executes a stamp.
#ifdef PM_GEMM_STAMP
#define PM_STAMP(i)                               \
  do {                                            \
    __builtin_amdgcn_sched_barrier(0);            \
    stamp_t[i] = __builtin_readcyclecounter();    \
    __builtin_amdgcn_sched_barrier(0);            \
  } while (0)
#else
#define PM_STAMP(i)
#endif

// ---- global -> register staging (generic kernel) ---------------------------------------------------
template <typename T, bool KMAJOR>
__device__ __forceinline__ void stage_load(u32x4 (&regs)[4], const T* __restrict__ base, long ld, int r0, int R,
                                           int k0, int K, int tid) {
  constexpr int EPC = 16 / sizeof(T);  // elements per chunk
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + kThreads * i;
    u32x4 v = {0u, 0u, 0u, 0u};
    if constexpr (!KMAJOR) {
      const int row = id >> 3, c = id & 7;
      const int gr = r0 + row, gk = k0 + c * EPC;
      if (gr < R && gk < K) v = *reinterpret_cast<const u32x4*>(base + (long)gr * ld + gk);
    } else {
      constexpr int CPR = 128 / EPC;  // chunks per k-row (16 bf16 / 32 f32)
      const int krow = id / CPR, c = id % CPR;
      const int gk = k0 + krow, gr = r0 + c * EPC;
      if (gk < K && gr < R) v = *reinterpret_cast<const u32x4*>(base + (long)gk * ld + gr);
    }
    regs[i] = v;
  }
}

template <typename T, bool KMAJOR>
__device__ __forceinline__ void stage_store(const u32x4 (&regs)[4], char* tile, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + kThreads * i;
    int off;
    if constexpr (!KMAJOR) {
      const int row = id >> 3, c = id & 7;
      off = row * 128 + 16 * (c ^ ((row >> 1) & 7));
    } else if constexpr (sizeof(T) == 2) {
      const int krow = id >> 4, c = id & 15;
      off = krow * 256 + 16 * (c ^ ((krow & 3) << 2));
    } else {
      off = id * 16;  // [32 k][128 r] f32, linear
    }
    *reinterpret_cast<u32x4*>(tile + off) = regs[i];
  }
}

// ---- global -> LDS by LDS-DMA (fast kernel) -------------------------------------------------------
// One side's 16-KiB tile = 16 wave-instructions of 1 KiB (lane l lands at tile + 1024*j + 16*l); wave w issues
// j = w, w+4, w+8, w+12.  The lane's SOURCE chunk is the inverse swizzle of its landing slot.
__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <typename T, bool KMAJOR>
__device__ __forceinline__ void stage_glds(char* tile, const T* __restrict__ base, long ld, int r0, int R, int k0,
                                           int wave, int lane) {
  constexpr int EPC = 16 / sizeof(T);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = wave + 4 * i;
    const T* src;
    if constexpr (!KMAJOR) {
      const int row = 8 * j + (lane >> 3), cs = lane & 7;
      const int c = cs ^ ((row >> 1) & 7);
      int gr = r0 + row;
      gr = gr < R ? gr : R - 1;  // clamp: rows beyond R feed outputs that are never stored
      src = base + (long)gr * ld + k0 + c * EPC;
    } else if constexpr (sizeof(T) == 2) {
      const int krow = 4 * j + (lane >> 4), cs = lane & 15;
      const int c = cs ^ ((krow & 3) << 2);
      int gc = r0 + c * EPC;
      gc = gc < R ? gc : R - EPC;
      src = base + (long)(k0 + krow) * ld + gc;
    } else {
      const int krow = 2 * j + (lane >> 5), c = lane & 31;
      int gc = r0 + c * EPC;
      gc = gc < R ? gc : R - EPC;
      src = base + (long)(k0 + krow) * ld + gc;
    }
    glds16(src, tile + 1024 * j);
  }
}

// ---- LDS -> MFMA operand fragment -----------------------------------------------------------
template <typename T, bool KMAJOR>
__device__ __forceinline__ Frag16 read_frag(const char* PM_LDS_IMAGE tile, int rb, int kk, int lane) {
  Frag16 f;
  if constexpr (!KMAJOR) {
    const int row = rb + (lane & 31);
    const int c = 2 * kk + (lane >> 5);
    f.u = *reinterpret_cast<const u32x4*>(tile + row * 128 + 16 * (c ^ ((row >> 1) & 7)));
  } else if constexpr (sizeof(T) == 2) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int ch = (rb >> 3) + 2 * (g & 1) + (p >> 1);
    const int sw = 16 * (ch ^ (q << 2)) + 8 * (p & 1);
    const int kbase = kk * 16 + 8 * (g >> 1) + q;
    using lds_s4 = __attribute__((address_space(3))) short4v;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(tile + kbase * 256 + sw));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(tile + (kbase + 4) * 256 + sw));
    f.u[0] = ((unsigned)(unsigned short)lo[0]) | (((unsigned)(unsigned short)lo[1]) << 16);
    f.u[1] = ((unsigned)(unsigned short)lo[2]) | (((unsigned)(unsigned short)lo[3]) << 16);
    f.u[2] = ((unsigned)(unsigned short)hi[0]) | (((unsigned)(unsigned short)hi[1]) << 16);
    f.u[3] = ((unsigned)(unsigned short)hi[2]) | (((unsigned)(unsigned short)hi[3]) << 16);
  } else {
    const int r = rb + (lane & 31), h = lane >> 5;
#pragma unroll
    for (int e = 0; e < 4; ++e) f.f[e] = *reinterpret_cast<const float*>(tile + (8 * kk + 4 * h + e) * 512 + 4 * r);
  }
  return f;
}

template <typename T, bool XK, bool WK>
__device__ __forceinline__ void mma_kstep(const char* bx, const char* bw, int wm, int wn, int lane, f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    Frag16 fw[2], fx[2];
    fw[0] = read_frag<T, WK>(bw, wn * 64, kk, lane);
    fw[1] = read_frag<T, WK>(bw, wn * 64 + 32, kk, lane);
    fx[0] = read_frag<T, XK>(bx, wm * 64, kk, lane);
    fx[1] = read_frag<T, XK>(bx, wm * 64 + 32, kk, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = mfma16B<T>(fw[i], fx[j], acc[i][j]);
  }
}

// XCD-aware tile order: the 8 XCDs take blocks round-robin; give each XCD a contiguous run of tiles so
// that neighbours (same X panel, consecutive W panels) hit the same private L2.  Bijective for any grid.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + (bid >> 3);
}

// Epilogue on 4 consecutive n of row m (v = acc + bias already applied by the caller where relevant).
template <typename T>
__device__ __forceinline__ void epilogue4(const GemmArgs& a, int epi, long off, f32x4 v) {
  if (epi == PM_EPI_RESIDUAL) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(a.resid + off);
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.C) + off) = r + v;
  } else if (epi == PM_EPI_ACCUM) {
    float* c = reinterpret_cast<float*>(a.C) + off;
    *reinterpret_cast<f32x4*>(c) = *reinterpret_cast<const f32x4*>(c) + v;
  } else {
    if (epi == PM_EPI_GELU) {
      if (a.aux) store4<T>(reinterpret_cast<T*>(a.aux) + off, v);   // (no aux: nobody will run a backward through this Linear)
      v = gelu_act4<T>(round_through<T>(v));  // gelu of the value backward will see
    } else if (epi == PM_EPI_DGELU) {
      const f32x4 pre = load4<T>(reinterpret_cast<const T*>(a.aux) + off);
      v *= gelu_act_grad4<T>(pre);
    }
    if (a.c_dtype == PM_F32) {
      store4<float>(reinterpret_cast<float*>(a.C) + off, v);
    } else if constexpr (sizeof(T) == 2) {
      store4<T>(reinterpret_cast<T*>(a.C) + off, v);  // (a 16-bit C has the operands' type: checked by the dispatcher)
    } else {
      if (a.c_dtype == PM_F16) store4<_Float16>(reinterpret_cast<_Float16*>(a.C) + off, v);
      else store4<__bf16>(reinterpret_cast<__bf16*>(a.C) + off, v);
    }
  }
}

// The same epilogues on NV vectors at once: every load the epilogue needs (residual / saved pre-activation / C) is
// issued before the first store, so the loads overlap instead of forming one load -> store latency chain per vector
// (stamped on the 256x256 tile: 25.6k cycles per wave for 32 dependent chains).  off[] must be valid addresses (the
// caller clamps rows / columns beyond M / N); ok[] gates the stores.
template <typename E, int NV>
__device__ __forceinline__ void epilogue_batch(const GemmArgs& a, int epi, const long (&off)[NV], const bool (&ok)[NV],
                                               f32x4 (&v)[NV]) {
  if (epi == PM_EPI_RESIDUAL || epi == PM_EPI_ACCUM) {
    const float* src = epi == PM_EPI_RESIDUAL ? a.resid : reinterpret_cast<const float*>(a.C);
    f32x4 r[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) r[e] = *reinterpret_cast<const f32x4*>(src + off[e]);
#pragma unroll
    for (int e = 0; e < NV; ++e)
      if (ok[e]) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.C) + off[e]) = r[e] + v[e];
    return;
  }
  if (epi == PM_EPI_DGELU) {
    f32x4 pre[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) pre[e] = load4<E>(reinterpret_cast<const E*>(a.aux) + off[e]);
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] *= gelu_act_grad4<E>(pre[e]);
  } else if (epi == PM_EPI_GELU) {
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      if (a.aux && ok[e]) store4<E>(reinterpret_cast<E*>(a.aux) + off[e], v[e]);
      v[e] = gelu_act4<E>(round_through<E>(v[e]));  // what backward will see
    }
  }
  if (a.c_dtype == PM_F32) {
#pragma unroll
    for (int e = 0; e < NV; ++e)
      if (ok[e]) store4<float>(reinterpret_cast<float*>(a.C) + off[e], v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < NV; ++e)
      if (ok[e]) store4<E>(reinterpret_cast<E*>(a.C) + off[e], v[e]);
  }
}

// 8 consecutive n per vector, act-typed (16-bit) C, epilogues STORE / GELU / DGELU: 16-B accesses.
template <typename E, int NV>
__device__ __forceinline__ void epilogue_batch8(const GemmArgs& a, int epi, const long (&off)[NV], const bool (&ok)[NV],
                                                f32x4 (&lo)[NV], f32x4 (&hi)[NV]) {
  if (epi == PM_EPI_DGELU) {
    f32x4 plo[NV], phi[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) load8_16<E>(reinterpret_cast<const E*>(a.aux) + off[u], plo[u], phi[u]);
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      lo[u] *= gelu_act_grad4<E>(plo[u]);
      hi[u] *= gelu_act_grad4<E>(phi[u]);
    }
  } else if (epi == PM_EPI_GELU) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (a.aux && ok[u]) store8_16<E>(reinterpret_cast<E*>(a.aux) + off[u], lo[u], hi[u]);
      lo[u] = gelu_act4<E>(round_through<E>(lo[u]));  // gelu of the value backward will see (the rounded pre-activation)
      hi[u] = gelu_act4<E>(round_through<E>(hi[u]));
    }
  }
#pragma unroll
  for (int u = 0; u < NV; ++u)
    if (ok[u]) store8_16<E>(reinterpret_cast<E*>(a.C) + off[u], lo[u], hi[u]);
}

// exchange between lane l and lane l+32: afterwards the low half-wave holds (x of lane l, x of lane l+32) in (x, y)
// and the high half-wave holds (y of lane l-32, y of its own) -- v_permlane32_swap
__device__ __forceinline__ void swap_halves(float& x, float& y) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  const u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  y = __uint_as_float(r[1]);
}

// ------------------------------------------------------------------------------------------------
// fast path
// ------------------------------------------------------------------------------------------------
template <typename T, bool XK, bool WK>
__global__ __launch_bounds__(kThreads, 2) void gemm_glds_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][X tile | W tile]; reused for staging
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = tile / a.tiles_n, tn = tile % a.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  constexpr int KE = KB / sizeof(T);  // k elements per step
  const int nk_total = a.K / KE;
  const int kbeg = blockIdx.y * a.ksteps_split;
  const int kend = (kbeg + a.ksteps_split) < nk_total ? (kbeg + a.ksteps_split) : nk_total;
  const T* X = reinterpret_cast<const T*>(a.X);
  const T* W = reinterpret_cast<const T*>(a.W);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (kbeg < kend) {
    stage_glds<T, XK>(smem, X, a.ldx, m0, a.M, kbeg * KE, wave, lane);
    stage_glds<T, WK>(smem + TILE_BYTES, W, a.ldw, n0, a.N, kbeg * KE, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = kbeg; t < kend; ++t) {
      const int cur = (t - kbeg) & 1;
      const char* bx = smem + cur * 2 * TILE_BYTES;
      if (t + 1 < kend) {
        char* nb = smem + (cur ^ 1) * 2 * TILE_BYTES;
        stage_glds<T, XK>(nb, X, a.ldx, m0, a.M, (t + 1) * KE, wave, lane);
        stage_glds<T, WK>(nb + TILE_BYTES, W, a.ldw, n0, a.N, (t + 1) * KE, wave, lane);
      }
      mma_kstep<T, XK, WK>(bx, bx + TILE_BYTES, wm, wn, lane, acc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // ---- epilogue: stage this wave's 64(m) x 64(n) accumulators through LDS, leave as 16-B vectors along n ----
  char* st = smem + wave * STAGE_BYTES;  // all waves are past the last barrier: tiles are dead
  const int h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ml = j * 32 + (lane & 31);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        *reinterpret_cast<f32x4*>(st + ml * STAGE_ROW + (i * 32 + 8 * g + 4 * h) * 4) = v;
      }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's own LDS writes
  __builtin_amdgcn_wave_barrier();
  const bool split = a.split_k > 1;
  const int epi = split ? PM_EPI_STORE : a.epilogue;
  float* slab = split ? reinterpret_cast<float*>(a.C) + (long)blockIdx.y * a.M * a.ldc : nullptr;
  const int mw = m0 + wm * 64, nw = n0 + wn * 64;
  if (!split && (sizeof(T) == 2 || a.c_dtype == PM_F32)) {  // (f32 operands with a 16-bit C: the per-vector path below)
    // every load the epilogue needs for the wave's 64 x 64 tile (f32 residual / C, or the saved pre-activation) is issued before the
    // first store: one exposed trip to memory per tile instead of sixteen load -> store chains (the compiler cannot hoist a load over
    // a store that may alias it).  Clamped addresses for rows / columns beyond M / N, the stores are gated.
    const int c4 = (lane & 15) * 4, n = nw + c4;
    const bool nok = n < a.N;
    const long ncl = nok ? n : a.N - 4;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + ncl);
    long off[16];
    bool ok[16];
    f32x4 v[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int ml = it * 4 + (lane >> 4), m = mw + ml;
      ok[it] = m < a.M && nok;
      off[it] = (long)(m < a.M ? m : a.M - 1) * a.ldc + ncl;
      v[it] = *reinterpret_cast<const f32x4*>(st + ml * STAGE_ROW + c4 * 4) + bv;
    }
    epilogue_batch<T, 16>(a, epi, off, ok, v);
    return;
  }
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int ml = it * 4 + (lane >> 4), c4 = (lane & 15) * 4;
    const int m = mw + ml, n = nw + c4;
    if (m >= a.M || n >= a.N) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(st + ml * STAGE_ROW + c4 * 4);
    const long off = (long)m * a.ldc + n;
    if (split) {
      *reinterpret_cast<f32x4*>(slab + off) = v;
      continue;
    }
    if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + n);
    epilogue4<T>(a, epi, off, v);
  }
}

// out[m][n] = (accumulate ? out : 0) + sum_s slab[s][m][n], fixed order (deterministic)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out,
                                                            long ldc, int M, int N, int splits, int accumulate) {
  const long nvec = (long)M * (N >> 2);
  const long slab_stride = (long)M * ldc;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const int m = i / (N >> 2), n = (i % (N >> 2)) * 4;
    const long off = (long)m * ldc + n;
    f32x4 v = accumulate ? *reinterpret_cast<const f32x4*>(out + off) : (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) v += *reinterpret_cast<const f32x4*>(slabs + s * slab_stride + off);
    *reinterpret_cast<f32x4*>(out + off) = v;
  }
}

// ------------------------------------------------------------------------------------------------
// generic path (predicated, register staged)
// ------------------------------------------------------------------------------------------------
template <typename T, bool XK, bool WK>
__global__ __launch_bounds__(kThreads, 2) void gemm_generic_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][X tile | W tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = tile / a.tiles_n, tn = tile % a.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  constexpr int KE = KB / sizeof(T);  // k elements per step
  const int nk = (a.K + KE - 1) / KE;
  const T* X = reinterpret_cast<const T*>(a.X);
  const T* W = reinterpret_cast<const T*>(a.W);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  u32x4 rx[4], rw[4];
  stage_load<T, XK>(rx, X, a.ldx, m0, a.M, 0, a.K, tid);
  stage_load<T, WK>(rw, W, a.ldw, n0, a.N, 0, a.K, tid);
  stage_store<T, XK>(rx, smem, tid);
  stage_store<T, WK>(rw, smem + TILE_BYTES, tid);
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    const char* bx = smem + (t & 1) * 2 * TILE_BYTES;
    const bool more = (t + 1) < nk;
    if (more) {
      stage_load<T, XK>(rx, X, a.ldx, m0, a.M, (t + 1) * KE, a.K, tid);
      stage_load<T, WK>(rw, W, a.ldw, n0, a.N, (t + 1) * KE, a.K, tid);
    }
    mma_kstep<T, XK, WK>(bx, bx + TILE_BYTES, wm, wn, lane, acc);
    if (more) {
      char* nb = smem + ((t + 1) & 1) * 2 * TILE_BYTES;
      stage_store<T, XK>(rx, nb, tid);
      stage_store<T, WK>(rw, nb + TILE_BYTES, tid);
    }
    __syncthreads();
  }

  // ---- epilogue straight from registers: lane = row m, register quad = 4 consecutive n ----
  const int h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm * 64 + j * 32 + (lane & 31);
    if (m >= a.M) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + i * 32 + 8 * g + 4 * h;
        if (n >= a.N) continue;
        f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + n);
        epilogue4<T>(a, a.epilogue, (long)m * a.ldc + n, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// large-tile path (bf16, X k-normal): BM x BN block tile, 8 waves, 4-stage LDS-DMA ring
// ------------------------------------------------------------------------------------------------
// Why: with 128x128 tiles every k-step moves 32 KiB into LDS for 2.1 MFLOP (64 FLOP/B) and has only ONE stage
// of prefetch, so a k-step can never be shorter than the global->LDS round trip.  Here a block owns 256x256
// (or 256x128) outputs = 128 FLOP/B, a k-step is 32 elements (64-B rows: 4 chunks, XOR-swizzled by (row>>2)&3),
// and 4 ring slots keep 3 stages (96 KiB / CU) in flight behind a COUNTED s_waitcnt vmcnt(N) and a raw
// s_barrier (one per k-step): the DMA of stages t+1, t+2 overlaps the MFMAs of stage t.
// 8 waves in WM x WN = 2 x 4 (256-wide tiles) or 4 x 2 (128-wide); per-wave tile (BM/WM) x (BN/WN) = 128x64, 96x64 (192-row
// tiles) or 64x64 (256x128): 12 / 8 ds_read_b128 per 16 / 8 MFMAs per k-step.
constexpr int V3_STAGES = 4;                 // ring slots
constexpr int V3_KE = 32;                    // bf16 elements of k per stage
constexpr int V3_STAGE_WAVE = 64 * STAGE_ROW;  // epilogue staging per wave (64 rows x 64 f32, padded)

constexpr int V3_WAVES = 8;                  // waves per workgroup: two per SIMD

// One 1-KiB LDS-DMA piece j of a k-normal tile (16 rows x 64 B; the lane's SOURCE chunk is the inverse swizzle of its slot:
// 16-B chunk c of row r sits at c ^ ((r >> 2) & 3), conflict-free for the 32x32x16 operand read of v3_frag_kn).
__device__ __forceinline__ void v3_piece_kn(char* tile, const __bf16* __restrict__ base, long ld, int r0, int R, int k0,
                                            int j, int lane) {
  const int row = 16 * j + (lane >> 2), cs = lane & 3;
  const int c = cs ^ ((row >> 2) & 3);
  int gr = r0 + row;
  gr = gr < R ? gr : R - 1;
  glds16(base + (long)gr * ld + k0 + c * 8, tile + 1024 * j);
}

template <int ROWS>
__device__ __forceinline__ void v3_stage_kn(char* tile, const __bf16* __restrict__ base, long ld, int r0, int R, int k0,
                                            int wave, int lane) {
  constexpr int TI = ROWS * 64 / 1024;  // wave-instructions for the tile, dealt round-robin to the waves
#pragma unroll
  for (int i = 0; i < (TI + V3_WAVES - 1) / V3_WAVES; ++i) {
    const int j = wave + V3_WAVES * i;
    if (j >= TI) break;  // (192-row tiles: waves 4-7 issue one instruction less)
    v3_piece_kn(tile, base, ld, r0, R, k0, j, lane);
  }
}

// One piece j of a k-major tile (COLS columns: 1024 / (2 COLS) k-rows per piece).
template <int COLS>
__device__ __forceinline__ void v3_piece_km(char* tile, const __bf16* __restrict__ base, long ld, int r0, int R, int k0,
                                            int j, int lane) {
  constexpr int RB = COLS * 2;         // bytes per k-row
  constexpr int KPI = 1024 / RB;       // k-rows per wave-instruction (2 or 4)
  constexpr int CPR = RB / 16;         // chunks per k-row
  const int krow = KPI * j + lane / CPR, cs = lane % CPR;
  const int c = cs ^ ((krow & 3) << 2);
  int gc = r0 + c * 8;
  gc = gc < R ? gc : R - 8;
  glds16(base + (long)(k0 + krow) * ld + gc, tile + 1024 * j);
}

template <int COLS>
__device__ __forceinline__ void v3_stage_km(char* tile, const __bf16* __restrict__ base, long ld, int r0, int R, int k0,
                                            int wave, int lane) {
  constexpr int NI = 32 * COLS * 2 / 1024 / V3_WAVES;
#pragma unroll
  for (int i = 0; i < NI; ++i) v3_piece_km<COLS>(tile, base, ld, r0, R, k0, wave + V3_WAVES * i, lane);
}

__device__ __forceinline__ Frag16 v3_frag_kn(const char* tile, int rb, int kk, int lane) {
  const int row = rb + (lane & 31);
  const int c = 2 * kk + (lane >> 5);
  Frag16 f;
  f.u = *reinterpret_cast<const u32x4*>(tile + row * 64 + 16 * (c ^ ((row >> 2) & 3)));
  return f;
}

template <int RB>
__device__ __forceinline__ Frag16 v3_frag_km(const char* PM_LDS_IMAGE tile, int rb, int kk, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int ch = (rb >> 3) + 2 * (g & 1) + (p >> 1);
  const int sw = 16 * (ch ^ (q << 2)) + 8 * (p & 1);
  const int kbase = kk * 16 + 8 * (g >> 1) + q;
  using lds_s4 = __attribute__((address_space(3))) short4v;
  const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(tile + kbase * RB + sw));
  const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(tile + (kbase + 4) * RB + sw));
  Frag16 f;
  f.u[0] = ((unsigned)(unsigned short)lo[0]) | (((unsigned)(unsigned short)lo[1]) << 16);
  f.u[1] = ((unsigned)(unsigned short)lo[2]) | (((unsigned)(unsigned short)lo[3]) << 16);
  f.u[2] = ((unsigned)(unsigned short)hi[0]) | (((unsigned)(unsigned short)hi[1]) << 16);
  f.u[3] = ((unsigned)(unsigned short)hi[2]) | (((unsigned)(unsigned short)hi[3]) << 16);
  return f;
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
  else static_assert(N == 0, "add the immediate");
}

// One block = one BM_ x BN_ output tile (`tile` = row-major tile index, `split_idx` = k-slice for split-K).  The body of
// gemm_v3_kernel (one GEMM per launch) and of wgrad_group_kernel (the weight gradients of a whole transformer block in
// one launch, full-K tiles).
// PP: the ping-pong k-loop; otherwise the software-pipelined one.  DIRECT: the epilogue leaves straight from the accumulator
// registers; otherwise staged through LDS.  XK / WK: that operand is k-major.  XSUM: row sums of X beside the GEMM.
template <int BM_, int BN_, bool WK, bool DIRECT, bool PP, bool XK, bool XSUM, typename E>
__device__ __forceinline__ void gemm_v3_tile(GemmArgs& a, const int tile, const int split_idx) {
  constexpr int STAGES = V3_STAGES, NW = V3_WAVES;
  constexpr int WN = BN_ / 64, WM = NW / WN;       // wave grid
  constexpr int TM = BM_ / WM, TN = BN_ / WN;      // per-wave tile
  constexpr int MT = TM / 32, NTL = TN / 32;       // 32x32 accumulators per wave
  constexpr int XB = BM_ * 64, WB = BN_ * 64;      // bytes per stage per side
  constexpr int SB = XB + WB;
  constexpr int G = (SB / 1024 + NW - 1) / NW;     // LDS-DMA instructions per wave per stage (max over waves)
  static_assert((WB % (1024 * NW)) == 0 && ((XB % (1024 * NW)) == 0 || (!XK && XB == 12288 && DIRECT)),
                "whole wave-instructions per wave, except the 192-row k-normal X tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
#ifdef PM_GEMM_STAMP
  const unsigned long long stamp_entry = __builtin_readcyclecounter();
  const unsigned long long stamp_entry_rt = __builtin_amdgcn_s_memrealtime();  // 100 MHz: clock = d(cycles) / d(realtime) x 100 MHz
  unsigned long long stamp_loop_end = 0, stamp_loop_end_rt = 0;
  auto stamp_finish = [&]() {
    const unsigned long long t_issued = __builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t_acked = __builtin_readcyclecounter();
    if (a.stamps && lane == 0 && blockIdx.y == 0) {
      unsigned long long* o = a.stamps + ((long)blockIdx.x * NW + wave) * 16;
      o[8] = stamp_entry; o[9] = stamp_loop_end; o[10] = t_issued; o[11] = t_acked;
      o[12] = stamp_entry_rt; o[13] = stamp_loop_end_rt;
    }
  };
#endif
  int tm, tn;
  if (a.col_major >= 2) {  // bands of col_major tile columns, row by row inside a band (the last band may be narrower)
    const int per_band = a.tiles_m * a.col_major;
    const int band = tile / per_band, r = tile - band * per_band;
    const int left = a.tiles_n - band * a.col_major;
    const int bw = left < a.col_major ? left : a.col_major;
    tm = r / bw;
    tn = band * a.col_major + (r - tm * bw);
  } else {
    tm = a.col_major ? tile % a.tiles_m : tile / a.tiles_n;
    tn = a.col_major ? tile / a.tiles_m : tile % a.tiles_n;
  }
  const int m0 = tm * BM_, n0 = tn * BN_;
  const __bf16* X = reinterpret_cast<const __bf16*>(a.X);
  const __bf16* W = reinterpret_cast<const __bf16*>(a.W);
  int nk = a.K / V3_KE;
  if (a.split_k > 1) {  // split-K: this block owns k-steps [kbeg, kend) and writes an f32 partial slab
    const int kbeg = split_idx * a.ksteps_split;
    const int kend = (kbeg + a.ksteps_split) < nk ? (kbeg + a.ksteps_split) : nk;
    nk = kend - kbeg;
    X += XK ? (long)kbeg * V3_KE * a.ldx : (long)kbeg * V3_KE;
    W += WK ? (long)kbeg * V3_KE * a.ldw : (long)kbeg * V3_KE;
    a.C = reinterpret_cast<float*>(a.C) + (long)split_idx * a.M * a.ldc;
  }

  f32x16 acc[NTL][MT];
#pragma unroll
  for (int i = 0; i < NTL; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Row sums of the X operand beside the GEMM (grouped weight gradients: X = dY^T, so xsum = the Linear's bias gradient).
  // The 32x32x16 X fragment (lane l: row l&31, k-half l>>5) is fed as the B operand of a 16x16x32 MFMA, which reads it as
  // column l&15, k-group l>>4: rows r and r+16 of the fragment fall on the same column in k-groups {0,2} / {1,3}.  An A
  // operand that is all ones in row 0 for k-groups {0,2} and in row 1 for k-groups {1,3} (lanes 0, 32 / 17, 49) therefore
  // yields D[0][c] = sum_k X[c][k], D[1][c] = sum_k X[16+c][k]: lane c < 16 holds them in registers 0 and 1.
  // 2*MT extra 16-cycle MFMAs per k-step, only in the waves of column 0 of the tiles of column 0 (each row once).
  static_assert(!XSUM || XK, "row sums ride on the k-major X fragments");
  f32x4 xs[MT];
  Frag16 ones_sel;
  bool do_xsum = false;
  if constexpr (XSUM) {
    do_xsum = a.xsum != nullptr && tn == 0 && wn == 0;
    const bool one = lane == 0 || lane == 32 || lane == 17 || lane == 49;
    const unsigned v = one ? ones2<E>() : 0u;  // two 1.0 of the operand type
    ones_sel.u = u32x4{v, v, v, v};
#pragma unroll
    for (int j = 0; j < MT; ++j) xs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto issue = [&](int t) {
    char* buf = smem + (t % STAGES) * SB;
    if constexpr (XK) v3_stage_km<BM_>(buf, X, a.ldx, m0, a.M, t * V3_KE, wave, lane);
    else v3_stage_kn<BM_>(buf, X, a.ldx, m0, a.M, t * V3_KE, wave, lane);
    if constexpr (WK) v3_stage_km<BN_>(buf + XB, W, a.ldw, n0, a.N, t * V3_KE, wave, lane);
    else v3_stage_kn<BN_>(buf + XB, W, a.ldw, n0, a.N, t * V3_KE, wave, lane);
  };
  auto read_frags = [&](int t, Frag16 (&fw)[2][NTL], Frag16 (&fx)[2][MT]) {
    const char* bx = smem + (t % STAGES) * SB;
    const char* bw = bx + XB;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < NTL; ++i) {
        if constexpr (WK) fw[kk][i] = v3_frag_km<BN_ * 2>(bw, wn * TN + 32 * i, kk, lane);
        else fw[kk][i] = v3_frag_kn(bw, wn * TN + 32 * i, kk, lane);
      }
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        if constexpr (XK) fx[kk][j] = v3_frag_km<BM_ * 2>(bx, wm * TM + 32 * j, kk, lane);
        else fx[kk][j] = v3_frag_kn(bx, wm * TM + 32 * j, kk, lane);
      }
    }
  };
  auto mma_all = [&](const Frag16 (&fw)[2][NTL], const Frag16 (&fx)[2][MT]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          acc[i][j] = mfma16B<E>(fw[kk][i], fx[kk][j], acc[i][j]);
    if constexpr (XSUM) {
      if (do_xsum) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < MT; ++j)
            xs[j] = mfma16x16<E>(ones_sel, fx[kk][j], xs[j]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  if constexpr (!PP) {
    // Software-pipelined loop, one barrier per k-step.  Iteration t runs the MFMAs of stage t on fragments that were
    // read from LDS during iteration t-1, and between those MFMAs issues (a) the fragment reads of stage t+1 into the
    // other register set and (b) this wave's LDS-DMA pieces of stage t+3 into the slot of stage t-1 (every wave
    // consumed its stage-(t-1) fragments before it reached this iteration's barrier).  LDS reads and DMA issue cost
    // far less in the shadow of the wave's own MFMAs than in a phase of their own (stamped: 12 ds_read_b128 276 cyc,
    // 4 pieces 416 cyc in the ping-pong read phase), and the SIMD's two waves cover each other's remaining stalls.
    // Ring of 4 slots: the pieces of stage t+3 go into the slot of stage t-1; stage t+2 may still be in flight at the
    // barrier of iteration t.
    constexpr int AHEAD = STAGES - 1;   // issue distance
    constexpr int TIX = XB / 1024, TIW = WB / 1024;         // DMA pieces per side per stage
    constexpr int GX = (TIX + NW - 1) / NW, GW = TIW / NW;  // per wave (GX: max over waves)
    constexpr int NR = 2 * (NTL + MT), NMF = 2 * NTL * MT;  // fragment reads / MFMAs per k-step
    constexpr int PER = NMF / (GX + GW);                    // one DMA piece every PER MFMAs
    static_assert(GX + GW == G && NR <= NMF && PER >= 2, "interleave plan");
    constexpr bool UNEVEN = (TIX % NW) != 0;
    const int gq = wave >> 2;
    auto wait_stages = [&](auto n) {  // all but the n youngest stages of this wave's pieces have landed
      constexpr int N = decltype(n)::value;
      if constexpr (UNEVEN) {
        if (gq == 0) wait_vmcnt<N * G>(); else wait_vmcnt<N * (G - 1)>();
      } else {
        wait_vmcnt<N * G>();
      }
    };
    auto piece = [&](int t, int p) {
      char* buf = smem + (t % STAGES) * SB;
      const int k0 = t * V3_KE;
      if (p < GX) {
        const int j = wave + NW * p;
        if (UNEVEN && j >= TIX) return;
        if constexpr (XK) v3_piece_km<BM_>(buf, X, a.ldx, m0, a.M, k0, j, lane);
        else v3_piece_kn(buf, X, a.ldx, m0, a.M, k0, j, lane);
      } else {
        const int j = wave + NW * (p - GX);
        if constexpr (WK) v3_piece_km<BN_>(buf + XB, W, a.ldw, n0, a.N, k0, j, lane);
        else v3_piece_kn(buf + XB, W, a.ldw, n0, a.N, k0, j, lane);
      }
    };
    auto read_one = [&](int t, int q, Frag16 (&fw)[2][NTL], Frag16 (&fx)[2][MT]) {
      const char* bx = smem + (t % STAGES) * SB;
      const char* bw = bx + XB;
      const int kk = q / (NTL + MT), r = q % (NTL + MT);
      if (r < NTL) {
        if constexpr (WK) fw[kk][r] = v3_frag_km<BN_ * 2>(bw, wn * TN + 32 * r, kk, lane);
        else fw[kk][r] = v3_frag_kn(bw, wn * TN + 32 * r, kk, lane);
      } else {
        if constexpr (XK) fx[kk][r - NTL] = v3_frag_km<BM_ * 2>(bx, wm * TM + 32 * (r - NTL), kk, lane);
        else fx[kk][r - NTL] = v3_frag_kn(bx, wm * TM + 32 * (r - NTL), kk, lane);
      }
    };
#ifdef PM_GEMM_STAMP
    unsigned long long stamp_t[8], stamp_acc[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
    // FULL: stages t+1 and t+3 exist (steady state, no branches in the MFMA stream)
    auto step =[&](auto full, int t, const Frag16 (&cw)[2][NTL], const Frag16 (&cx)[2][MT], Frag16 (&nw)[2][NTL],
                    Frag16 (&nx)[2][MT]) {
      constexpr bool FULL = decltype(full)::value;
      PM_STAMP(0);
      __builtin_amdgcn_sched_barrier(0);
      if (FULL || t + 2 < nk) wait_stages(std::integral_constant<int, 1>{});  // stage t+1 landed, stage t+2 may fly
      else wait_vmcnt<0>();
      PM_STAMP(1);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      PM_STAMP(2);
      const bool rd = FULL || t + 1 < nk, ld = FULL || t + AHEAD < nk;
#pragma unroll
      for (int m = 0; m < NMF; ++m) {
        const int kk = m / (NTL * MT), i = (m / MT) % NTL, j = m % MT;
        acc[i][j] = mfma16B<E>(cw[kk][i], cx[kk][j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (m < NR && rd) read_one(t + 1, m, nw, nx);
        if ((m % PER) == 1 && m / PER < G && ld) piece(t + AHEAD, m / PER);
        __builtin_amdgcn_sched_barrier(0);
#ifdef PM_GEMM_STAMP
        if (m == NMF / 2 - 1) PM_STAMP(3);
#endif
      }
      if constexpr (XSUM) {
        if (do_xsum) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < MT; ++j)
              xs[j] = mfma16x16<E>(ones_sel, cx[kk][j], xs[j]);
        }
      }
#ifdef PM_GEMM_STAMP
      PM_STAMP(4);
#pragma unroll
      for (int i = 0; i < 4; ++i) stamp_acc[i] += stamp_t[i + 1] - stamp_t[i];
#endif
    };
#pragma unroll
    for (int t = 0; t < AHEAD; ++t)
      if (t < nk) issue(t);
    if (nk > 2) wait_stages(std::integral_constant<int, 2>{});
    else if (nk > 1) wait_stages(std::integral_constant<int, 1>{});
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    Frag16 fwA[2][NTL], fxA[2][MT], fwB[2][NTL], fxB[2][MT];
    read_frags(0, fwA, fxA);
    __builtin_amdgcn_sched_barrier(0);
    int t = 0;
    for (; t + 1 + AHEAD < nk; t += 2) {
      step(std::true_type{}, t, fwA, fxA, fwB, fxB);
      step(std::true_type{}, t + 1, fwB, fxB, fwA, fxA);
    }
    for (; t < nk; t += 2) {
      step(std::false_type{}, t, fwA, fxA, fwB, fxB);
      if (t + 1 < nk) step(std::false_type{}, t + 1, fwB, fxB, fwA, fxA);
    }
#ifdef PM_GEMM_STAMP
    if (a.stamps && lane == 0 && blockIdx.y == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) a.stamps[((long)blockIdx.x * NW + wave) * 16 + i] = stamp_acc[i];
      a.stamps[((long)blockIdx.x * NW + wave) * 16 + 7] = nk;
    }
#endif
  } else {
    // Ping-pong: waves 0-3 and 4-7 (SIMD partners: wave w and w+4 share a SIMD) run the same two-phase loop
    //   R_t: 12 LDS fragment reads of stage t + LDS-DMA refill      M_t: 16 back-to-back MFMAs
    // one phase apart (waves 4-7 pass one extra barrier first), so on every SIMD one wave's MFMA phase runs
    // beside its partner's read / DMA-issue phase instead of both stalling on LDS latency together.
    // Ring: DP = 2 stages in flight; R_t refills the slot of stage t-2, which both halves finished reading
    // (and waited lgkmcnt(0) on) at least two barriers ago.  Stage readiness: every wave waits for its own DMA share
    // of stage t+1 before the barrier that opens its M_t -- for the lagging half that barrier is the one that opens
    // the leading half's R_{t+1}.
    // (Issuing the refill, or half of it, between the MFMAs of M_t instead was measured neutral to slightly worse:
    // the stamped read phase shrinks from 810 to 392 cycles but the MFMA phase grows from 575 to 730.)
    constexpr int DP = STAGES - 2;
    const int gq = wave >> 2;
#pragma unroll
    for (int t = 0; t < DP; ++t)
      if (t < nk) issue(t);
    // DMA instructions per stage of THIS wave: G for whole tiles; 192-row X tiles deal 12 instructions to 8 waves,
    // so waves 4-7 (= the lagging half) issue G - 1
    constexpr bool UNEVEN = (XB % 8192) != 0;
    auto wait_one_stage_in_flight = [&]() {
      if constexpr (UNEVEN) {
        if (gq == 0) wait_vmcnt<G>(); else wait_vmcnt<G - 1>();
      } else {
        wait_vmcnt<G>();
      }
    };
    if (nk > 1) wait_one_stage_in_flight();
    else wait_vmcnt<0>();
    if (gq == 1) __builtin_amdgcn_s_barrier();
#ifdef PM_GEMM_STAMP
    unsigned long long stamp_t[8], stamp_acc[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
    for (int t = 0; t < nk; ++t) {
      PM_STAMP(0);
      __builtin_amdgcn_s_barrier();  // opens R_t
      PM_STAMP(1);
      Frag16 fw[2][NTL], fx[2][MT];
      read_frags(t, fw, fx);
      __builtin_amdgcn_sched_barrier(0);
      PM_STAMP(2);
      if (t + DP < nk) issue(t + DP);
      PM_STAMP(3);
      if (t + 2 < nk) wait_one_stage_in_flight();  // stage t+1 landed, stage t+2 may fly
      else wait_vmcnt<0>();
      PM_STAMP(4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      PM_STAMP(5);
      __builtin_amdgcn_s_barrier();  // opens M_t
      PM_STAMP(6);
      mma_all(fw, fx);
#ifdef PM_GEMM_STAMP
      PM_STAMP(7);
#pragma unroll
      for (int i = 0; i < 7; ++i) stamp_acc[i] += stamp_t[i + 1] - stamp_t[i];
#endif
    }
#ifdef PM_GEMM_STAMP
    if (a.stamps && lane == 0 && blockIdx.y == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) a.stamps[((long)blockIdx.x * NW + wave) * 16 + i] = stamp_acc[i];
      a.stamps[((long)blockIdx.x * NW + wave) * 16 + 7] = nk;
    }
#endif
    if (gq == 0) __builtin_amdgcn_s_barrier();
  }
#ifdef PM_GEMM_STAMP
  stamp_loop_end = __builtin_readcyclecounter();
  stamp_loop_end_rt = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (XSUM) {
    if (do_xsum && lane < 16) {  // one wave per row range: plain read-modify-write, fixed order
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = m0 + wm * TM + 32 * j + lane;
        if (m < a.M) a.xsum[m] = (a.xsum_store ? 0.f : a.xsum[m]) + xs[j][0];
        if (m + 16 < a.M) a.xsum[m + 16] = (a.xsum_store ? 0.f : a.xsum[m + 16]) + xs[j][1];
      }
    }
  }
  const int h = lane >> 5;
  const int epi = a.epilogue;
  if constexpr (DIRECT) {
    // straight from registers (lane = row m, register quad = 4 consecutive n): no LDS, no block barrier -- the
    // stores drain while the CU's other resident block keeps the MFMA pipe busy
    if (a.c_dtype != PM_F32 && epi != PM_EPI_RESIDUAL && epi != PM_EPI_ACCUM && (a.N & 7) == 0 && (a.ldc & 7) == 0) {
      // act-typed output: lanes l and l+32 (same row m, columns 8g+4h) trade 4-vectors so that each holds 8
      // consecutive columns -> 16-B stores
      constexpr int NV8 = NTL * 2;
      long noff8[NV8];
      bool nok8[NV8];
      f32x4 b0[NV8], b1[NV8];
#pragma unroll
      for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int n = n0 + wn * TN + i * 32 + 16 * p + 8 * h;
          nok8[i * 2 + p] = n < a.N;
          noff8[i * 2 + p] = n < a.N ? n : a.N - 8;
        }
#pragma unroll
      for (int e = 0; e < NV8; ++e) {
        b0[e] = b1[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.bias) {
          b0[e] = *reinterpret_cast<const f32x4*>(a.bias + noff8[e]);
          b1[e] = *reinterpret_cast<const f32x4*>(a.bias + noff8[e] + 4);
        }
      }
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = m0 + wm * TM + j * 32 + (lane & 31);
        const bool mok = m < a.M;
        const long row = (long)(mok ? m : a.M - 1) * a.ldc;
#pragma unroll
        for (int i = 0; i < NTL; ++i) {
          long off[2];
          bool ok[2];
          f32x4 lo[2], hi[2];
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int e = i * 2 + p;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float x = acc[i][j][8 * p + k], y = acc[i][j][8 * p + 4 + k];
              swap_halves(x, y);
              lo[p][k] = x + b0[e][k];
              hi[p][k] = y + b1[e][k];
            }
            off[p] = row + noff8[e];
            ok[p] = mok && nok8[e];
          }
          epilogue_batch8<E, 2>(a, epi, off, ok, lo, hi);
        }
      }
#ifdef PM_GEMM_STAMP
      stamp_finish();
#endif
      return;
    }
    constexpr int NV = NTL * 4;
    long noff[NV];
    bool nok[NV];
    f32x4 bv[NV];
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * TN + i * 32 + 8 * g + 4 * h;
        nok[i * 4 + g] = n < a.N;
        noff[i * 4 + g] = n < a.N ? n : a.N - 4;
      }
    if (a.bias) {
#pragma unroll
      for (int e = 0; e < NV; ++e) bv[e] = *reinterpret_cast<const f32x4*>(a.bias + noff[e]);
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) bv[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = m0 + wm * TM + j * 32 + (lane & 31);
      const bool mok = m < a.M;
      const long row = (long)(mok ? m : a.M - 1) * a.ldc;
#pragma unroll
      for (int i = 0; i < NTL; ++i) {  // 4 vectors (one 32x32 accumulator row) per batch
        long off[4];
        bool ok[4];
        f32x4 v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int e = i * 4 + g;
          off[g] = row + noff[e];
          ok[g] = mok && nok[e];
          v[g] = f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]} + bv[e];
        }
        epilogue_batch<E, 4>(a, epi, off, ok, v);
      }
    }
#ifdef PM_GEMM_STAMP
    stamp_finish();
#endif
    return;
  }
  __syncthreads();  // all ring slots dead: reuse LDS for the epilogue staging
  char* st = smem + wave * V3_STAGE_WAVE;
#pragma unroll
  for (int mh = 0; mh < MT / 2; ++mh) {    // 64 rows of the wave tile per pass
#pragma unroll
    for (int nh = 0; nh < NTL / 2; ++nh) {  // 64 columns per pass
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ml = j * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x16& t16 = acc[nh * 2 + i][mh * 2 + j];
            const f32x4 v = {t16[4 * g], t16[4 * g + 1], t16[4 * g + 2], t16[4 * g + 3]};
            *reinterpret_cast<f32x4*>(st + ml * STAGE_ROW + (i * 32 + 8 * g + 4 * h) * 4) = v;
          }
      }
      __builtin_amdgcn_wave_barrier();
      const int mw = m0 + wm * TM + mh * 64, nw = n0 + wn * TN + nh * 64;
      if (a.c_dtype != PM_F32 && epi != PM_EPI_RESIDUAL && epi != PM_EPI_ACCUM && (a.N & 7) == 0 && (a.ldc & 7) == 0) {
        // act-typed output: 8 columns per lane -> 16-B stores (8 rows x 128 B per wave instruction)
        const int c8 = (lane & 7) * 8, n8 = nw + c8;
        const bool nok8 = n8 < a.N;
        const long ncl8 = nok8 ? n8 : a.N - 8;
        f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
        if (a.bias) {
          b0 = *reinterpret_cast<const f32x4*>(a.bias + ncl8);
          b1 = *reinterpret_cast<const f32x4*>(a.bias + ncl8 + 4);
        }
#pragma unroll
        for (int it4 = 0; it4 < 2; ++it4) {
          long off[4];
          bool ok[4];
          f32x4 lo[4], hi[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int ml = (it4 * 4 + u) * 8 + (lane >> 3);
            const int m = mw + ml;
            ok[u] = m < a.M && nok8;
            off[u] = (long)(m < a.M ? m : a.M - 1) * a.ldc + ncl8;
            lo[u] = *reinterpret_cast<const f32x4*>(st + ml * STAGE_ROW + c8 * 4) + b0;
            hi[u] = *reinterpret_cast<const f32x4*>(st + ml * STAGE_ROW + c8 * 4 + 16) + b1;
          }
          epilogue_batch8<E, 4>(a, epi, off, ok, lo, hi);
        }
        __builtin_amdgcn_wave_barrier();
        continue;
      }
      const int c4 = (lane & 15) * 4, n = nw + c4;
      const bool nok = n < a.N;
      const long ncl = nok ? n : a.N - 4;
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + ncl);
#pragma unroll
      for (int it4 = 0; it4 < 4; ++it4) {  // 4 rows x 4 batches of 4: loads of a batch overlap
        long off[4];
        bool ok[4];
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int ml = (it4 * 4 + u) * 4 + (lane >> 4);
          const int m = mw + ml;
          ok[u] = m < a.M && nok;
          off[u] = (long)(m < a.M ? m : a.M - 1) * a.ldc + ncl;
          v[u] = *reinterpret_cast<const f32x4*>(st + ml * STAGE_ROW + c4 * 4) + bv;
        }
        epilogue_batch<E, 4>(a, epi, off, ok, v);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#ifdef PM_GEMM_STAMP
  stamp_finish();
#endif
}

template <int BM_, int BN_, bool WK, bool DIRECT, bool PP, bool XK, typename E>
__global__ __launch_bounds__(V3_WAVES * 64, 2) void gemm_v3_kernel(GemmArgs a) {
  gemm_v3_tile<BM_, BN_, WK, DIRECT, PP, XK, false, E>(a, xcd_remap(blockIdx.x, gridDim.x), blockIdx.y);
}

// ------------------------------------------------------------------------------------------------
// grouped weight gradients: every dW of one transformer block in ONE launch, one full-K tile per workgroup
// ------------------------------------------------------------------------------------------------
// The weight gradients have a huge reduction dimension (K = number of tokens: 12 608 ... 50 432) and few output tiles
// (ViT-B: 27 + 9 + 36 + 36 tiles of 256x256).  One GEMM per launch therefore needs split-K to fill the chip: short
// k-loops, f32 slabs written and re-read, a reduce launch each -- and the prologue / epilogue paid per slice.  Grouping
// the four gradients of a block gives ~108 independent tiles at once: each workgroup runs ONE tile over the whole K
// (394+ k-steps: prologue and epilogue vanish, no slabs, no reduce, the result is deterministic by construction) and the
// launch takes ~100 CUs, which is the share the engine wants to give the weight-gradient stream beside the dgrad chain.
constexpr int kMaxGroup = 8;
struct WgradProb {
  const void* dY;     // [K][M]  (tokens x out features: the Linear's output gradient as stored)
  const void* X;      // [K][N]  (tokens x in features: the Linear's input as stored)
  float* dW;          // [M][N]
  long lddy, ldx, lddw;
  int M, N;           // out features, in features
  int tiles_n, tiles_m;
  int tile_begin;     // first global tile id of this problem
  int accumulate;     // dW += instead of dW =
  float* dbias;       // [M] += column sums of dY (the Linear's bias gradient), or NULL
  float* slab;        // split > 1: f32 partial products [split][M][N] (caller's workspace)
  float* bias_part;   // split > 1 and dbias: partial row sums [split][M]
  long vec_begin;     // split > 1: first float4 index of this problem in the reduce launch
};
struct WgradGroupArgs {
  WgradProb p[kMaxGroup];
  int n, K, total_tiles;
  int split;          // k-slices per tile (1: the tile's workgroup writes dW itself)
  int ksteps_split;
  long total_vec, bias_begin, bias_total;  // reduce launch: float4 items, then bias rows
#ifdef PM_GEMM_STAMP
  unsigned long long* stamps;
#endif
};

// 256 x BN_ tiles, 8 waves on the ping-pong loop (two waves per SIMD, 128 x 64 per wave at BN_ = 256), row sums of dY beside the GEMM.
// (The software-pipelined loop needs 254 VGPRs without the row sums: with them it spills 73 and runs 1.5x slower;
//  without them, bias gradients by separate column-sum passes, it equals this loop with the row sums inside.)
template <int BN_, typename E>
__global__ __launch_bounds__(V3_WAVES * 64, 2) void wgrad_group_kernel(WgradGroupArgs g) {
  // gridDim.x workgroups (a multiple of 8, or the whole work list) walk the (k-slice, tile) items t = blockIdx.x,
  // + gridDim.x, ...: the caller chooses how many CUs the weight-gradient stream takes from the dgrad chain beside it.
  // xcd_remap gives every XCD a contiguous run of items; within a k-slice consecutive items are neighbouring tiles
  // (same dY panel -> same private L2); with gridDim.x % 8 == 0 a workgroup stays on its XCD's run.
  const int work = g.total_tiles * g.split;
  for (int t = blockIdx.x; t < work; t += gridDim.x) {
    const int w = xcd_remap(t, work);
    const int slice = w / g.total_tiles, tile = w - slice * g.total_tiles;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxGroup; ++i)
      if (i < g.n && tile >= g.p[i].tile_begin) pi = i;
    const WgradProb& pr = g.p[pi];
    GemmArgs a;
    a.X = pr.dY; a.W = pr.X; a.ldx = pr.lddy; a.ldw = pr.ldx; a.bias = nullptr; a.C = pr.dW; a.ldc = pr.lddw; a.aux = nullptr;
    a.resid = nullptr; a.M = pr.M; a.N = pr.N; a.K = g.K; a.epilogue = pr.accumulate ? PM_EPI_ACCUM : PM_EPI_STORE;
    a.c_dtype = PM_F32; a.tiles_m = pr.tiles_m; a.tiles_n = pr.tiles_n; a.split_k = 1; a.ksteps_split = 0;
    a.xsum = pr.dbias; a.xsum_store = 0;
    // Consecutive work items run on one XCD (xcd_remap) at the same pace, so what they share they fetch once into that XCD's
    // L2: a tile reads a dY panel [K x 256] and an X panel [K x 256] (6.4 MB each at K = 12 608).  Walk the SHORTER side of the
    // problem fastest, so that a run of ~13 tiles covers a compact rectangle: fc2's gradient is 3 x 12 tiles -- row by row a run
    // touches 2 + 12 panels, column by column 3 + 5 (PMC before: 557 MB fetched per ViT-B block against 335 MB algorithmic).
    a.col_major = pr.tiles_m < pr.tiles_n;
    if (g.split > 1) {  // a k-slice: plain f32 partials into the slab (gemm_v3_tile offsets C by the slice), reduced afterwards
      a.C = pr.slab; a.ldc = pr.N; a.epilogue = PM_EPI_STORE; a.split_k = g.split; a.ksteps_split = g.ksteps_split;
      a.xsum = pr.dbias ? pr.bias_part + (long)slice * pr.M : nullptr; a.xsum_store = 1;
    }
#ifdef PM_GEMM_STAMP
    a.stamps = g.stamps;  // (rows of the block index: the caller hands a region of its own to the grouped launches)
#endif
    gemm_v3_tile<256, BN_, true, true, true, true, true, E>(a, tile - pr.tile_begin, slice);
    __syncthreads();  // every wave is done with the LDS ring before the next tile's first stages are issued
  }
}

// dW (+)= sum over the k-slices of the slab, dbias += sum of the partial row sums: fixed order, one launch for the group.
__global__ __launch_bounds__(256) void wgrad_group_reduce_kernel(WgradGroupArgs g) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < g.bias_begin + g.bias_total; v += stride) {
    if (v < g.total_vec) {
      int pi = 0;
#pragma unroll
      for (int i = 1; i < kMaxGroup; ++i)
        if (i < g.n && v >= g.p[i].vec_begin) pi = i;
      const WgradProb& pr = g.p[pi];
      const long e = (v - pr.vec_begin) * 4;  // element index in [M][N] (N % 8 == 0)
      const long per = (long)pr.M * pr.N;
      f32x4 acc = *reinterpret_cast<const f32x4*>(pr.slab + e);
      for (int sl = 1; sl < g.split; ++sl) acc += *reinterpret_cast<const f32x4*>(pr.slab + sl * per + e);
      const long m = e / pr.N, c = e - m * pr.N;
      float* out = pr.dW + m * pr.lddw + c;
      if (pr.accumulate) acc += *reinterpret_cast<const f32x4*>(out);
      *reinterpret_cast<f32x4*>(out) = acc;
    } else if (v >= g.bias_begin) {
      long r = v - g.bias_begin;
      for (int i = 0; i < g.n; ++i) {
        const WgradProb& pr = g.p[i];
        if (!pr.dbias) continue;
        if (r < pr.M) {
          float sum = 0.f;
          for (int sl = 0; sl < g.split; ++sl) sum += pr.bias_part[(long)sl * pr.M + r];
          pr.dbias[r] += sum;
          break;
        }
        r -= pr.M;
      }
    }
  }
}

// (xk, wk) -> the compile-time pair: f(XK, WK) with std::bool_constant arguments
template <typename F>
int with_layouts(int xk, int wk, F&& f) {
  if (xk) return wk ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  return wk ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

template <typename T>
int launch_generic(const GemmArgs& a, int xk, int wk, hipStream_t s) {
  return with_layouts(xk, wk, [&](auto XK, auto WK) {
    hipLaunchKernelGGL((gemm_generic_kernel<T, decltype(XK)::value, decltype(WK)::value>), dim3(a.tiles_m * a.tiles_n),
                       dim3(kThreads), 4 * TILE_BYTES, s, a);
    return pm_check_launch();
  });
}

template <typename T>
int launch_glds(const GemmArgs& a, int xk, int wk, hipStream_t s) {
  return with_layouts(xk, wk, [&](auto XK, auto WK) {
    auto kern = gemm_glds_kernel<T, decltype(XK)::value, decltype(WK)::value>;
    PM_ALLOW_LDS(kern, GLDS_LDS_BYTES);
    hipLaunchKernelGGL(kern, dim3(a.tiles_m * a.tiles_n, a.split_k), dim3(kThreads), GLDS_LDS_BYTES, s, a);
    return pm_check_launch();
  });
}

// one ring kernel: grid = tiles x k-slices
template <typename E, int BM_, int BN_, bool WK, bool DIRECT, bool PP, bool XK>
int launch_v3(const GemmArgs& a, hipStream_t s) {
  constexpr int ring = V3_STAGES * (BM_ + BN_) * 64;
  constexpr int stage = DIRECT ? 0 : V3_WAVES * V3_STAGE_WAVE;
  constexpr size_t lds = ring > stage ? ring : stage;
  auto kern = gemm_v3_kernel<BM_, BN_, WK, DIRECT, PP, XK, E>;
  PM_ALLOW_LDS(kern, lds);
  hipLaunchKernelGGL(kern, dim3(a.tiles_m * a.tiles_n, a.split_k), dim3(V3_WAVES * 64), lds, s, a);
  return pm_check_launch();
}

// The ring kernels of the forward / dgrad GEMMs (X k-normal, BM x 256 tiles): every configuration the heuristics of plan_gemm
// choose, with the W layouts they choose it for.  plan_gemm and the launcher both read this table; nothing else is instantiated
// (what was measured and left the tree: docs/EXPERIMENT_LOG.md).
struct RingCfg {
  int cfg;         // pm_gemm_opts.variant bits 0-5
  int bm;          // tile rows (192: finer M granularity)
  bool direct;     // register epilogue (LDS-staged otherwise: whole 128-B row segments per store)
  bool pp;         // ping-pong k-loop (software-pipelined otherwise: fragment reads and DMA issue between the wave's own MFMAs)
  bool w_kmajor;   // also built for W k-major (dgrads); every entry is built for W k-normal
};
constexpr RingCfg kRingCfgs[] = {
    {8, 256, false, true, true},   {9, 256, true, true, false},   {10, 192, true, true, false},
    {24, 256, false, false, true}, {25, 256, true, false, false}, {26, 192, true, false, false},
};
constexpr int kNumRingCfgs = sizeof(kRingCfgs) / sizeof(kRingCfgs[0]);
inline const RingCfg* find_ring_cfg(int cfg, int w_kmajor) {
  for (const RingCfg& c : kRingCfgs)
    if (c.cfg == cfg && (!w_kmajor || c.w_kmajor)) return &c;
  return nullptr;
}

template <typename E, int I = 0>
int launch_ring(int cfg, const GemmArgs& a, int w_kmajor, hipStream_t s) {
  if constexpr (I == kNumRingCfgs) {
    return PM_EINVAL;
  } else {
    constexpr RingCfg c = kRingCfgs[I];
    if (c.cfg != cfg) return launch_ring<E, I + 1>(cfg, a, w_kmajor, s);
    if constexpr (c.w_kmajor)
      if (w_kmajor) return launch_v3<E, c.bm, 256, true, c.direct, c.pp, false>(a, s);
    return w_kmajor ? PM_EINVAL : launch_v3<E, c.bm, 256, false, c.direct, c.pp, false>(a, s);
  }
}

#ifdef PM_GEMM_STAMP
unsigned long long* g_stamps = nullptr;  // diagnostic build: set by pm_debug_gemm_stamps
#endif
inline bool is16(int dtype) { return dtype == PM_BF16 || dtype == PM_F16; }

// out[m][n] = (accumulate ? out : 0) + the split-K slabs in the workspace
int launch_splitk_reduce(const void* slabs, void* out, long ldc, int M, int N, int splits, bool accumulate, hipStream_t s) {
  const long nvec = (long)M * (N >> 2);
  int grid = (int)((nvec + 255) / 256);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, (const float*)slabs, (float*)out, ldc, M, N, splits,
                     accumulate ? 1 : 0);
  return pm_check_launch();
}

// Everything the dispatcher decides for one call, as a function of the call's arguments only (no pointers, no state).
struct GemmPlan {
  int status;          // PM_OK, or the refusal of the arguments / shapes (the fields below are then meaningless)
  int family;          // PM_GEMM_GENERIC / LDS128 / RING / RING_WGRAD
  int cfg;             // PM_GEMM_RING: the entry of kRingCfgs
  int tile_m, tile_n;
  int split_k;         // k-slices (> 1: f32 slabs in the workspace, then splitk_reduce_kernel)
  int ksteps_split;    // k-steps of the family's kernel per slice
  int band;            // GemmArgs::col_major
  size_t ws_bytes;     // scratch used
};

// Thresholds of the rules below, each measured (the comment at the rule says how).
constexpr int kTallM = 20000;            // rows from which a problem counts as "tall"
constexpr int kFewTiles = 128;           // fewer 256 x 256 tiles than this: the 128 x 128 kernel ...
constexpr int kFewTilesMaxM = 4096;      // ... for a short chain ...
constexpr int kFewTilesNarrowN = 512;    // ... or a narrow one
constexpr int kTileBand = 6;             // tile columns per band of a wide problem's tile order
constexpr int kWideN = 2048;             // act-typed forward outputs from this width take the LDS-staged epilogue

// The ring configuration of a forward / dgrad GEMM.  Tuned on the ViT-B/16 shapes at M = 12 608.
int choose_ring_cfg(int w_kmajor, int epilogue, int M, int N) {
  // fc1 + GELU, and the dGELU dgrad (reads the saved pre-activation, writes an act-typed [M, 4D] tensor): ping-pong loop with the
  // LDS-staged epilogue -- dGELU stand-alone 96.8 vs 95.1 us at ViT-B, 197 vs 220 us at the MAE decoder, and +0.6 % cls step rate
  // in-step (whole 128-B row segments per store instead of 16-B pieces at a 6-KB stride)
  if (epilogue == PM_EPI_GELU || epilogue == PM_EPI_DGELU) return 8;
  // plain dgrads (dfc1 / dproj / dqkv; W read as stored by ds_read_b64_tr_b16): the software-pipelined loop wins since those reads
  // stopped waiting for the whole DMA ring (PM_LDS_IMAGE): dfc1 66 -> 61 us, dqkv 51 -> 47, decoder dfc1 118 -> 107.  256-row
  // tiles with the staged epilogue although the 192-row direct kernel is faster ALONE (59-62 vs 65 us): in the step the chain runs
  // beside the grouped weight gradients, which hold 108 CUs -- 150 tiles of 256 rows + 108 = the chip, 198 tiles of 192 rows + 108
  // oversubscribe it and the chain's third of a round queues behind the long weight-gradient workgroups (+1.0 % cls in four
  // same-box pairs, MAE +0.2 %)
  if (w_kmajor) return 24;
  // wide act-typed forward outputs (qkv): ping-pong, LDS-staged epilogue
  if (epilogue == PM_EPI_STORE && N >= kWideN) return 8;
  // tall problems (MAE decoder: M = 50 432 -> 197 row tiles, 1.5 rounds of the chip): the epilogue is paid 197 x 2 times and the
  // direct register epilogue's strided 16-B stores cost more than the staging pass: software-pipelined loop + staged epilogue for
  // f32 outputs (proj 59 vs 66 us, fc2 145 vs 147), ping-pong + staged for the act-typed qkv (96 vs 102)
  if (M >= kTallM) return epilogue == PM_EPI_STORE ? 8 : 24;
  // otherwise the direct register epilogue; whole tiles per CU round: 192-row tiles when they need fewer (rounds x rows)
  const long nt = (N + 255) / 256;
  const long c256 = (((M + 255) / 256 * nt + 255) / 256) * 256, c192 = (((M + 191) / 192 * nt + 255) / 256) * 192;
  const bool rows192 = c192 < c256;
  // f32 residual outputs: the software-pipelined loop wins (fc2 80 -> 70 us); narrow act-typed / accumulated ones: ping-pong
  if (epilogue == PM_EPI_RESIDUAL) return rows192 ? 26 : 25;
  return rows192 ? 10 : 9;
}

GemmPlan plan_gemm(int a_kmajor, int b_kmajor, int in_dtype, bool has_bias, int c_dtype, bool ldc_is_n, int epilogue, int M, int N,
                   int K, bool has_ws, size_t ws_bytes, const pm_gemm_opts* opts) {
  GemmPlan p{PM_OK, PM_GEMM_GENERIC, 0, BM, BN, 1, 0, 0, 0};
  auto refuse = [&p](int status) { p.status = status; return p; };
  // per-call options (no process-wide state): the kernel override (bits 0-5: 0 / 1 / a ring cfg; bits 6-7: the weight-gradient
  // tile) and the number of workgroups a split-K weight gradient may spread over
  const int variant = opts ? opts->variant : 0;
  const int force = variant & 63, force_wgrad = (variant >> 6) & 3;
  if ((variant & ~255) || force_wgrad == 3 || (force > 1 && !find_ring_cfg(force, 0))) return refuse(PM_EINVAL);
  int wgrad_blocks = (opts && opts->max_blocks > 0) ? opts->max_blocks : 256;
  if (wgrad_blocks < 16) wgrad_blocks = 16;
  if (wgrad_blocks > 1024) wgrad_blocks = 1024;
  if (M <= 0 || N <= 0 || K <= 0) return refuse(PM_ESHAPE);
  if (!is16(in_dtype) && in_dtype != PM_F32) return refuse(PM_EINVAL);
  if (!is16(c_dtype) && c_dtype != PM_F32) return refuse(PM_EINVAL);
  if (is16(in_dtype) && is16(c_dtype) && c_dtype != in_dtype) return refuse(PM_EINVAL);  // a 16-bit C has the operands' type
  const int epc = is16(in_dtype) ? 8 : 4;
  // 16-byte global chunks: the contiguous dimension of each operand must be a chunk multiple
  if (!a_kmajor && (K % epc)) return refuse(PM_EALIGN);
  if (a_kmajor && (M % epc)) return refuse(PM_EALIGN);
  if (!b_kmajor && (K % epc)) return refuse(PM_EALIGN);
  if (b_kmajor && (N % epc)) return refuse(PM_EALIGN);
  if (N & 3) return refuse(PM_EALIGN);
  if (epilogue < PM_EPI_STORE || epilogue > PM_EPI_ACCUM) return refuse(PM_EINVAL);
  if (epilogue == PM_EPI_RESIDUAL && c_dtype != PM_F32) return refuse(PM_EINVAL);
  if (epilogue == PM_EPI_ACCUM && c_dtype != PM_F32) return refuse(PM_EINVAL);
  const int ke = is16(in_dtype) ? 64 : 32;
  if (K % ke) return p;  // the generic kernel
  // Few tiles (scratch/bench_gemm_smallm.py, profiles/r4_exp3_gemm_smallm*.txt): a problem with fewer than ~half as many
  // 256 x 256 tiles as the chip has CUs runs ONE partial round of long workgroups on the ring kernel -- its time is a tile's
  // latency whatever M is (proj at M = 1 600 ... 6 304: 25-28 us) -- while the 128 x 128 LDS-DMA kernel spreads the same work over
  // 4x the workgroups, two per CU: M = 3 200 (MAE encoder at bs = 64/GPU) qkv 25.3 -> 21.2 us, proj 27.1 -> 18.7, fc2 57.4 -> 43.9,
  // dfc1 55.0 -> 37.4, dqkv 43.3 -> 29.3; the half-batch forward chains of the fine-tune (M = 6 304) proj 28.1 -> 26.0, fc2 58.7 ->
  // 54.0; the 512-wide MAE decoder at M = 12 608: dfc1 44.1 -> 38.5, dqkv 35.6 -> 30.7.  The crossover sits between 117 tiles
  // (128 x 128 wins) and 150 (the ring wins) on all 56 measured (shape, epilogue) points: fewer than 128 tiles -> 128 x 128.
  // ... in the step the rule holds only where the WHOLE chain is small (profiles/r4_exp4_few_tiles.txt): sent to the
  // 128 x 128 kernel, the half-batch proj / fc2 of the fine-tune forward (M = 6 304) cost the step 4 % (MAE bs = 256: 1.6 %) although
  // they are faster alone -- two 66-KB workgroups on a CU keep the other chain's 128-KB ring workgroups off it -- while MAE at
  // bs = 64/GPU gains 4.5-6 %.  Hence the cap on M.
  // ... or narrow (N <= 512: the MAE decoder's proj / fc2 / dgrads at bs = 64/GPU, M = 6 304 / 12 608 -- 50 / 100 tiles; the same
  // experiment: +0.7 % on top; a 512-wide problem never belongs to the fine-tune's or the bs = 256 encoder's half-batch chains).
  // A forced ring cfg switches the rule off.
  const long tiles256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  const bool few_tiles = force == 0 && tiles256 < kFewTiles && (M <= kFewTilesMaxM || N <= kFewTilesNarrowN);
  // large-tile ring kernel: 16-bit operands, X k-normal (forward and dgrad GEMMs), big M
  if (is16(in_dtype) && !a_kmajor && (K % V3_KE) == 0 && M >= 1024 && force != 1 && !few_tiles) {
    const RingCfg* c = find_ring_cfg(force ? force : choose_ring_cfg(b_kmajor, epilogue, M, N), b_kmajor);
    if (!c) return refuse(PM_EINVAL);  // (a forced cfg that is not built for this W layout)
    p.family = PM_GEMM_RING;
    p.cfg = c->cfg;
    p.tile_m = c->bm;
    p.tile_n = 256;
    // Tile order of a wide problem.  xcd_remap hands each XCD a contiguous run of tiles; row by row, a run of ~75 tiles of the dGELU
    // dgrad (50 x 12 tiles) walks all 12 W panels (4.7 MB: more than the XCD's 4 MB L2, beside a 77-MB stream of saved
    // pre-activations) six times -- PMC: 205.8 MB fetched per launch against ~135 MB if every XCD read W once.  In bands of 6 tile
    // columns a run is ~12 row blocks x 6 panels: the band's W (2.4 MB) stays in the L2 while the row blocks stream through once.
    // Measured (profiles/r4_exp11_tile_bands.txt): dGELU dgrad 205.7 -> 172.7 MB fetched, fc1 + GELU 67.5 -> 57.7 MB; stand-alone
    // fc1 + GELU 99.5 -> 95.9 us; in the step +0.6 ... +1.2 % (cls), +0.7 % (MAE bs = 256), two same-box rounds each.
    if ((N + 255) / 256 > kTileBand) p.band = kTileBand;
    return p;
  }
  // split-K: only for f32 plain-store / accumulate outputs without bias (the wgrad shapes: K = #tokens, few tiles)
  const bool splittable = has_ws && !has_bias && c_dtype == PM_F32 && (epilogue == PM_EPI_STORE || epilogue == PM_EPI_ACCUM) &&
                          ldc_is_n;
  // large-K weight gradient (both operands k-major) on the ping-pong ring kernel, split so that tiles x splits ~ one block per CU
  if (splittable && is16(in_dtype) && a_kmajor && b_kmajor && (K % V3_KE) == 0 && K >= 2048 && M >= 256 && N >= 128 && force != 1) {
    // 256x256 tiles (twice the MFMAs per barrier) from 2x2 tiles up: ViT-B qkv / fc1 / fc2 gradients 74 us vs 83 with
    // 256x128; the MAE decoder's 512-wide gradients (K = 50 432 tokens) +2.8 % step rate; neutral for 768x768.
    const bool wide = force_wgrad ? force_wgrad == 2 : ((M + 255) / 256) * ((N + 255) / 256) >= 4;
    p.family = PM_GEMM_RING_WGRAD;
    p.tile_m = 256;
    p.tile_n = wide ? 256 : 128;
    const int tiles = ((M + 255) / 256) * ((N + p.tile_n - 1) / p.tile_n);
    const int nk = K / V3_KE;
    int split = wgrad_blocks / tiles;
    if (split > nk / 16) split = nk / 16;
    if (split > 16) split = 16;
    if (split < 1) split = 1;
    while (split > 1 && (size_t)split * M * N * sizeof(float) > ws_bytes) --split;
    p.ksteps_split = (nk + split - 1) / split;
    p.split_k = (nk + p.ksteps_split - 1) / p.ksteps_split;  // no empty slice
    if (split > 1) p.ws_bytes = (size_t)split * M * N * sizeof(float);
    return p;
  }
  p.family = PM_GEMM_LDS128;
  const int nk = K / ke, tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  p.ksteps_split = nk;
  if (splittable && tiles < 256 && nk >= 16) {
    int split = 512 / tiles;                      // fill the 2-blocks-per-CU machine once
    if (split > nk / 8) split = nk / 8;           // >= 8 k-steps per split
    if (split > 16) split = 16;
    const size_t need = (size_t)split * M * N * sizeof(float);
    if (split > 1 && need <= ws_bytes) {
      p.ksteps_split = (nk + split - 1) / split;
      p.split_k = (nk + p.ksteps_split - 1) / p.ksteps_split;  // no empty split
      p.ws_bytes = need;
    }
  }
  return p;
}

// validate the pointers, plan, launch what the plan says
int gemm_dispatch(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
                  const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid, int M, int N,
                  int K, void* workspace, size_t ws_bytes, const pm_gemm_opts* opts, void* stream) {
  if (!A || !B || !C) return PM_EINVAL;
  const GemmPlan p = plan_gemm(a_kmajor, b_kmajor, in_dtype, bias != nullptr, c_dtype, ldc == N, epilogue, M, N, K,
                               workspace != nullptr, workspace ? ws_bytes : 0, opts);
  if (p.status) return p.status;
  const int epc = is16(in_dtype) ? 8 : 4;
  if ((lda % epc) || (ldb % epc) || (ldc & 3)) return PM_EALIGN;  // leading dimensions: whole 16-byte chunks
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)C & 15)) return PM_EALIGN;
  if (epilogue == PM_EPI_DGELU && !aux) return PM_EINVAL;   // (GELU without aux: the pre-activation is not kept -- forward-only use)
  if (epilogue == PM_EPI_RESIDUAL && !resid) return PM_EINVAL;
  GemmArgs a;
  a.X = A; a.W = B; a.ldx = lda; a.ldw = ldb; a.bias = bias; a.C = C; a.ldc = ldc; a.aux = aux; a.resid = resid;
  a.M = M; a.N = N; a.K = K; a.epilogue = epilogue; a.c_dtype = c_dtype;
  a.tiles_m = (M + p.tile_m - 1) / p.tile_m;
  a.tiles_n = (N + p.tile_n - 1) / p.tile_n;
  a.split_k = p.split_k;
  a.ksteps_split = p.ksteps_split;
  a.xsum = nullptr;
  a.xsum_store = 0;
  a.col_major = p.band;
#ifdef PM_GEMM_STAMP
  a.stamps = g_stamps;
#endif
  if (p.split_k > 1) {  // the kernel writes f32 partial slabs, the reduce launch applies STORE / ACCUM
    a.C = workspace;
    a.epilogue = PM_EPI_STORE;
  }
  hipStream_t s = pm_stream(stream);
  int st = PM_EINVAL;
  switch (p.family) {
    case PM_GEMM_GENERIC: PM_DISPATCH_ACT(in_dtype, T, st = launch_generic<T>(a, a_kmajor, b_kmajor, s)); break;
    case PM_GEMM_LDS128: PM_DISPATCH_ACT(in_dtype, T, st = launch_glds<T>(a, a_kmajor, b_kmajor, s)); break;
    case PM_GEMM_RING: PM_DISPATCH_16(in_dtype, E, st = launch_ring<E>(p.cfg, a, b_kmajor, s)); break;
    case PM_GEMM_RING_WGRAD:  // direct epilogue, ping-pong loop
      PM_DISPATCH_16(in_dtype, E, st = p.tile_n == 128 ? launch_v3<E, 256, 128, true, true, true, true>(a, s)
                                                       : launch_v3<E, 256, 256, true, true, true, true>(a, s));
      break;
  }
  if (st || p.split_k == 1) return st;
  return launch_splitk_reduce(workspace, C, ldc, M, N, p.split_k, epilogue == PM_EPI_ACCUM, s);
}

}  // namespace

extern "C" int pm_gemm_plan(int a_kmajor, int b_kmajor, int in_dtype, int has_bias, int c_dtype, int ldc_is_n, int epilogue, int M,
                            int N, int K, size_t ws_bytes, const pm_gemm_opts* opts, pm_gemm_plan_info* info) {
  const GemmPlan p = plan_gemm(a_kmajor, b_kmajor, in_dtype, has_bias != 0, c_dtype, ldc_is_n != 0, epilogue, M, N, K, ws_bytes > 0,
                               ws_bytes, opts);
  if (p.status == PM_OK && info)
    *info = pm_gemm_plan_info{p.family, p.cfg, p.tile_m, p.tile_n, p.split_k, p.band, p.ws_bytes};
  return p.status;
}

// the split-K slabs of a weight gradient (both operands k-major; f32 dW, no bias) when the caller can give any amount
extern "C" size_t pm_gemm_workspace_bytes(int a_kmajor, int b_kmajor, int in_dtype, int M, int N, int K,
                                          const pm_gemm_opts* opts) {
  if (!(a_kmajor && b_kmajor)) return 0;  // only the split-K weight gradients use scratch
  const GemmPlan p = plan_gemm(a_kmajor, b_kmajor, in_dtype, false, PM_F32, true, PM_EPI_STORE, M, N, K, true, (size_t)-1, opts);
  return p.status == PM_OK ? p.ws_bytes : 0;
}

#ifdef PM_GEMM_STAMP
extern "C" void pm_debug_gemm_stamps(void* p) { g_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

extern "C" int pm_gemm_ex(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
                          const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid,
                          int M, int N, int K, void* workspace, size_t ws_bytes, const pm_gemm_opts* opts, void* stream) {
  return gemm_dispatch(A, lda, a_kmajor, B, ldb, b_kmajor, in_dtype, bias, C, ldc, c_dtype, epilogue, aux, resid, M, N, K,
                       workspace, ws_bytes, opts, stream);
}

extern "C" int pm_gemm_ws(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
                          const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux,
                          const float* resid, int M, int N, int K, void* workspace, size_t ws_bytes, void* stream) {
  return gemm_dispatch(A, lda, a_kmajor, B, ldb, b_kmajor, in_dtype, bias, C, ldc, c_dtype, epilogue, aux, resid, M, N, K,
                       workspace, ws_bytes, nullptr, stream);
}

extern "C" int pm_gemm(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
                       const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid,
                       int M, int N, int K, void* stream) {
  return pm_gemm_ws(A, lda, a_kmajor, B, ldb, b_kmajor, in_dtype, bias, C, ldc, c_dtype, epilogue, aux, resid, M, N, K,
                    nullptr, 0, stream);
}

namespace {

// work items (tiles x k-slices) a group with few tiles is cut into: 224 of the 256 CUs
constexpr int kGroupSplitTarget = 224;

struct GroupPlan {
  int status;        // PM_OK or the refusal
  int bn;            // tile width
  int split;         // k-slices per tile
  int ksteps_split;
  size_t ws_bytes;   // slabs + partial row sums (0 when split == 1)
};

GroupPlan plan_group(const pm_wgrad_item* items, int n, int K, int in_dtype) {
  GroupPlan pl{PM_OK, 256, 1, 0, 0};
  if (!items || n <= 0) { pl.status = PM_EINVAL; return pl; }
  if (n > kMaxGroup || K <= 0) { pl.status = PM_ESHAPE; return pl; }
  if (!is16(in_dtype)) { pl.status = PM_ESHAPE; return pl; }               // (f32 mode keeps the per-GEMM split-K path)
  if ((K % V3_KE) != 0 || K < 2048) { pl.status = PM_ESHAPE; return pl; }  // ring kernel: whole 32-element k-steps, long reduction
  long t256 = 0;
  for (int i = 0; i < n; ++i) {
    const pm_wgrad_item& it = items[i];
    if (!it.dY || !it.X || !it.dW) { pl.status = PM_EINVAL; return pl; }
    if (it.n_out < 256 || it.n_in < 128) { pl.status = PM_ESHAPE; return pl; }
    if ((it.n_out & 7) || (it.n_in & 7) || (it.lddy & 7) || (it.ldx & 7) || (it.lddw & 3)) { pl.status = PM_EALIGN; return pl; }
    if (((uintptr_t)it.dY & 15) || ((uintptr_t)it.X & 15) || ((uintptr_t)it.dW & 15)) { pl.status = PM_EALIGN; return pl; }
    t256 += (long)((it.n_out + 255) / 256) * ((it.n_in + 255) / 256);
  }
  // >= 64 tiles of 256x256 (a ViT-B block: 108): one full-K tile per workgroup, no slabs.  Fewer (the 512-wide MAE decoder
  // block: 48 tiles, K = 50 432 tokens): each tile is cut into k-slices so that tiles x slices ~ the chip (48 x 4 = 192 work
  // items of 394 k-steps), f32 partials in the caller's workspace, ONE reduce launch for the whole group.
  const int nk = K / V3_KE;
  if (t256 < 64) {
    int split = (int)(kGroupSplitTarget / t256);
    if (split > 8) split = 8;
    if (split > nk / 128) split = nk / 128;  // >= 128 k-steps per slice: prologue / epilogue stay small
    if (split > 1) {
      pl.ksteps_split = (nk + split - 1) / split;
      pl.split = (nk + pl.ksteps_split - 1) / pl.ksteps_split;  // no empty slice
    }
  }
  if (pl.split > 1) {
    for (int i = 0; i < n; ++i) {
      pl.ws_bytes += (size_t)pl.split * items[i].n_out * items[i].n_in * sizeof(float);
      if (items[i].dbias) pl.ws_bytes += (((size_t)pl.split * items[i].n_out * sizeof(float)) + 15) & ~(size_t)15;
    }
  } else {
    pl.bn = t256 >= 64 ? 256 : 128;  // without slices: 256x128 tiles double the workgroups of a small group
  }
  return pl;
}

}  // namespace

extern "C" size_t pm_wgrad_group_workspace_bytes(const pm_wgrad_item* items, int n, int K, int in_dtype) {
  const GroupPlan pl = plan_group(items, n, K, in_dtype);
  return pl.status == PM_OK ? pl.ws_bytes : 0;
}

extern "C" int pm_wgrad_group_plan(const pm_wgrad_item* items, int n, int K, int in_dtype, size_t* ws_bytes, int* tiles256,
                                   int* k_slices) {
  const GroupPlan pl = plan_group(items, n, K, in_dtype);
  if (ws_bytes) *ws_bytes = pl.status == PM_OK ? pl.ws_bytes : 0;
  if (k_slices) *k_slices = pl.status == PM_OK ? pl.split : 0;
  if (tiles256) {
    long t = 0;
    if (pl.status == PM_OK)
      for (int i = 0; i < n; ++i) t += (long)((items[i].n_out + 255) / 256) * ((items[i].n_in + 255) / 256);
    *tiles256 = (int)t;
  }
  return pl.status;
}

extern "C" int pm_wgrad_group(const pm_wgrad_item* items, int n, int K, int in_dtype, int max_blocks, void* workspace,
                              size_t ws_bytes, void* stream) {
  GroupPlan pl = plan_group(items, n, K, in_dtype);
  if (pl.status != PM_OK) return pl.status;
  if (pl.split > 1 && (!workspace || ws_bytes < pl.ws_bytes || ((uintptr_t)workspace & 15))) {
    pl.split = 1;  // no room for the slabs: whole-K tiles, narrower so that there are twice as many
    pl.bn = 128;
  }
  if (max_blocks == PM_GROUP_WHOLE_K) {  // the caller pairs this small group with another launch: whole-K 256x256 tiles, no slabs
    pl.split = 1;
    pl.bn = 256;
  }
  const int bn = pl.bn;
  WgradGroupArgs g;
  g.n = n; g.K = K; g.split = pl.split; g.ksteps_split = pl.ksteps_split;
#ifdef PM_GEMM_STAMP
  g.stamps = g_stamps ? g_stamps + 4096L * 8 * 16 : nullptr;  // rows [4096, 4608) x 8 waves of the caller's stamp buffer
#endif
  int total = 0;
  long vec = 0;
  char* ws = reinterpret_cast<char*>(workspace);
  for (int i = 0; i < n; ++i) {
    const pm_wgrad_item& it = items[i];
    WgradProb& p = g.p[i];
    p.dY = it.dY; p.X = it.X; p.dW = it.dW; p.lddy = it.lddy; p.ldx = it.ldx; p.lddw = it.lddw;
    p.M = it.n_out; p.N = it.n_in; p.accumulate = it.accumulate ? 1 : 0; p.dbias = it.dbias;
    p.tiles_n = (it.n_in + bn - 1) / bn;
    p.tiles_m = (it.n_out + 255) / 256;
    p.tile_begin = total;
    total += ((it.n_out + 255) / 256) * p.tiles_n;
    p.slab = nullptr; p.bias_part = nullptr; p.vec_begin = vec;
    if (pl.split > 1) {
      p.slab = reinterpret_cast<float*>(ws);
      ws += (size_t)pl.split * it.n_out * it.n_in * sizeof(float);
      if (it.dbias) {
        p.bias_part = reinterpret_cast<float*>(ws);
        ws += (((size_t)pl.split * it.n_out * sizeof(float)) + 15) & ~(size_t)15;
      }
      vec += (long)it.n_out * it.n_in / 4;
    }
  }
  for (int i = n; i < kMaxGroup; ++i) g.p[i] = g.p[0];
  g.total_tiles = total;
  g.total_vec = vec; g.bias_begin = vec; g.bias_total = 0;
  if (pl.split > 1)
    for (int i = 0; i < n; ++i)
      if (items[i].dbias) g.bias_total += items[i].n_out;
  const int work = total * pl.split;
  int grid = work;
  if (max_blocks > 0 && max_blocks < work) {
    grid = (max_blocks / 8) * 8;  // whole XCD rounds: a workgroup keeps walking its own XCD's run of items
    if (grid < 8) grid = 8;
    if (grid > work) grid = work;
  }
  hipStream_t s = pm_stream(stream);
  PM_DISPATCH_16(in_dtype, E, {
    if (bn == 256) {
      auto kern = wgrad_group_kernel<256, E>;
      constexpr int ring = V3_STAGES * (256 + 256) * 64;
      PM_ALLOW_LDS(kern, ring);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(512), ring, s, g);
    } else {
      auto kern = wgrad_group_kernel<128, E>;
      constexpr int ring = V3_STAGES * (256 + 128) * 64;
      PM_ALLOW_LDS(kern, ring);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(512), ring, s, g);
    }
  });
  int st = pm_check_launch();
  if (st || pl.split == 1) return st;
  const long items_r = g.bias_begin + g.bias_total;
  int rgrid = (int)((items_r + 255) / 256);
  if (rgrid > 2048) rgrid = 2048;
  hipLaunchKernelGGL(wgrad_group_reduce_kernel, dim3(rgrid), dim3(256), 0, s, g);
  return pm_check_launch();
}
