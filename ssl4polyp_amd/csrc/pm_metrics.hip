// pm_metrics.hip -- cluster-bootstrap replicates of the binary test metrics (include/polypmae.h: pm_boot_metrics), of the whole set
// and per group of frames (pm_group_metrics).
//
// A replicate is a multiset of frames: frame i appears w_i = (times its cluster was drawn) times, and every metric of the
// reference's compute_binary_metrics (classification/analysis/common_metrics.py:100-183) is a function of (score, label, w).
// Nothing is gathered: with the frames of a run sorted once by descending score, a replicate is one integer-weighted scan.
//
//   boot_prepare_kernel  once per bootstrap (the first call of a series, sorted_ready = 0): the sorted view of every run -- score, per-frame log loss (f64), cluster << 1 | label
//   boot_mult_kernel     the multiplicity of every cluster per replicate (integer atomics: order-independent)
//   boot_scan_kernel     one workgroup per (replicate, run): tiles of kTile sorted frames, a carried scan of the weighted
//                        (positives, negatives) pair packed into one 64-bit integer, a carried running maximum that names the
//                        prefix at the previous tie-group end, f64 terms added per thread in tile order and reduced by a fixed
//                        tree at the end.  Integer counts are exact; the result does not depend on how R is cut into calls.
//   group_scan_kernel    one workgroup per (replicate, run, group): the same scan (scan_segment) over the group's segment of the
//                        entry list alone -- tiles from the segment's start, ties end at its end.
#include "pm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kTile = kThreads * kItems;  // metrics.SCAN_TILE
constexpr int kWaves = kThreads / PM_WAVE;
constexpr int kMaxN = 1 << 20, kMaxK = 1 << 20, kMaxC = 1 << 20, kMaxM = 256, kMaxR = 4096;
constexpr int kOut = 16;

typedef unsigned long long u64;

struct BootWs {
  size_t score, loss, cl, mult, bytes;
};

BootWs boot_ws(int N, int M, int R, int C) {
  BootWs w;
  const size_t mn = (size_t)M * N;
  w.score = 0;
  w.loss = w.score + mn * sizeof(double);
  w.cl = w.loss + mn * sizeof(double);
  w.mult = (w.cl + mn * sizeof(int) + 15) & ~(size_t)15;
  w.bytes = (w.mult + (size_t)R * C * sizeof(unsigned) + 15) & ~(size_t)15;
  return w;
}

int boot_shape(int N, int M, int R, int K, int C) {
  if (N < 1 || M < 1 || R < 1 || K < 1 || C < 1) return PM_ESHAPE;
  if (N > kMaxN || M > kMaxM || R > kMaxR || K > kMaxK || C > kMaxC) return PM_ESHAPE;
  if ((long long)N * K > 0x7fffffffLL) return PM_ESHAPE;  // a replicate's total weight <= N * K: the 32-bit halves of the scan
  return PM_OK;
}

// The sorted view of run m: position j of its E positions holds frame order[m][j] (pm_boot_metrics: E = N, every frame once;
// pm_group_metrics: the entry list).  An index outside [0, N) or a cluster outside [0, C) gives the position weight zero (cl = -1)
// instead of an access outside the buffers.
__global__ __launch_bounds__(kThreads) void boot_prepare_kernel(const double* __restrict__ score, const int* __restrict__ order,
                                                                const unsigned char* __restrict__ label,
                                                                const int* __restrict__ cluster, int N, int E, int M, int C,
                                                                double* __restrict__ s_sorted, double* __restrict__ l_sorted,
                                                                int* __restrict__ cl_sorted) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long long)M * E) return;
  const int i = order[idx];
  double s = 0.0, l = 0.0;
  int cl = -1;
  if ((unsigned)i < (unsigned)N) {
    const long long m = idx / E;
    s = score[m * N + i];
    const int c = cluster[i];
    const int y = label[i] != 0;
    if ((unsigned)c < (unsigned)C) cl = (c << 1) | y;
    const double p = fmin(fmax(s, 1e-12), 1.0 - 1e-12);  // np.clip(probs, eps, 1 - eps), common_metrics.py:153-154
    l = y ? -log(p) : -log(1.0 - p);
  }
  s_sorted[idx] = s;
  l_sorted[idx] = l;
  cl_sorted[idx] = cl;
}

__global__ __launch_bounds__(kThreads) void boot_mult_kernel(const int* __restrict__ draws, long long total, int K, int C,
                                                             unsigned* __restrict__ mult) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += stride) {
    const int c = draws[idx];
    if ((unsigned)c < (unsigned)C) atomicAdd(&mult[(idx / K) * C + c], 1u);  // -1 (padding) and anything else outside: no draw
  }
}

__device__ inline u64 wave_scan_add(u64 x, int lane) {
#pragma unroll
  for (int d = 1; d < PM_WAVE; d <<= 1) {
    const u64 v = __shfl_up(x, d);
    if (lane >= d) x += v;
  }
  return x;
}

__device__ inline u64 wave_scan_max(u64 x, int lane) {
#pragma unroll
  for (int d = 1; d < PM_WAVE; d <<= 1) {
    const u64 v = __shfl_up(x, d);
    if (lane >= d && v > x) x = v;
  }
  return x;
}

__device__ inline u64 u64_max(u64 a, u64 b) { return a > b ? a : b; }

// Weighted counts travel as one 64-bit integer: positives in the high half, negatives in the low half.  Both halves stay below
// 2^31 (boot_shape), so sums never carry across, and -- both being non-decreasing along the order -- the packed prefix is
// non-decreasing too: the maximum over earlier tie-group ends IS the prefix at the previous group end.
//
// scan_segment: the n positions s[0 .. n) of one run's view, weights mu[cluster], threshold t -> the 16 values at o.  Called by every
// thread of the workgroup with the same arguments.  Nothing beyond position n - 1 is read: the look-ahead of the last position is
// replaced by "the tie group ends here", so a segment that is followed by another one (pm_group_metrics) ends its last tie group
// whatever score comes next.  n = 0 gives the empty sample's row.
__device__ inline void scan_segment(const double* __restrict__ s, const double* __restrict__ ls, const int* __restrict__ cls,
                                    const unsigned* __restrict__ mu, const double t, const int N, double* __restrict__ o) {
  __shared__ u64 sh_sum[kWaves], sh_max[kWaves], sh_conf[kWaves], sh_roc[kWaves];
  __shared__ double sh_ap[kWaves], sh_loss[kWaves];
  const int tid = threadIdx.x, lane = tid & (PM_WAVE - 1), wave = tid / PM_WAVE;

  u64 carry = 0, last_end = 0;      // the same in every thread: prefix before this tile, prefix at the last group end before it
  u64 conf = 0, roc = 0;            // per thread: weighted (tp, fp) at tau; the AUROC numerator
  double ap = 0.0, loss = 0.0;      // per thread, in tile order

  for (int base = 0; base < N; base += kTile) {
    const int j0 = base + tid * kItems;
    double sc[kItems + 1];
    u64 pre[kItems];
    bool end[kItems];
#pragma unroll
    for (int e = 0; e <= kItems; ++e) sc[e] = (j0 + e < N) ? s[j0 + e] : 0.0;
    u64 run = 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int j = j0 + e;
      u64 w = 0;
      if (j < N) {
        const int c = cls[j];
        const unsigned wt = c >= 0 ? mu[c >> 1] : 0u;
        w = (c & 1) ? (u64)wt << 32 : (u64)wt;
        loss += (double)wt * ls[j];
        if (sc[e] >= t) conf += w;
      }
      end[e] = j < N && (j + 1 >= N || sc[e + 1] != sc[e]);
      run += w;
      pre[e] = run;
    }
    // inclusive prefix of the weights at every position
    const u64 incl = wave_scan_add(run, lane);
    if (lane == PM_WAVE - 1) sh_sum[wave] = incl;
    __syncthreads();
    u64 excl = carry + (incl - run), tile_total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) excl += sh_sum[w];
      tile_total += sh_sum[w];
    }
    u64 tmax = 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      pre[e] += excl;
      if (end[e]) tmax = pre[e];  // non-decreasing: the last end of the thread is its maximum
    }
    // the prefix at the last group end before every position
    const u64 incl_max = wave_scan_max(tmax, lane);
    if (lane == PM_WAVE - 1) sh_max[wave] = incl_max;
    u64 prev = __shfl_up(incl_max, 1);
    if (lane == 0) prev = 0;
    __syncthreads();
    prev = u64_max(prev, last_end);
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) prev = u64_max(prev, sh_max[w]);
      last_end = u64_max(last_end, sh_max[w]);
    }
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      if (end[e]) {
        const u64 d = pre[e] - prev;  // the group's own weighted counts; no borrow, both halves are non-decreasing
        if (d != 0) {                 // a group of total weight zero is no group of the replicate
          const u64 tp = pre[e] >> 32, fp = pre[e] & 0xffffffffu, dtp = d >> 32, dfp = d & 0xffffffffu;
          ap += (double)dtp * ((double)tp / (double)(tp + fp));
          roc += dfp * (2 * (tp - dtp) + dtp);
        }
        prev = pre[e];
      }
    }
    carry += tile_total;
  }

  // fixed-order reductions: a shuffle tree inside the wave, then the waves in order
#pragma unroll
  for (int d = PM_WAVE / 2; d >= 1; d >>= 1) {
    conf += __shfl_down(conf, d);
    roc += __shfl_down(roc, d);
    ap += __shfl_down(ap, d);
    loss += __shfl_down(loss, d);
  }
  if (lane == 0) {
    sh_conf[wave] = conf;
    sh_roc[wave] = roc;
    sh_ap[wave] = ap;
    sh_loss[wave] = loss;
  }
  __syncthreads();
  if (tid != 0) return;
  conf = roc = 0;
  ap = loss = 0.0;
  for (int w = 0; w < kWaves; ++w) {
    conf += sh_conf[w];
    roc += sh_roc[w];
    ap += sh_ap[w];
    loss += sh_loss[w];
  }
  const long long P = (long long)(carry >> 32), Nn = (long long)(carry & 0xffffffffu), n = P + Nn;
  const long long tp = (long long)(conf >> 32), fp = (long long)(conf & 0xffffffffu), tn = Nn - fp, fn = P - tp;
  const double nan = __builtin_nan("");
  o[0] = (double)n;
  o[1] = (double)P;
  o[2] = (double)Nn;
  o[4] = (double)tp;
  o[5] = (double)fp;
  o[6] = (double)tn;
  o[7] = (double)fn;
  if (n == 0) {  // an empty sample: common_metrics.py:112-125
    o[3] = nan;
    for (int k = 8; k < kOut; ++k) o[k] = nan;
    return;
  }
  o[3] = (double)P / (double)n;
  // What scikit-learn 1.7 returns when a class is absent (recorded in tests/golden/boot_metrics.npz): average precision 0 without
  // positives (recall is undefined, every step of it is taken as 0), AUROC undefined, a ratio with an empty denominator 0
  // (zero_division=0), balanced accuracy = the mean recall of the classes that are present, MCC 0 when a marginal is empty.
  o[8] = P > 0 ? ap / (double)P : 0.0;
  o[9] = (P > 0 && Nn > 0) ? (double)roc / (2.0 * (double)P * (double)Nn) : nan;
  const double rec = P > 0 ? (double)tp / (double)P : 0.0;
  const double spec = Nn > 0 ? (double)tn / (double)Nn : 0.0;
  o[10] = rec;
  o[11] = tp + fp > 0 ? (double)tp / (double)(tp + fp) : 0.0;
  o[12] = 2 * tp + fp + fn > 0 ? (double)(2 * tp) / (double)(2 * tp + fp + fn) : 0.0;
  o[13] = (P > 0 && Nn > 0) ? 0.5 * (rec + spec) : (P > 0 ? rec : spec);
  const double den = (double)P * (double)Nn * (double)(tp + fp) * (double)(tn + fn);
  o[14] = den > 0.0 ? (double)(tp * tn - fp * fn) / sqrt(den) : 0.0;
  o[15] = loss / (double)n;
}

__global__ __launch_bounds__(kThreads) void boot_scan_kernel(const double* __restrict__ s_sorted, const double* __restrict__ l_sorted,
                                                             const int* __restrict__ cl_sorted, const unsigned* __restrict__ mult,
                                                             const double* __restrict__ tau, int N, int M, int C,
                                                             double* __restrict__ out) {
  const long long r = blockIdx.x / M, m = blockIdx.x % M;
  scan_segment(s_sorted + m * N, l_sorted + m * N, cl_sorted + m * N, mult + r * C, tau[m], N, out + (long long)blockIdx.x * kOut);
}

// block = (r * M + m) * G + g.  The offsets are clamped to [0, E] and a segment whose start is not below its end is empty, so a
// wrong table gives wrong numbers and never an access outside the view.
__global__ __launch_bounds__(kThreads) void group_scan_kernel(const double* __restrict__ s_sorted, const double* __restrict__ l_sorted,
                                                              const int* __restrict__ cl_sorted, const unsigned* __restrict__ mult,
                                                              const double* __restrict__ tau, const int* __restrict__ seg, int E,
                                                              int M, int G, int C, double* __restrict__ out) {
  const long long g = blockIdx.x % G, rm = blockIdx.x / G, r = rm / M, m = rm % M;
  const int lo = min(max(seg[g], 0), E), hi = min(max(seg[g + 1], 0), E);
  const int n = hi > lo ? hi - lo : 0;
  const long long at = m * E + lo;
  scan_segment(s_sorted + at, l_sorted + at, cl_sorted + at, mult + r * C, tau[m], n, out + (long long)blockIdx.x * kOut);
}

constexpr int kMaxE = 1 << 22, kMaxG = 1 << 16;

int group_shape(int N, int M, int E, int G, int R, int K, int C) {
  if (E < 1 || G < 1 || E > kMaxE || G > kMaxG) return PM_ESHAPE;
  const int st = boot_shape(N, M, R, K, C);
  if (st != PM_OK) return st;
  if ((long long)E * K > 0x7fffffffLL) return PM_ESHAPE;      // a segment's total weight <= E * K: the 32-bit halves of the scan
  if ((long long)R * M * G > 0x7fffffffLL) return PM_ESHAPE;  // one workgroup per (replicate, run, group): the grid's x limit
  return PM_OK;
}

struct BootView {
  double *score, *loss;
  int* cl;
  unsigned* mult;
};

// What both entry points do before their scan, after their shape check: the buffers, the workspace and the alignment, then the
// counters (a memset and boot_mult_kernel) and -- unless the caller states it is there -- the view of E positions per run.
int boot_prepare(const double* score, const int* order, const unsigned char* label, const int* cluster, const int* draws,
                 const double* tau, double* out, int N, int E, int M, int R, int K, int C, int sorted_ready, void* workspace,
                 size_t ws_bytes, hipStream_t s, BootView* v) {
  if (!score || !order || !label || !cluster || !draws || !tau || !out || !workspace) return PM_EINVAL;
  const BootWs ws = boot_ws(E, M, R, C);
  if (ws_bytes < ws.bytes) return PM_EINVAL;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)score & 7) || ((uintptr_t)tau & 7) || ((uintptr_t)out & 7)) return PM_EALIGN;
  unsigned char* wsb = static_cast<unsigned char*>(workspace);
  v->score = reinterpret_cast<double*>(wsb + ws.score);
  v->loss = reinterpret_cast<double*>(wsb + ws.loss);
  v->cl = reinterpret_cast<int*>(wsb + ws.cl);
  v->mult = reinterpret_cast<unsigned*>(wsb + ws.mult);
  if (hipMemsetAsync(v->mult, 0, (size_t)R * C * sizeof(unsigned), s) != hipSuccess) return PM_ELAUNCH;
  const long long me = (long long)M * E, rk = (long long)R * K;
  if (!sorted_ready)  // the view does not depend on the replicates: later calls of a series reuse it
    hipLaunchKernelGGL(boot_prepare_kernel, dim3((unsigned)((me + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, score, order,
                       label, cluster, N, E, M, C, v->score, v->loss, v->cl);
  long long mult_blocks = (rk + kThreads - 1) / kThreads;
  if (mult_blocks > 4096) mult_blocks = 4096;
  hipLaunchKernelGGL(boot_mult_kernel, dim3((unsigned)mult_blocks), dim3(kThreads), 0, s, draws, rk, K, C, v->mult);
  return PM_OK;
}

}  // namespace

extern "C" int pm_boot_metrics_workspace(int N, int M, int R, int K, int C, size_t* bytes) {
  const int st = boot_shape(N, M, R, K, C);
  if (st != PM_OK) return st;
  if (!bytes) return PM_EINVAL;
  *bytes = boot_ws(N, M, R, C).bytes;
  return PM_OK;
}

extern "C" int pm_boot_metrics(const double* score, const int* order, const unsigned char* label, const int* cluster, const int* draws,
                               const double* tau, double* out, int N, int M, int R, int K, int C, int sorted_ready, void* workspace,
                               size_t ws_bytes, void* stream) {
  int st = boot_shape(N, M, R, K, C);
  if (st != PM_OK) return st;
  hipStream_t s = pm_stream(stream);
  BootView v;
  st = boot_prepare(score, order, label, cluster, draws, tau, out, N, N, M, R, K, C, sorted_ready, workspace, ws_bytes, s, &v);
  if (st != PM_OK) return st;
  hipLaunchKernelGGL(boot_scan_kernel, dim3((unsigned)(R * M)), dim3(kThreads), 0, s, v.score, v.loss, v.cl, v.mult, tau, N, M, C, out);
  return pm_check_launch();
}

extern "C" int pm_group_metrics_workspace(int N, int M, int E, int G, int R, int K, int C, size_t* bytes) {
  const int st = group_shape(N, M, E, G, R, K, C);
  if (st != PM_OK) return st;
  if (!bytes) return PM_EINVAL;
  *bytes = boot_ws(E, M, R, C).bytes;  // the view is per entry
  return PM_OK;
}

extern "C" int pm_group_metrics(const double* score, const int* member, const int* seg, const unsigned char* label, const int* cluster,
                                const int* draws, const double* tau, double* out, int N, int M, int E, int G, int R, int K, int C,
                                int sorted_ready, void* workspace, size_t ws_bytes, void* stream) {
  int st = group_shape(N, M, E, G, R, K, C);
  if (st != PM_OK) return st;
  if (!seg) return PM_EINVAL;
  if (((uintptr_t)seg & 3) || ((uintptr_t)member & 3)) return PM_EALIGN;
  hipStream_t s = pm_stream(stream);
  BootView v;
  st = boot_prepare(score, member, label, cluster, draws, tau, out, N, E, M, R, K, C, sorted_ready, workspace, ws_bytes, s, &v);
  if (st != PM_OK) return st;
  hipLaunchKernelGGL(group_scan_kernel, dim3((unsigned)((long long)R * M * G)), dim3(kThreads), 0, s, v.score, v.loss, v.cl, v.mult, tau, seg,
                     E, M, G, C, out);
  return pm_check_launch();
}
