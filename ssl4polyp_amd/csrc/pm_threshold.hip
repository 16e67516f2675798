// pm_threshold.hip -- the decision threshold of a run, chosen on the device (include/polypmae.h: pm_select_tau).
//
// The reference chooses tau on the validation scores (classification/metrics/thresholds.py): compute_policy_threshold for
// f1_opt_on_val / youden_on_val / val_opt_youden (:299-390: at most 200 candidates out of the ascending unique values of
// {0} + scores + {1}, the confusion counts of `score >= candidate`, an objective with two tie-breakers) and
// compute_youden_j_threshold for youden (:68-110: scikit-learn's roc_curve with drop_intermediate, the first maximum of tpr - fpr).
// With the frames of a run in descending score order every candidate is the end of a tie group, and its counts are the prefix
// counts there.  This file is compiled with -ffp-contract=off: the candidate indices restate numpy.linspace(...).astype(int),
// one f64 product each, and every reported ratio is one f64 division of exact integers.
//
//   select_tau_kernel   one workgroup per run.  Phase 1: tiles of kTile sorted frames (gathered through `order`), one carried
//                       integer scan of (positives, negatives, tie-group ends) packed into 3 x 21 bits; every tie-group end writes
//                       its score and its prefix counts to slot (number of ends before it) of the workspace -- the distinct
//                       scores in descending order.  Phase 2: the candidates (one thread each) or the ROC points (strided) read
//                       those slots; maxima and minima across the workgroup are taken by a fixed tree and are exact, so the
//                       reference's comparisons are applied literally.
#include "pm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kTile = kThreads * kItems;  // metrics.SCAN_TILE, as pm_metrics.hip
constexpr int kWaves = kThreads / PM_WAVE;
constexpr int kMaxN = 1 << 20, kMaxM = 256;  // boot_shape's limits
constexpr int kOut = 16, kMaxCand = 200;     // _MAX_THRESHOLD_CANDIDATES
constexpr double kEps = 1e-12;               // _EPS
constexpr int kBits = 21;                    // a count <= 2^20 fits 21 bits
constexpr int kPolicyYouden = 3;             // 0 f1_opt_on_val, 1 youden_on_val, 2 val_opt_youden (the same objective as 1)

typedef unsigned long long u64;
constexpr u64 kMask = (1ull << kBits) - 1;

int tau_shape(int N, int M) {
  if (N < 1 || M < 1 || N > kMaxN || M > kMaxM) return PM_ESHAPE;
  return PM_OK;
}

// per run: the distinct scores in descending order (f64 [N]) and the prefix counts at their group ends (u64 [N]: positives << 21 | negatives)
size_t tau_ws_bytes(int N, int M) { return ((size_t)M * N * (sizeof(double) + sizeof(u64)) + 15) & ~(size_t)15; }

__device__ inline u64 wave_scan_add(u64 x, int lane) {
#pragma unroll
  for (int d = 1; d < PM_WAVE; d <<= 1) {
    const u64 v = __shfl_up(x, d);
    if (lane >= d) x += v;
  }
  return x;
}

struct OpMax {
  __device__ double operator()(double a, double b) const { return a > b ? a : b; }
};
struct OpMin {
  __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; }
};
struct OpAdd {
  __device__ long long operator()(long long a, long long b) const { return a + b; }
};

// The value of `op` over the workgroup, in every thread: a butterfly inside the wave, then the waves in order.  max, min and an
// integer sum are exact, so the tree's shape does not show in the result.
template <typename T, typename Op> __device__ inline T block_all(T v, T* sh, Op op) {
  const int lane = threadIdx.x & (PM_WAVE - 1), wave = threadIdx.x / PM_WAVE;
#pragma unroll
  for (int d = PM_WAVE / 2; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
  __syncthreads();  // the previous use of sh has been read
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  T r = sh[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r = op(r, sh[w]);
  return r;
}

__device__ inline double ratio(long long num, long long den) { return den > 0 ? (double)num / (double)den : 0.0; }  // _safe_divide

// _compute_metrics_for_tau (thresholds.py:254-272) behind the first four columns
__device__ inline void write_row(double* o, double tau, double n_cand, double degenerate, double objective, long long tp, long long fp,
                                 long long P, long long Nn, double n_unique, double index) {
  const long long tn = Nn - fp, fn = P - tp;
  const double rec = ratio(tp, tp + fn), fpr = ratio(fp, fp + tn);
  o[0] = tau;
  o[1] = n_cand;
  o[2] = degenerate;
  o[3] = objective;
  o[4] = (double)tp;
  o[5] = (double)fp;
  o[6] = (double)tn;
  o[7] = (double)fn;
  o[8] = rec;
  o[9] = ratio(tp, tp + fp);
  o[10] = ratio(2 * tp, 2 * tp + fp + fn);
  o[11] = rec;
  o[12] = fpr;
  o[13] = rec - fpr;
  o[14] = n_unique;
  o[15] = index;
}

__global__ __launch_bounds__(kThreads) void select_tau_kernel(const double* __restrict__ score, const int* __restrict__ order,
                                                              const unsigned char* __restrict__ label,
                                                              const double* __restrict__ previous_tau, int policy, int N,
                                                              double* pt_score, u64* pt_count,  // written, then read by other threads
                                                              double* __restrict__ out, double* __restrict__ candidates) {
  __shared__ u64 sh_sum[kWaves];
  __shared__ double sh_f[kWaves];
  __shared__ long long sh_i[kWaves];
  const int tid = threadIdx.x, lane = tid & (PM_WAVE - 1), wave = tid / PM_WAVE;
  const long long m = blockIdx.x;
  const double* s = score + m * N;
  const int* ord = order + m * N;
  double* ps = pt_score + m * N;
  u64* pc = pt_count + m * N;
  double* o = out + m * kOut;
  double* cand_out = candidates ? candidates + m * kMaxCand : nullptr;
  const double nan = __builtin_nan("");
  const double prev_tau = previous_tau[m];
  const bool carried = prev_tau - prev_tau == 0.0;  // math.isfinite(previous_tau)
  const double t_fixed = carried ? prev_tau : 0.5;

  // ---- phase 1: the distinct scores and the counts at their group ends
  u64 carry = 0;       // the same in every thread: (positives, negatives, ends) before this tile
  long long conf = 0;  // per thread: (tp << 21 | fp) at t_fixed, for the one-class case
  for (int base = 0; base < N; base += kTile) {
    const int j0 = base + tid * kItems;
    double sc[kItems + 1];
    u64 pre[kItems];
    bool end[kItems];
    int lab[kItems];
#pragma unroll
    for (int e = 0; e <= kItems; ++e) {
      sc[e] = 0.0;
      if (e < kItems) lab[e] = -1;
      if (j0 + e < N) {
        const int i = ord[j0 + e];
        if ((unsigned)i < (unsigned)N) {  // anything else: a frame of score 0 and of no class
          sc[e] = s[i];
          if (e < kItems) lab[e] = label[i] != 0;
        }
      }
    }
    u64 run = 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int j = j0 + e;
      end[e] = j < N && (j + 1 >= N || sc[e + 1] != sc[e]);
      const u64 w = lab[e] < 0 ? 0 : (lab[e] ? 1ull << (2 * kBits) : 1ull << kBits);
      if (sc[e] >= t_fixed) conf += (long long)(w >> kBits);
      run += w + (end[e] ? 1 : 0);
      pre[e] = run;
    }
    const u64 incl = wave_scan_add(run, lane);
    __syncthreads();  // the previous tile's sh_sum has been read
    if (lane == PM_WAVE - 1) sh_sum[wave] = incl;
    __syncthreads();
    u64 excl = carry + (incl - run), tile_total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) excl += sh_sum[w];
      tile_total += sh_sum[w];
    }
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      if (end[e]) {
        const u64 p = pre[e] + excl;
        const int g = (int)(p & kMask) - 1;  // ends before this one: 0 <= g <= j < N
        ps[g] = sc[e];
        pc[g] = p >> kBits;
      }
    }
    carry += tile_total;
  }
  conf = block_all(conf, sh_i, OpAdd());  // (also the barrier that makes the slots visible to the whole workgroup)
  const long long P = (long long)(carry >> (2 * kBits)), Nn = (long long)((carry >> kBits) & kMask);
  const int D = (int)(carry & kMask);

  // ---- one class only (thresholds.py:326-345); youden has no answer there (:98-99)
  if (P == 0 || Nn == 0) {
    if (cand_out && tid < kMaxCand) cand_out[tid] = (tid == 0 && policy != kPolicyYouden) ? t_fixed : nan;
    if (tid == 0) {
      const bool y = policy == kPolicyYouden;
      write_row(o, y ? nan : t_fixed, 0.0, 1.0, nan, y ? 0 : conf >> kBits, y ? 0 : conf & (long long)kMask, P, Nn, nan,
                (carried && !y) ? -2.0 : -1.0);
    }
    return;
  }

  if (policy != kPolicyYouden) {
    // ---- phase 2: the candidates of _prepare_candidate_thresholds, one thread each
    const bool has0 = ps[D - 1] == 0.0, has1 = ps[0] == 1.0;
    const int U = D + (has0 ? 0 : 1) + (has1 ? 0 : 1);
    const int n_cand = U < kMaxCand ? U : kMaxCand;
    const double step = (double)(U - 1) / (double)(kMaxCand - 1);  // numpy.linspace: delta / div
    const double ninf = -__builtin_inf();
    double c = nan, obj = ninf, rec = ninf;
    long long tp = 0, fp = 0;
    if (tid < n_cand) {
      int idx = tid;
      if (U > kMaxCand) idx = tid == kMaxCand - 1 ? U - 1 : (int)floor((double)tid * step);
      if (idx == 0 && !has0) {
        c = 0.0, tp = P, fp = Nn;  // below every score: all positive
      } else if (idx == U - 1 && !has1) {
        c = 1.0;                   // above every score: none positive
      } else {
        const int g = D - 1 - (idx - (has0 ? 0 : 1));
        c = ps[g];
        tp = (long long)(pc[g] >> kBits), fp = (long long)(pc[g] & kMask);
      }
      const long long fn = P - tp;
      rec = ratio(tp, P);
      obj = policy == 0 ? ratio(2 * tp, 2 * tp + fp + fn) : rec - ratio(fp, Nn);
    }
    if (cand_out && tid < kMaxCand) cand_out[tid] = c;
    const double best = block_all(obj, sh_f, OpMax());
    const bool s0 = tid < n_cand && obj >= best - kEps;
    const double rmax = block_all(s0 ? rec : ninf, sh_f, OpMax());
    const bool s1 = s0 && rec >= rmax - kEps;
    const long long pick = block_all(s1 ? (long long)tid : (long long)kThreads, sh_i, OpMin());  // ascending: the lowest tau
    if (tid == pick) write_row(o, c, (double)n_cand, 0.0, obj, tp, fp, P, Nn, (double)U, (double)tid);
    return;
  }

  // ---- phase 2, youden: the points roc_curve keeps, J = tps / P - fps / Nn, the first maximum
  if (cand_out && tid < kMaxCand) cand_out[tid] = nan;
  int Dp = D;  // a last group without a frame (padding of `order`) is no point
  if (D >= 2 && pc[D - 1] == pc[D - 2]) Dp = D - 1;
  double jbest = -__builtin_inf();
  long long gbest = kMaxN, kept = 0;
  for (int g = tid; g < Dp; g += kThreads) {
    const u64 cur = pc[g];
    const long long tp = (long long)(cur >> kBits), fp = (long long)(cur & kMask);
    bool keep = g == 0 || g == Dp - 1;
    if (!keep) {  // np.diff(fps, 2) or np.diff(tps, 2) at this point
      const u64 a = pc[g - 1], b = pc[g + 1];
      const long long tpa = (long long)(a >> kBits), fpa = (long long)(a & kMask);
      const long long tpb = (long long)(b >> kBits), fpb = (long long)(b & kMask);
      keep = (fpb - 2 * fp + fpa) != 0 || (tpb - 2 * tp + tpa) != 0;
    }
    if (keep) {
      ++kept;
      const double J = (double)tp / (double)P - (double)fp / (double)Nn;
      if (J > jbest) jbest = J, gbest = g;
    }
  }
  const double jmax = block_all(jbest, sh_f, OpMax());
  const long long pick = block_all(jbest == jmax ? gbest : (long long)kMaxN, sh_i, OpMin());
  kept = block_all(kept, sh_i, OpAdd());
  if (tid != 0) return;
  if (!(jmax > 0.0)) {  // the prepended point (0, 0) at +inf comes first: tau = nextafter(max score, 1.0)
    const double top = ps[0], tau = nextafter(top, 1.0);
    const bool at = top >= tau;  // a top score of 1.0 stays a prediction
    write_row(o, tau, (double)(kept + 1), 0.0, 0.0, at ? (long long)(pc[0] >> kBits) : 0, at ? (long long)(pc[0] & kMask) : 0, P, Nn,
              (double)Dp, 0.0);
    return;
  }
  write_row(o, ps[pick], (double)(kept + 1), 0.0, jmax, (long long)(pc[pick] >> kBits), (long long)(pc[pick] & kMask), P, Nn, (double)Dp,
            (double)(pick + 1));
}

}  // namespace

extern "C" int pm_select_tau_workspace(int N, int M, size_t* bytes) {
  const int st = tau_shape(N, M);
  if (st != PM_OK) return st;
  if (!bytes) return PM_EINVAL;
  *bytes = tau_ws_bytes(N, M);
  return PM_OK;
}

extern "C" int pm_select_tau(const double* score, const int* order, const unsigned char* label, const double* previous_tau, int policy,
                             double* out, double* candidates, int N, int M, void* workspace, size_t ws_bytes, void* stream) {
  const int st = tau_shape(N, M);
  if (st != PM_OK) return st;
  if (!score || !order || !label || !previous_tau || !out || !workspace) return PM_EINVAL;
  if (policy < 0 || policy > kPolicyYouden) return PM_EINVAL;
  if (ws_bytes < tau_ws_bytes(N, M)) return PM_EINVAL;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)score & 7) || ((uintptr_t)previous_tau & 7) || ((uintptr_t)out & 7) ||
      ((uintptr_t)candidates & 7) || ((uintptr_t)order & 3))
    return PM_EALIGN;
  double* pt_score = static_cast<double*>(workspace);
  u64* pt_count = reinterpret_cast<u64*>(pt_score + (size_t)M * N);
  hipLaunchKernelGGL(select_tau_kernel, dim3((unsigned)M), dim3(kThreads), 0, pm_stream(stream), score, order, label, previous_tau,
                     policy, N, pt_score, pt_count, out, candidates);
  return pm_check_launch();
}
