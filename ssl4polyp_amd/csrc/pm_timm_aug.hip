// pm_timm_aug.hip -- timm's RandAugment and random erasing of the reference's MAE fine-tune transform (mae/util/datasets.py:37-47:
// create_transform(is_training=True, auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25, re_mode='pixel'))
// on the device.  The policy works on the cropped uint8 HWC batch, one op per sample and layer; every op restates the Pillow
// routine timm's auto_augment.py calls -- ImageOps.py (autocontrast, equalize, invert, posterize, solarize: point tables),
// ImageEnhance.py -> Blend.c, Filter.c (SMOOTH), Geometry.c (ImagingGenericTransform + affine_transform + bicubic_filter32RGB,
// all double) -- integer for integer, float for float and double for double, so that the frames equal Pillow's byte for byte
// (tests/randaug_ref.py restates the same arithmetic in numpy and holds it to Pillow 12.2 itself).  The erasing works in place on
// the normalised f32 NCHW batch with the counter-based generator of pm_mae.hip (restated here).
// All kernels are byte movers over a batch of a few MB: what matters is the launch count (a layer is two launches, the erasing
// one) and the arithmetic, not tuning.  The host (timm_aug.py) draws everything that is random and per sample.
#include "pm_common.h"

// Blend.c, Filter.c and Geometry.c are C compiled without fused multiply-add, and numpy does not fuse: this file is compiled with
// -ffp-contract=off (__graft_entry__.SOURCE_FLAGS), as pm_augment.hip is; the pragma documents it for other build recipes.
#pragma clang fp contract(off)

namespace {

enum {
  OP_IDENTITY = 0, OP_AUTOCONTRAST = 1, OP_EQUALIZE = 2, OP_INVERT = 3, OP_POSTERIZE = 4, OP_SOLARIZE = 5, OP_SOLARIZE_ADD = 6,
  OP_COLOR = 7, OP_CONTRAST = 8, OP_BRIGHTNESS = 9, OP_SHARPNESS = 10, OP_AFFINE = 11, OP_TRANSPOSE = 12
};
constexpr int kStatWords = 776;  // per sample: 768 u32 bins (R, G, B) + the u64 luminance sum, 3104 bytes (a multiple of 8)

__device__ __forceinline__ bool needs_stats(int op) { return op == OP_AUTOCONTRAST || op == OP_EQUALIZE || op == OP_CONTRAST; }

// the frame an op reads: frame b of src, mirrored when timm's RandomHorizontalFlip (which runs BEFORE the policy) drew a flip
struct Frame {
  const unsigned char* img;
  int H, W;
  bool flip;
  __device__ __forceinline__ const unsigned char* px(int x, int y) const {
    return img + ((long)y * W + (flip ? W - 1 - x : x)) * 3;
  }
};

// (restated from pm_augment.hip) Convert.c rgb2l and Blend.c ImagingBlend(in1 = degenerate, in2 = image, alpha) in C float
__device__ __forceinline__ int rgb2l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ int blend1(int deg, int v, float a, bool interp) {
  const float t = __fadd_rn((float)deg, __fmul_rn(a, __fsub_rn((float)v, (float)deg)));
  if (interp) return (int)t;  // 0 <= alpha <= 1: (UINT8) cast, truncation
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Filter.c ImagingFilter3x3 with ImageFilter.SMOOTH = (1, 1, 1, 1, 5, 1, 1, 1, 1) / 13: the kernel is divided in float first, the
// sum starts at offset + 0.5 and takes the row below, the row itself, the row above, each as (a k0 + b k1) + c k2; clip8
// truncates.  The pixels of the frame's border are copied.
__device__ __forceinline__ int smooth_px(const Frame& f, int x, int y, int c) {
  if (x == 0 || y == 0 || x == f.W - 1 || y == f.H - 1) return f.px(x, y)[c];
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float ss = 0.5f;
  ss += (float)f.px(x - 1, y + 1)[c] * k1 + (float)f.px(x, y + 1)[c] * k1 + (float)f.px(x + 1, y + 1)[c] * k1;
  ss += (float)f.px(x - 1, y)[c] * k1 + (float)f.px(x, y)[c] * k5 + (float)f.px(x + 1, y)[c] * k1;
  ss += (float)f.px(x - 1, y - 1)[c] * k1 + (float)f.px(x, y - 1)[c] * k1 + (float)f.px(x + 1, y - 1)[c] * k1;
  return ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (int)ss);
}

// Geometry.c BICUBIC: p1 + d (p2 + d (p3 + d p4)), every product and sum rounded on its own
__device__ __forceinline__ double bicubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ int clipi(int v, int n) { return v < 0 ? 0 : (v < n ? v : n - 1); }

// Geometry.c bicubic_filter32RGB at the source point (xin, yin): false when the point is outside the frame (the caller leaves the
// fill colour there).  The first of the four rows is clipped into the frame, a later row outside it repeats the row before.
__device__ __forceinline__ bool bicubic_px(const Frame& f, double xin, double yin, int* out) {
  if (xin < 0.0 || xin >= (double)f.W || yin < 0.0 || yin >= (double)f.H) return false;
  xin -= 0.5;
  yin -= 0.5;
  int x = xin < 0.0 ? (int)floor(xin) : (int)xin;
  int y = yin < 0.0 ? (int)floor(yin) : (int)yin;
  const double dx = xin - x, dy = yin - y;
  --x;
  --y;
  const int x0 = clipi(x, f.W), x1 = clipi(x + 1, f.W), x2 = clipi(x + 2, f.W), x3 = clipi(x + 3, f.W);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int yy = y + r;
      if (r == 0 || (yy >= 0 && yy < f.H)) {
        const int yc = r == 0 ? clipi(yy, f.H) : yy;
        v[r] = bicubic((double)f.px(x0, yc)[c], (double)f.px(x1, yc)[c], (double)f.px(x2, yc)[c], (double)f.px(x3, yc)[c], dx);
      } else {
        v[r] = v[r - 1];
      }
    }
    const double t = bicubic(v[0], v[1], v[2], v[3], dy);
    out[c] = t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (int)t);  // (UINT8) v: the RGB filter truncates, it does not round
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// pass 1: what an op needs of the WHOLE frame -- the three histograms (AutoContrast, Equalize) or the luminance sum (Contrast).
// One workgroup per sample; all of it is mirror-invariant, so the flip does not matter here.  Integer atomics in LDS, plain stores
// to global memory: no buffer has to be zeroed first, and integers are order-free.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void randaug_stats_kernel(const unsigned char* __restrict__ src,
                                                             const pm_randaug_op* __restrict__ ops, int stride,
                                                             unsigned int* __restrict__ stats, int HW) {
  __shared__ unsigned int hist[768];
  __shared__ unsigned long long part[16];
  const int b = blockIdx.x;
  const int op = ops[(long)b * stride].op;  // (uniform over the workgroup)
  if (!needs_stats(op)) return;
  const unsigned char* img = src + (long)b * HW * 3;
  unsigned int* out = stats + (long)b * kStatWords;
  if (op == OP_CONTRAST) {
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < HW; i += 1024) {
      const unsigned char* p = img + (long)i * 3;
      acc += (unsigned)rgb2l(p[0], p[1], p[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long s = 0;
      for (int w = 0; w < 16; ++w) s += part[w];
      out[768] = (unsigned int)s;
      out[769] = (unsigned int)(s >> 32);
    }
    return;
  }
  for (int i = threadIdx.x; i < 768; i += 1024) hist[i] = 0u;
  __syncthreads();
  for (int j = threadIdx.x; j < HW * 3; j += 1024) atomicAdd(&hist[(j % 3) * 256 + img[j]], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += 1024) out[i] = hist[i];
}

// the 3 x 256 point table of a table op, built per workgroup
__device__ __forceinline__ void build_lut(unsigned char* lut, int* scratch, const pm_randaug_op& r, const unsigned int* st) {
  const int t = threadIdx.x;
  if (r.op == OP_AUTOCONTRAST) {
    // ImageOps.autocontrast(cutoff=0): lo / hi = first / last non-empty bin of the channel
    if (t < 3) {
      const unsigned int* h = st + t * 256;
      int lo = 0, hi = 255;
      while (lo < 255 && !h[lo]) ++lo;
      while (hi > 0 && !h[hi]) --hi;
      scratch[2 * t] = lo;
      scratch[2 * t + 1] = hi;
    }
    __syncthreads();
    for (int i = t; i < 768; i += 256) {
      const int lo = scratch[2 * (i >> 8)], hi = scratch[2 * (i >> 8) + 1], v = i & 255;
      int ix = v;
      if (hi > lo) {
        const double scale = 255.0 / (double)(hi - lo);
        const double offset = (double)(-lo) * scale;
        ix = (int)((double)v * scale + offset);  // Python's int(): truncation
        ix = ix < 0 ? 0 : (ix > 255 ? 255 : ix);
      }
      lut[i] = (unsigned char)ix;
    }
    return;
  }
  if (r.op == OP_EQUALIZE) {
    // ImageOps.equalize: step = (sum of the non-empty bins - the last of them) // 255; identity with fewer than two non-empty bins
    // or step == 0; else n = step // 2, lut[i] = n // step, n += h[i] (the table entry is an 8-bit value: Image.point clips it)
    if (t < 3) {
      const unsigned int* h = st + t * 256;
      int nonzero = 0, total = 0, last = 0;
      for (int i = 0; i < 256; ++i)
        if (h[i]) { ++nonzero; total += (int)h[i]; last = (int)h[i]; }
      const int step = (total - last) / 255;
      unsigned char* l = lut + t * 256;
      if (nonzero <= 1 || step == 0) {
        for (int i = 0; i < 256; ++i) l[i] = (unsigned char)i;
      } else {
        int n = step / 2;
        for (int i = 0; i < 256; ++i) {
          const int q = n / step;
          l[i] = (unsigned char)(q > 255 ? 255 : q);
          n += (int)h[i];
        }
      }
    }
    return;
  }
  for (int i = t; i < 768; i += 256) {
    const int v = i & 255;
    int o = v;
    switch (r.op) {
      case OP_INVERT: o = 255 - v; break;
      case OP_POSTERIZE: {  // ImageOps.posterize: i & ~(2 ** (8 - bits) - 1)
        const int bits = r.iarg < 0 ? 0 : (r.iarg > 8 ? 8 : r.iarg);
        o = v & ~((1 << (8 - bits)) - 1);
        break;
      }
      case OP_SOLARIZE: o = v < r.iarg ? v : 255 - v; break;
      case OP_SOLARIZE_ADD: o = v < 128 ? (v + r.iarg > 255 ? 255 : (v + r.iarg < 0 ? 0 : v + r.iarg)) : v; break;
      default: break;
    }
    lut[i] = (unsigned char)o;
  }
}

// pass 2: the op.  Sample b = blockIdx.y: its record, and with it the branch taken, is uniform over the workgroup.
__global__ __launch_bounds__(256) void randaug_apply_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                            const pm_randaug_op* __restrict__ ops, int stride,
                                                            const unsigned char* __restrict__ hflip,
                                                            const unsigned int* __restrict__ stats, int H, int W, int fill_r,
                                                            int fill_g, int fill_b) {
  __shared__ unsigned char lut[768];
  __shared__ int scratch[6];
  const int b = blockIdx.y;
  const pm_randaug_op r = ops[(long)b * stride];
  const int HW = H * W;
  const Frame f{src + (long)b * HW * 3, H, W, hflip != nullptr && hflip[b] != 0};
  unsigned char* out = dst + (long)b * HW * 3;
  const unsigned int* st = stats ? stats + (long)b * kStatWords : nullptr;
  int op = r.op;
  if (needs_stats(op) && !st) op = OP_IDENTITY;  // (refused by the entry point; never read through a null pointer)
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;

  if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE || (op >= OP_INVERT && op <= OP_SOLARIZE_ADD)) {
    build_lut(lut, scratch, r, st);
    __syncthreads();
    for (int i = first; i < HW; i += step) {
      const unsigned char* p = f.px(i % W, i / W);
      unsigned char* q = out + (long)i * 3;
      q[0] = lut[p[0]]; q[1] = lut[256 + p[1]]; q[2] = lut[512 + p[2]];
    }
    return;
  }
  if (op >= OP_COLOR && op <= OP_SHARPNESS) {
    const float a = r.farg;
    const bool interp = a >= 0.0f && a <= 1.0f;
    int mean_l = 0;
    if (op == OP_CONTRAST) {  // ImageStat mean = sum / count in double, int(mean + 0.5)
      const unsigned long long s = (unsigned long long)st[768] | ((unsigned long long)st[769] << 32);
      mean_l = (int)((double)s / (double)HW + 0.5);
    }
    for (int i = first; i < HW; i += step) {
      const int x = i % W, y = i / W;
      const unsigned char* p = f.px(x, y);
      int d0 = 0, d1 = 0, d2 = 0;  // Brightness: black
      if (op == OP_COLOR) d0 = d1 = d2 = rgb2l(p[0], p[1], p[2]);
      else if (op == OP_CONTRAST) d0 = d1 = d2 = mean_l;
      else if (op == OP_SHARPNESS) { d0 = smooth_px(f, x, y, 0); d1 = smooth_px(f, x, y, 1); d2 = smooth_px(f, x, y, 2); }
      unsigned char* q = out + (long)i * 3;
      q[0] = (unsigned char)blend1(d0, p[0], a, interp);
      q[1] = (unsigned char)blend1(d1, p[1], a, interp);
      q[2] = (unsigned char)blend1(d2, p[2], a, interp);
    }
    return;
  }
  if (op == OP_AFFINE) {
    for (int i = first; i < HW; i += step) {
      const int x = i % W, y = i / W;
      const double xs = x + 0.5, ys = y + 0.5;  // Geometry.c affine_transform: from the pixel's centre, not accumulated along the row
      const double xin = r.a[0] * xs + r.a[1] * ys + r.a[2];
      const double yin = r.a[3] * xs + r.a[4] * ys + r.a[5];
      int v[3] = {fill_r, fill_g, fill_b};
      bicubic_px(f, xin, yin, v);
      unsigned char* q = out + (long)i * 3;
      q[0] = (unsigned char)v[0]; q[1] = (unsigned char)v[1]; q[2] = (unsigned char)v[2];
    }
    return;
  }
  // Transpose (Image.rotate's early returns: ROTATE_180, and ROTATE_90 / ROTATE_270 of a square frame), identity, unknown op: copy
  int mode = op == OP_TRANSPOSE ? r.iarg : 1;
  if ((mode == 3 || mode == 4) && H != W) mode = 1;
  for (int i = first; i < HW; i += step) {
    const int x = i % W, y = i / W;
    int sx = x, sy = y;
    if (mode == 2) { sx = W - 1 - x; sy = H - 1 - y; }
    else if (mode == 3) { sx = W - 1 - y; sy = x; }   // np.rot90(k=1)
    else if (mode == 4) { sx = y; sy = H - 1 - x; }   // np.rot90(k=3)
    const unsigned char* p = f.px(sx, sy);
    unsigned char* q = out + (long)i * 3;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
  }
}

// ---------------------------------------------------------------------------------------------
// random erasing (timm random_erasing.py) on the normalised f32 batch
// ---------------------------------------------------------------------------------------------
// (restated from pm_mae.hip) Philox4x32-10, Salmon et al. SC'11
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// normal number e of stream sid: Box-Muller over one word pair of block e / 4; u1 in (0, 1], u2 in [0, 1), 24 bits each
// (uniforms: the pair itself -- u1 for an even e, u2 for an odd one -- exact 24-bit values, for checking the words alone)
__device__ __forceinline__ float erase_normal(unsigned long long seed, unsigned long long counter, unsigned sid, unsigned e,
                                              bool uniforms = false) {
  unsigned c[4] = {e >> 2, sid, (unsigned)counter, (unsigned)(counter >> 32)};
  philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
  const unsigned w0 = (e & 2) ? c[2] : c[0], w1 = (e & 2) ? c[3] : c[1];
  const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(w1 >> 8) * 0x1p-24f;
  if (uniforms) return (e & 1) ? u2 : u1;
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (e & 1) ? rad * sn : rad * cs;
}

struct EraseBox { int top, left, h, w; };
__device__ __forceinline__ bool box_ok(const EraseBox& k, int H, int W) {
  return k.h > 0 && k.w > 0 && k.top >= 0 && k.left >= 0 && k.h <= H && k.w <= W && k.top <= H - k.h && k.left <= W - k.w;
}

__global__ __launch_bounds__(256) void random_erase_kernel(float* __restrict__ x, const EraseBox* __restrict__ boxes, int max_count,
                                                           int mode, unsigned long long seed, unsigned long long counter, int C,
                                                           int H, int W) {
  const int b = blockIdx.y;
  float* img = x + (long)b * C * H * W;
  for (int k = 0; k < max_count; ++k) {
    const EraseBox bx = boxes[(long)b * max_count + k];
    if (!box_ok(bx, H, W)) continue;
    const int area = bx.h * bx.w, total = C * area;
    const unsigned sid = (unsigned)b * (unsigned)max_count + (unsigned)k;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
      const int c = e / area, rem = e % area;
      const int y = bx.top + rem / bx.w, xx = bx.left + rem % bx.w;
      bool later = false;  // a later box of the sample covers this element: timm's loop leaves that one's value
      for (int k2 = k + 1; k2 < max_count; ++k2) {
        const EraseBox o = boxes[(long)b * max_count + k2];
        later |= box_ok(o, H, W) && y >= o.top && y < o.top + o.h && xx >= o.left && xx < o.left + o.w;
      }
      if (later) continue;
      float v = 0.0f;
      if (mode == 1) v = erase_normal(seed, counter, sid, (unsigned)c);
      else if (mode == 2) v = erase_normal(seed, counter, sid, (unsigned)e);
      else if (mode == 3) v = erase_normal(seed, counter, sid, (unsigned)e, true);
      img[((long)c * H + y) * W + xx] = v;
    }
  }
}

}  // namespace

static_assert(sizeof(pm_randaug_op) == 64, "pm_randaug_op layout");

static int randaug_shape(int B, int H, int W) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return PM_ESHAPE;
  if ((long)H * W > (1L << 28)) return PM_ESHAPE;  // (pixel and byte indices inside a frame are int)
  return PM_OK;
}

extern "C" int pm_randaug_workspace(int B, size_t* bytes) {
  if (B <= 0 || B > 65535) return PM_ESHAPE;
  if (!bytes) return PM_EINVAL;
  *bytes = (size_t)B * kStatWords * sizeof(unsigned int);
  return PM_OK;
}

extern "C" int pm_randaug_stats(const unsigned char* src, const pm_randaug_op* ops, int stride, void* stats, size_t stats_bytes,
                                int B, int H, int W, void* stream) {
  if (!src || !ops || !stats) return PM_EINVAL;
  const int st = randaug_shape(B, H, W);
  if (st != PM_OK) return st;
  if (stride < 1) return PM_ESHAPE;
  if (stats_bytes < (size_t)B * kStatWords * sizeof(unsigned int)) return PM_EINVAL;
  if ((uintptr_t)stats & 7) return PM_EALIGN;
  hipLaunchKernelGGL(randaug_stats_kernel, dim3(B), dim3(1024), 0, pm_stream(stream), src, ops, stride,
                     reinterpret_cast<unsigned int*>(stats), H * W);
  return pm_check_launch();
}

extern "C" int pm_randaug_apply(const unsigned char* src, unsigned char* dst, const pm_randaug_op* ops, int stride,
                                const unsigned char* hflip, const void* stats, size_t stats_bytes, int B, int H, int W, int fill_r,
                                int fill_g, int fill_b, void* stream) {
  if (!src || !dst || !ops || src == dst) return PM_EINVAL;
  const int st = randaug_shape(B, H, W);
  if (st != PM_OK) return st;
  if (stride < 1) return PM_ESHAPE;
  if (stats && stats_bytes < (size_t)B * kStatWords * sizeof(unsigned int)) return PM_EINVAL;
  if ((uintptr_t)stats & 7) return PM_EALIGN;
  if ((fill_r | fill_g | fill_b) & ~255) return PM_EINVAL;
  int gx = (H * W + 256 * 8 - 1) / (256 * 8);
  const int cap = 8192 / B > 1 ? 8192 / B : 1;  // (at most 8192 blocks over the B samples, as the resized crop)
  gx = gx > cap ? cap : gx;
  hipLaunchKernelGGL(randaug_apply_kernel, dim3(gx, B), dim3(256), 0, pm_stream(stream), src, dst, ops, stride, hflip,
                     reinterpret_cast<const unsigned int*>(stats), H, W, fill_r, fill_g, fill_b);
  return pm_check_launch();
}

extern "C" int pm_random_erase_f32(float* x, const int* boxes, int max_count, int mode, unsigned long long seed,
                                   unsigned long long counter, int B, int C, int H, int W, void* stream) {
  if (!x || !boxes) return PM_EINVAL;
  if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || max_count < 1 || max_count > 64) return PM_ESHAPE;
  if ((long)C * H * W > 0x7fffffffL || (long)B * max_count > 0x7fffffffL) return PM_ESHAPE;
  if (mode < 0 || mode > 3) return PM_EINVAL;
  int gx = (int)(((long)C * H * W + 256 * 8 - 1) / (256 * 8));
  const int cap = 8192 / B > 1 ? 8192 / B : 1;
  gx = gx > cap ? cap : gx;
  hipLaunchKernelGGL(random_erase_kernel, dim3(gx, B), dim3(256), 0, pm_stream(stream), x, reinterpret_cast<const EraseBox*>(boxes),
                     max_count, mode, seed, counter, C, H, W);
  return pm_check_launch();
}
