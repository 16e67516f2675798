// Baseline JPEG decode on the device, bit for bit with libjpeg-turbo as Pillow runs it (ssl4polyp_amd/jpeg.py packs the batch on
// the host: unstuffed restart intervals, frame rows, derived Huffman tables, quantisation tables).  Three integer-only stages:
//   1. jpeg_huff_kernel: entropy decode (jdhuff.c decode_mcu) -> int16 coefficients in natural order.  One lane per restart
//      interval; a wave packs 64 intervals of different frames (the host sorts them by length so its lanes finish together), so
//      the decode holds few SIMDs while the training step runs beside it.  The bit reservoir lives in registers and is refilled
//      from aligned 16-byte loads issued a group ahead.  The coefficients are zeroed on the stream, then only the nonzero ones
//      are stored.  Lookahead tables in LDS when the batch's tables fit in 31 KiB (with the zigzag table: < 32 KiB).
//   2. jpeg_idct_kernel: dequantise + islow inverse DCT (jidctint.c) -> uint8 component planes padded to the MCU grid, one thread
//      per 8 x 8 block as in pm_augment.hip's jpeg_roundtrip_kernel.
//   3. jpeg_color_kernel: fancy upsampling where libjpeg-turbo uses it (jdsample.c h2v1 / h2v2 triangle filters, downsampled
//      width > 2; replication otherwise; the rows above / below the plane repeat its first / last real row as jdmainct.c's
//      context pointers do) + YCbCr -> RGB (jdcolor.c) or grey -> RGB, packed HWC at each frame's output offset.
//   jpeg_copy_kernel puts the frames decoded on the host (fallback) into their slots.
// pm_jpeg_decode_parallel replaces stage 1 by self-synchronising decoding inside an interval (Klein & Wiseman 2003; Weissenberger &
// Schmidt 2021), because real files carry no restart markers and a frame would otherwise be one lane.  The host cuts every interval
// into subsequences of kSubBytes, one lane each, 256 lanes per workgroup:
//   jpeg_sync_kernel (1 + sync_rounds launches): a lane decodes, without storing, from its entry state E (bit position, block in
//      MCU, zigzag index; the true start for an interval's first lane, a guess for every other) to the first symbol boundary at or
//      past its subsequence's end and keeps the exit state X, the blocks it completed and the DC differences it summed.  Inside the
//      workgroup E[i + 1] <- X[i] and the lanes whose entry changed decode again until nothing changes; across workgroups the first
//      lane takes the exit state its predecessor held after the previous launch (double-buffered, one launch per round).
//   jpeg_verify_kernel: an interval is converged iff E[i] == X[i - 1] for each of its lanes but the first -- by induction from the
//      true start every E is then the sequential decoder's state.  Nothing else is accepted.  Also the per-workgroup totals of
//      (blocks, DC sums) for the scan.
//   jpeg_write_kernel: exclusive scan per interval (inside the workgroup + the totals of the workgroups before it) -> the block
//      index and the predictors a lane starts from; lanes of converged intervals decode once more, now storing as decode_block does.
//   jpeg_huff_kernel with a predicate decodes the intervals that are not converged (and the empty ones): never a wrong pixel.
// No kernel waits on another workgroup and the host reads nothing back: the number of launches is fixed by sync_rounds.
// Bad data follows libjpeg's rules, and every access is bounded by construction: a code longer than 16 bits decodes as symbol 0,
// reading past the interval yields zero bits and the MCUs after the one that ran out stay zero (jdhuff.c insufficient_data), runs
// index a natural-order table padded with 63, a lane writes its interval's MCUs only, and a table row that would address memory
// outside the caller's buffers is skipped.  (The pixels of a corrupt frame can still differ from Pillow's where libjpeg-turbo's SIMD
// IDCT saturates garbage coefficients that the C arithmetic restated here wraps.)
#include "pm_common.h"

namespace {

struct HuffTable {            // jpeg.py derive_huffman (jdhuff.c d_derived_tbl)
  unsigned short look[256];   // code length << 8 | symbol for codes of <= 8 bits; 9 << 8: longer
  int maxcode[18];
  int valoffset[18];
  unsigned char huffval[256];
  uint4 limit[2];             // lengths 9..16: (maxcode + 1) << (16 - l), carried over lengths without codes (non-decreasing)
  int voff[8];                // lengths 9..16: valoffset
  unsigned char pad[48];
};
static_assert(sizeof(HuffTable) == 1024, "HuffTable layout (jpeg.HUFF_RECORD)");

constexpr int kIntervalWords = 8;  // (the frame row: pm_common.h kFrameWords)
constexpr int kLdsTables = 31;  // < 32 KiB of LDS with the zigzag table (the step's GEMMs hold 128 of the CU's 160 KiB)
#ifndef PM_JPEG_SUBSEQ_BYTES
#define PM_JPEG_SUBSEQ_BYTES 128  // (-DPM_JPEG_SUBSEQ_BYTES=64 / 256 with jpeg.SUBSEQ_BYTES set alike: side builds for the timing script)
#endif
constexpr int kSubBytes = PM_JPEG_SUBSEQ_BYTES;  // bytes per subsequence (jpeg.SUBSEQ_BYTES): whole aligned 16-byte groups
static_assert(kSubBytes >= 16 && kSubBytes % 16 == 0, "a subsequence is whole 16-byte groups");
constexpr long kSubBits = 8L * kSubBytes;
constexpr int kWg = 256;        // subsequences (lanes) per workgroup of the parallel entropy stage
constexpr int kCntSequential = 0, kCntSteps = 1, kCntRounds = 2, kCntWords = 16;  // workspace header (uint32), zeroed per call

__device__ const unsigned char kNatural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33,
                                               40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                                               29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                               47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// The bit reservoir: 64 bits in registers, refilled 32 bits at a time from 16-byte groups of the interval, two groups in flight (the
// group being consumed and the next one, loaded when the one before it was taken up: ~128 bits ahead of its use).  `left` counts
// the interval's bits not yet consumed; below zero, a decode has read past its data (libjpeg's insufficient_data).
struct BitReader {
  const uint4* groups;
  long g, gend;            // next group to load, end of the interval's groups
  unsigned long long buf;  // the next `bits` bits of the interval, left-aligned; zeros below them
  int bits, ci;            // ci: words of `cur` taken up
  long left;
  uint4 cur, nxt;
  __device__ __forceinline__ uint4 load() {
    const uint4 v = g < gend ? groups[g] : make_uint4(0u, 0u, 0u, 0u);  // past the interval: zero bits
    ++g;
    return v;
  }
  __device__ __forceinline__ void init(const uint4* p, long g0, long n, long nbits) {
    groups = p;
    g = g0;
    gend = g0 + n;
    buf = 0;
    bits = 0;
    ci = 0;
    left = nbits;
    cur = load();
    nxt = load();
  }
  __device__ __forceinline__ void fill() {  // afterwards at least 32 bits are in the reservoir
    if (bits <= 32) {
      const unsigned v = ci == 0 ? cur.x : (ci == 1 ? cur.y : (ci == 2 ? cur.z : cur.w));
      buf |= (unsigned long long)__builtin_bswap32(v) << (32 - bits);
      bits += 32;
      if (++ci == 4) {
        cur = nxt;
        nxt = load();
        ci = 0;
      }
    }
  }
  __device__ __forceinline__ unsigned peek(int n) const { return (unsigned)(buf >> (64 - n)); }  // 1 <= n <= 32
  __device__ __forceinline__ void skip(int n) {
    buf <<= n;
    bits -= n;
    left -= n;
  }
};

// jdhuff.c HUFF_DECODE + jpeg_huff_decode: at most 17 bits (a code over 16 bits is symbol 0).  A code longer than the lookahead
// finds its length from the eight left-justified limits at once (two 16-byte reads) instead of one maxcode read per extra bit:
// the first l with (16 bits) < limit[l] is the first l with code_l <= maxcode[l], which is where jpeg_huff_decode's loop stops.
__device__ __forceinline__ int huff_decode(BitReader& br, const HuffTable* t) {
  const unsigned p16 = br.peek(16);
  const unsigned look = t->look[p16 >> 8];
  int nb = look >> 8, sym = look & 0xFF;
  if (nb > 8) {
    const uint4 a = t->limit[0], b = t->limit[1];
    const int l = 9 + (p16 >= a.x) + (p16 >= a.y) + (p16 >= a.z) + (p16 >= a.w) + (p16 >= b.x) + (p16 >= b.y) + (p16 >= b.z) +
                  (p16 >= b.w);
    if (l > 16) {
      sym = 0;
      nb = 17;
    } else {
      sym = t->huffval[((p16 >> (16 - l)) + t->voff[l - 9]) & 0xFF];
      nb = l;
    }
  }
  br.skip(nb);
  return sym;
}

__device__ __forceinline__ int huff_extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

// one block of decode_mcu: DC difference + prediction, then the AC run / size symbols; only nonzero coefficients are stored
__device__ __forceinline__ void decode_block(BitReader& br, const HuffTable* dc, const HuffTable* ac, int& pred, short* blk,
                                             const unsigned char* nat) {
  br.fill();
  int s = huff_decode(br, dc);
  s = s > 15 ? 15 : s;  // (DC tables are checked on the host: symbols <= 15)
  int diff = 0;
  if (s) {
    diff = huff_extend((int)br.peek(s), s);
    br.skip(s);
  }
  pred = (int)((unsigned)pred + (unsigned)diff);  // (libjpeg-turbo adds as unsigned: corrupt data may wrap)
  if ((short)pred != 0) blk[0] = (short)pred;
  for (int k = 1; k < 64; ++k) {
    br.fill();
    const int sym = huff_decode(br, ac);
    const int r = sym >> 4;
    s = sym & 15;
    if (s) {
      k += r;  // <= 78: the padded table keeps it inside the block
      const int v = huff_extend((int)br.peek(s), s);
      br.skip(s);
      blk[nat[k]] = (short)v;
    } else {
      if (r != 15) break;
      k += 15;
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(64) void jpeg_huff_kernel(const unsigned* __restrict__ words, long n_words, const int* __restrict__ iv,
                                                       int n_iv, const int* __restrict__ fr, int n_fr,
                                                       const HuffTable* __restrict__ huff, int n_huff, short* __restrict__ coef,
                                                       long blocks, const int* __restrict__ bad, const int* __restrict__ subseq,
                                                       int n_subseq, unsigned* __restrict__ counters) {
  // bad != null: the sequential way out of pm_jpeg_decode_parallel -- only the intervals that are not converged, or whose rows have
  // no (consistent) subsequences, are decoded here
  __shared__ HuffTable lds_tab[kLds ? kLdsTables : 1];
  __shared__ unsigned char nat[80];
  if (kLds) {
    const unsigned* src = reinterpret_cast<const unsigned*>(huff);
    unsigned* dst = reinterpret_cast<unsigned*>(lds_tab);
    for (int i = threadIdx.x; i < n_huff * 256; i += 64) dst[i] = src[i];
  }
  for (int i = threadIdx.x; i < 80; i += 64) nat[i] = kNatural[i];
  __syncthreads();
  const HuffTable* tabs = kLds ? lds_tab : huff;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_iv) return;
  const int* I = iv + (long)i * kIntervalWords;
  const int f = I[0], nbytes = I[2], m0 = I[3], nm = I[4];
  const long w0 = I[1];
  if (f < 0 || f >= n_fr || w0 < 0 || (w0 & 3) || nbytes < 0 || m0 < 0 || nm < 0) return;
  const long ng = ((long)nbytes + 15) >> 4;  // 16-byte groups
  if (w0 + ng * 4 > n_words) return;
  if (bad) {
    const long s0 = I[5], ns = ((long)nbytes + kSubBytes - 1) / kSubBytes;
    const bool covered = ns > 0 && s0 >= 0 && s0 + ns <= n_subseq && subseq[s0] == i && subseq[s0 + ns - 1] == i;
    if (covered && !bad[i]) return;
    if (ns > 0) atomicAdd(counters + kCntSequential, 1u);  // (a counter for pm_jpeg_decode_parallel's stats, not on the result path)
  }
  const int* F = fr + (long)f * kFrameWords;
  if (!frame_ok(F, blocks)) return;
  const int ncomp = F[2], hs = F[3], vs = F[4], mcux = F[5];
  if ((long)m0 + nm > (long)mcux * F[6]) return;
  const HuffTable *dc0 = nullptr, *dc1 = nullptr, *dc2 = nullptr, *ac0 = nullptr, *ac1 = nullptr, *ac2 = nullptr;
  for (int c = 0; c < ncomp; ++c)
    if (F[8 + c] < 0 || F[8 + c] >= n_huff || F[11 + c] < 0 || F[11 + c] >= n_huff) return;
  dc0 = tabs + F[8];
  ac0 = tabs + F[11];
  if (ncomp == 3) {
    dc1 = tabs + F[9];
    dc2 = tabs + F[10];
    ac1 = tabs + F[12];
    ac2 = tabs + F[13];
  }
  const long base0 = F[17], base1 = F[18], base2 = F[19];
  const int bw0 = mcux * hs;
  BitReader br;
  br.init(reinterpret_cast<const uint4*>(words), w0 >> 2, ng, 8L * nbytes);
  int p0 = 0, p1 = 0, p2 = 0;  // DC predictors, reset at every interval start
  for (int m = m0; m < m0 + nm; ++m) {
    const int my = m / mcux, mx = m - my * mcux;
    for (int by = 0; by < vs; ++by)
      for (int bx = 0; bx < hs; ++bx)
        decode_block(br, dc0, ac0, p0, coef + (base0 + (long)(my * vs + by) * bw0 + mx * hs + bx) * 64, nat);
    if (ncomp == 3) {
      const long cb = (long)my * mcux + mx;
      decode_block(br, dc1, ac1, p1, coef + (base1 + cb) * 64, nat);
      decode_block(br, dc2, ac2, p2, coef + (base2 + cb) * 64, nat);
    }
    if (br.left < 0) break;  // this MCU read past the data: the rest of the interval stays zero (uniform grey), as in decode_mcu
  }
}

// the device frame whose first entry (word `word` of its row, an int32 or the low word of an int64) is the last one <= key
__device__ __forceinline__ int find_frame(const int* fr, int n_fr, long key, bool wide, int word) {
  int lo = 0, hi = n_fr - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int* F = fr + (long)mid * kFrameWords;
    const long v = wide ? frame_long(F, word) : (long)F[word];
    if (v <= key) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, unsigned char* __restrict__ planes, long blocks,
                                                        const int* __restrict__ fr, int n_fr, const int* __restrict__ quant,
                                                        int n_quant) {
  const long gb = (long)blockIdx.x * 256 + threadIdx.x;
  if (gb >= blocks || n_fr <= 0) return;
  const int* F = fr + (long)find_frame(fr, n_fr, gb, false, 17) * kFrameWords;
  if (!frame_ok(F, blocks)) return;
  const int ncomp = F[2], hs = F[3], vs = F[4], mcux = F[5], mcuy = F[6];
  const int c = ncomp == 3 ? (gb >= F[19] ? 2 : (gb >= F[18] ? 1 : 0)) : 0;
  const int bw = c == 0 ? mcux * hs : mcux, bh = c == 0 ? mcuy * vs : mcuy;
  const long local = gb - F[17 + c];
  if (local < 0 || local >= (long)bw * bh) return;  // (a block between frames: nobody's)
  const int q = F[14 + c];
  if (q < 0 || q >= n_quant) return;
  const int* Q = quant + q * 64;
  int v[64];
  const int4* src = reinterpret_cast<const int4*>(coef + gb * 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int4 x = src[j];
    const int e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      v[8 * j + 2 * h] = (int)(short)(e[h] & 0xFFFF) * Q[8 * j + 2 * h];
      v[8 * j + 2 * h + 1] = (int)(short)((unsigned)e[h] >> 16) * Q[8 * j + 2 * h + 1];
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) jidct8(v + k, 8, true);
#pragma unroll
  for (int r = 0; r < 8; ++r) jidct8(v + 8 * r, 1, false);
  const long by = local / bw, bx = local - by * bw;
  unsigned char* dst = planes + (long)F[17 + c] * 64 + by * 8 * (bw * 8) + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int s = v[8 * r + k] + 128;
      s = s < 0 ? 0 : (s > 255 ? 255 : s);
      if (k < 4) lo |= (unsigned)s << (8 * k);
      else hi |= (unsigned)s << (8 * (k - 4));
    }
    *reinterpret_cast<uint2*>(dst + (long)r * bw * 8) = make_uint2(lo, hi);
  }
}

// stage 3: one thread per pixel of the device frames (the pixel fetch itself is pm_common.h jpeg_pixel_rgb)
__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* __restrict__ planes, long blocks, const int* __restrict__ fr,
                                                         int n_fr, long pixels, unsigned char* __restrict__ out, long out_bytes) {
  const long gp = (long)blockIdx.x * 256 + threadIdx.x;
  if (gp >= pixels || n_fr <= 0) return;
  const int* F = fr + (long)find_frame(fr, n_fr, gp, true, 22) * kFrameWords;
  if (!frame_ok(F, blocks)) return;
  const int H = F[0], W = F[1];
  const long local = gp - frame_long(F, 22), o = frame_long(F, 20);
  if (local < 0 || local >= (long)H * W || o < 0 || o + (long)H * W * 3 > out_bytes) return;
  const int y = (int)(local / W), x = (int)(local - (long)y * W);
  int r, g, b;
  jpeg_pixel_rgb(planes, F, x, y, r, g, b);
  unsigned char* d = out + o + local * 3;
  d[0] = (unsigned char)r;
  d[1] = (unsigned char)g;
  d[2] = (unsigned char)b;
}

// blockIdx.y: the fallback frame; table row (source offset, output offset, bytes)
__global__ __launch_bounds__(256) void jpeg_copy_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                        const long long* __restrict__ tab, unsigned char* __restrict__ out,
                                                        long out_bytes) {
  const long long* T = tab + (long)blockIdx.y * 3;
  const long s = T[0], d = T[1], n = T[2];
  if (s < 0 || d < 0 || n < 0 || s + n > src_bytes || d + n > out_bytes) return;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[d + i] = src[s + i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Parallel entropy decoding inside an interval (see the header comment)
// ---------------------------------------------------------------------------------------------------------------------------------
// A decoder state at a symbol boundary, relative to the end of the subsequence before it: bits past that end (< 32: a symbol is at
// most 17 + 15 bits), block in MCU << 8, zigzag index << 16 (0: a DC symbol is next).  The true start and the guess are both 0.
__device__ __forceinline__ unsigned pack_state(long off, int c, int z) { return (unsigned)off | ((unsigned)c << 8) | ((unsigned)z << 16); }

struct SubLane {  // what lane i (one subsequence) knows about its interval; ok: every row it names is inside the caller's buffers
  bool ok;
  int row, k, nsub;  // interval row, index of the subsequence in its interval, subsequences of the interval
  int m0, nm, bpm, lum;  // first MCU, MCU count, blocks per MCU, luma blocks per MCU
  long g0, ng, nbits;
  const int* F;
};

__device__ __forceinline__ SubLane sub_lane(long i, long n_words, const int* iv, int n_iv, const int* fr, int n_fr, int n_huff, long blocks,
                                            const int* subseq, int n_subseq) {
  SubLane L;
  L.ok = false;
  if (i >= n_subseq) return L;
  L.row = subseq[i];
  if (L.row < 0 || L.row >= n_iv) return L;
  const int* I = iv + (long)L.row * kIntervalWords;
  const int f = I[0], nbytes = I[2];
  const long w0 = I[1], s0 = I[5];
  L.m0 = I[3];
  L.nm = I[4];
  if (f < 0 || f >= n_fr || w0 < 0 || (w0 & 3) || nbytes < 0 || L.m0 < 0 || L.nm < 0) return L;
  L.ng = ((long)nbytes + 15) >> 4;
  if (w0 + L.ng * 4 > n_words) return L;
  L.nsub = (int)(((long)nbytes + kSubBytes - 1) / kSubBytes);
  if (s0 < 0 || s0 > i || i - s0 >= L.nsub || s0 + L.nsub > n_subseq) return L;
  L.k = (int)(i - s0);
  L.F = fr + (long)f * kFrameWords;
  if (!frame_ok(L.F, blocks)) return L;
  const int ncomp = L.F[2];
  if ((long)L.m0 + L.nm > (long)L.F[5] * L.F[6]) return L;
  for (int c = 0; c < ncomp; ++c)
    if (L.F[8 + c] < 0 || L.F[8 + c] >= n_huff || L.F[11 + c] < 0 || L.F[11 + c] >= n_huff) return L;
  L.lum = ncomp == 3 ? L.F[3] * L.F[4] : 1;
  L.bpm = ncomp == 3 ? L.lum + 2 : 1;
  L.g0 = w0 >> 2;
  L.nbits = 8L * nbytes;
  L.ok = true;
  return L;
}

// the reader positioned at bit p of the interval
__device__ __forceinline__ void reader_at(BitReader& br, const unsigned* words, const SubLane& L, long p) {
  br.init(reinterpret_cast<const uint4*>(words), L.g0 + (p >> 7), L.ng - (p >> 7), L.nbits - (p & ~31L));
  br.ci = (int)(p >> 5) & 3;
  br.fill();
  br.skip((int)(p & 31));
}

// One lane's decode from entry state `e`.  kStore = false (jpeg_sync_kernel): to the first symbol boundary at or past the end of
// the subsequence; returns the exit state and adds the blocks completed / the DC differences per component to `acc`.  kStore =
// true (jpeg_write_kernel): `acc` holds the block index and the three predictors at the entry; coefficients are stored as
// decode_block stores them, with jpeg_huff_kernel's stop rules (the interval's block count; after the MCU during which the reader
// ran past the interval's bits nothing more is decoded); the last lane of an interval does not stop at its subsequence's end.
template <bool kStore>
__device__ __forceinline__ unsigned sub_decode(const SubLane& L, const unsigned* words, const HuffTable* tabs, const unsigned char* nat,
                                               unsigned e, uint4& acc, short* coef) {
  const long off = e & 63;
  int c = (int)((e >> 8) & 7), z = (int)((e >> 16) & 63);
  c = c < L.bpm ? c : L.bpm - 1;
  const long end = (kStore && L.k == L.nsub - 1) ? (1L << 62) : (long)(L.k + 1) * kSubBits;
  BitReader br;
  reader_at(br, words, L, (long)L.k * kSubBits + off);
  const int* F = L.F;
  const int hs = F[3], vs = F[4], mcux = F[5];
  const long total = (long)L.nm * L.bpm;
  long b = kStore ? (long)acc.x : 0;
  if (kStore && (b >= total || (c == 0 && z == 0 && br.left < 0))) return 0;
  int comp = c < L.lum ? 0 : c - L.lum + 1;
  const HuffTable* dc = tabs + F[8 + comp];
  const HuffTable* ac = tabs + F[11 + comp];
  short* blk = nullptr;
  auto block_ptr = [&](long bi) -> short* {
    const long mi = bi / L.bpm;
    const int cc = (int)(bi - mi * L.bpm);
    const int m = L.m0 + (int)mi, my = m / mcux, mx = m - my * mcux;
    if (cc < L.lum) {
      const int by = cc / hs, bx = cc - by * hs;
      return coef + ((long)F[17] + (long)(my * vs + by) * (mcux * hs) + mx * hs + bx) * 64;
    }
    return coef + ((long)F[17 + cc - L.lum + 1] + (long)my * mcux + mx) * 64;
  };
  if (kStore) blk = block_ptr(b);
  while (L.nbits - br.left < end) {
    br.fill();
    if (z == 0) {
      int s = huff_decode(br, dc);
      s = s > 15 ? 15 : s;
      int diff = 0;
      if (s) {
        diff = huff_extend((int)br.peek(s), s);
        br.skip(s);
      }
      unsigned d;  // kStore: the predictor; else: the sum of differences
      if (comp == 0) d = (acc.y += (unsigned)diff);
      else if (comp == 1) d = (acc.z += (unsigned)diff);
      else d = (acc.w += (unsigned)diff);
      if (kStore && (short)d != 0) blk[0] = (short)d;
      z = 1;
    } else {
      const int sym = huff_decode(br, ac);
      const int r = sym >> 4, s = sym & 15;
      if (s) {
        z += r;  // <= 78: the padded table keeps it inside the block
        const int v = huff_extend((int)br.peek(s), s);
        br.skip(s);
        if (kStore) blk[nat[z]] = (short)v;
        ++z;
      } else {
        z = r == 15 ? z + 16 : 64;
      }
      if (z >= 64) {  // the block is complete
        z = 0;
        ++b;
        c = c + 1 == L.bpm ? 0 : c + 1;
        if (kStore) {
          if (b >= total || (c == 0 && br.left < 0)) break;
          blk = block_ptr(b);
        }
        comp = c < L.lum ? 0 : c - L.lum + 1;
        dc = tabs + F[8 + comp];
        ac = tabs + F[11 + comp];
      }
    }
  }
  if (!kStore) acc.x += (unsigned)b;
  return pack_state(L.nbits - br.left - end, c, z);
}

__device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ uint4 sub4(uint4 a, uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// inclusive prefix sums (wrapping) of one uint4 per thread over the workgroup; buf: 2 * kWg entries of LDS; returns where they lie
__device__ __forceinline__ const uint4* wg_scan(uint4 v, uint4* buf) {
  const int t = threadIdx.x;
  uint4* cur = buf;
  uint4* nxt = buf + kWg;
  cur[t] = v;
  __syncthreads();
  for (int d = 1; d < kWg; d <<= 1) {
    nxt[t] = t >= d ? add4(cur[t], cur[t - d]) : cur[t];
    __syncthreads();
    uint4* x = cur;
    cur = nxt;
    nxt = x;
  }
  return cur;
}

// copy the batch's tables into LDS (kLds) and the zigzag table; ends with a barrier
template <bool kLds>
__device__ __forceinline__ void load_tables(HuffTable* lds_tab, unsigned char* nat, const HuffTable* huff, int n_huff) {
  if (kLds) {
    const unsigned* src = reinterpret_cast<const unsigned*>(huff);
    unsigned* dst = reinterpret_cast<unsigned*>(lds_tab);
    for (int i = threadIdx.x; i < n_huff * 256; i += kWg) dst[i] = src[i];
  }
  for (int i = threadIdx.x; i < 80; i += kWg) nat[i] = kNatural[i];
  __syncthreads();
}

// Launch `round` of the synchronisation: E / X / ACC are the lanes' entry states, exit states and (blocks, DC sums x 3); wgx holds
// the exit state of every workgroup's last lane, written to half (round & 1) and read from the other half.
template <bool kLds>
__global__ __launch_bounds__(kWg) void jpeg_sync_kernel(const unsigned* __restrict__ words, long n_words, const int* __restrict__ iv,
                                                        int n_iv, const int* __restrict__ fr, int n_fr,
                                                        const HuffTable* __restrict__ huff, int n_huff, long blocks,
                                                        const int* __restrict__ subseq, int n_subseq, int round, int n_wg,
                                                        unsigned* __restrict__ E, unsigned* __restrict__ X, uint4* __restrict__ ACC,
                                                        unsigned* __restrict__ wgx, unsigned* __restrict__ counters) {
  __shared__ HuffTable lds_tab[kLds ? kLdsTables : 1];
  __shared__ unsigned char nat[80];
  __shared__ unsigned xs[kWg];
  const int t = threadIdx.x, wg = blockIdx.x;
  const long i = (long)wg * kWg + t;
  const SubLane L = sub_lane(i, n_words, iv, n_iv, fr, n_fr, n_huff, blocks, subseq, n_subseq);
  unsigned e = 0, x = 0;
  uint4 acc = make_uint4(0u, 0u, 0u, 0u);
  bool dirty = L.ok;
  unsigned* wgx_out = wgx + (long)(round & 1) * n_wg;
  if (round > 0) {
    const unsigned* wgx_in = wgx + (long)((round - 1) & 1) * n_wg;
    dirty = false;
    if (L.ok) {
      e = E[i];
      x = X[i];
      if (t == 0 && L.k > 0) {
        const unsigned ne = wgx_in[wg - 1];  // (k > 0: i > 0, so wg > 0)
        dirty = ne != e;
        e = ne;
      }
    }
    if (!__syncthreads_or(dirty)) {  // the workgroup's entry is the one it used: nothing changes
      if (t == kWg - 1) wgx_out[wg] = L.ok ? x : 0u;
      return;
    }
    if (t == 0) atomicOr(counters + kCntRounds, 1u << (round - 1));  // (counters: stats only)
  }
  load_tables<kLds>(lds_tab, nat, huff, n_huff);
  const HuffTable* tabs = kLds ? lds_tab : huff;
  bool touched = false;
  int steps = 0;
  // every step the prefix of lanes that descends from the workgroup's first lane grows by one: at most kWg steps
  for (int it = 0; it <= kWg; ++it) {
    if (dirty) {
      acc = make_uint4(0u, 0u, 0u, 0u);
      x = sub_decode<false>(L, words, tabs, nat, e, acc, nullptr);
      touched = true;
    }
    xs[t] = x;
    __syncthreads();
    ++steps;
    dirty = false;
    if (L.ok && L.k > 0 && t > 0) {  // the hand-over stays inside the interval and inside the workgroup
      const unsigned ne = xs[t - 1];
      dirty = ne != e;
      e = ne;
    }
    if (!__syncthreads_or(dirty)) break;
  }
  if (touched) {
    E[i] = e;
    X[i] = x;
    ACC[i] = acc;
  }
  if (t == kWg - 1) wgx_out[wg] = L.ok ? x : 0u;
  if (t == 0) atomicMax(counters + kCntSteps, (unsigned)steps);
}

// the acceptance rule + the per-workgroup totals of the scan: tails[wg] = the sums over the lanes of the interval that holds the
// workgroup's last lane
__global__ __launch_bounds__(kWg) void jpeg_verify_kernel(long n_words, const int* __restrict__ iv, int n_iv, const int* __restrict__ fr,
                                                          int n_fr, int n_huff, long blocks, const int* __restrict__ subseq,
                                                          int n_subseq, const unsigned* __restrict__ E,
                                                          const unsigned* __restrict__ X, const uint4* __restrict__ ACC,
                                                          uint4* __restrict__ tails, int* __restrict__ bad) {
  __shared__ uint4 buf[2 * kWg];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * kWg + t;
  const SubLane L = sub_lane(i, n_words, iv, n_iv, fr, n_fr, n_huff, blocks, subseq, n_subseq);
  if (L.ok && L.k > 0 && (subseq[i - 1] != L.row || E[i] != X[i - 1])) bad[L.row] = 1;  // (plain store of one value: no order matters)
  const uint4* P = wg_scan(L.ok ? ACC[i] : make_uint4(0u, 0u, 0u, 0u), buf);
  if (t == kWg - 1) {
    uint4 tail = make_uint4(0u, 0u, 0u, 0u);
    if (L.ok) tail = L.k < t ? sub4(P[t], P[t - L.k - 1]) : P[t];
    tails[blockIdx.x] = tail;
  }
}

template <bool kLds>
__global__ __launch_bounds__(kWg) void jpeg_write_kernel(const unsigned* __restrict__ words, long n_words, const int* __restrict__ iv,
                                                         int n_iv, const int* __restrict__ fr, int n_fr,
                                                         const HuffTable* __restrict__ huff, int n_huff, long blocks,
                                                         const int* __restrict__ subseq, int n_subseq,
                                                         const unsigned* __restrict__ E, const uint4* __restrict__ ACC,
                                                         const uint4* __restrict__ tails, const int* __restrict__ bad,
                                                         short* __restrict__ coef) {
  __shared__ HuffTable lds_tab[kLds ? kLdsTables : 8];  // (first the scan's 8 KiB, then the tables)
  __shared__ unsigned char nat[80];
  __shared__ int first_wg;
  uint4* buf = reinterpret_cast<uint4*>(lds_tab);
  const int t = threadIdx.x, wg = blockIdx.x;
  const long i = (long)wg * kWg + t;
  const SubLane L = sub_lane(i, n_words, iv, n_iv, fr, n_fr, n_huff, blocks, subseq, n_subseq);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  // the interval's lanes before this one: inside the workgroup ...
  const uint4* P = wg_scan(L.ok ? ACC[i] : zero, buf);
  uint4 start = zero;
  if (L.ok) {
    if (t > 0) start = P[t - 1];
    if (L.k < t) start = sub4(start, P[t - L.k - 1]);
  }
  if (t == 0) first_wg = (L.ok && L.k > 0) ? (int)((i - L.k) / kWg) : wg;
  __syncthreads();
  // ... and in the workgroups before it, back to the one where the first lane's interval starts
  uint4 part = zero;
  for (int w = first_wg + t; w < wg; w += kWg) part = add4(part, tails[w]);
  P = wg_scan(part, buf);
  if (L.ok && L.k > t) start = add4(start, P[kWg - 1]);
  __syncthreads();
  load_tables<kLds>(lds_tab, nat, huff, n_huff);
  const HuffTable* tabs = kLds ? lds_tab : huff;
  if (!L.ok || bad[L.row]) return;
  sub_decode<true>(L, words, tabs, nat, E[i], start, coef);
}

__global__ void jpeg_stats_kernel(const unsigned* __restrict__ counters, int n_subseq, int n_iv, int* __restrict__ stats) {
  stats[0] = n_subseq;
  stats[1] = n_iv;
  stats[2] = (int)counters[kCntSequential];
  stats[3] = (int)counters[kCntSteps];
  stats[4] = __popc(counters[kCntRounds]);
}

// workspace of pm_jpeg_decode_parallel: counters, bad[n_iv] (zeroed together), then E, X, ACC per lane, wgx, tails per workgroup
struct ParallelWs {
  size_t bad, e, x, acc, wgx, tails, bytes;
  int n_wg;
};
static ParallelWs parallel_ws(int n_iv, int n_subseq) {
  ParallelWs w;
  w.n_wg = (n_subseq + kWg - 1) / kWg;
  const size_t lanes = (size_t)w.n_wg * kWg;
  w.bad = kCntWords * 4;
  w.acc = (w.bad + (size_t)n_iv * 4 + 15) & ~(size_t)15;
  w.tails = w.acc + lanes * 16;
  w.e = w.tails + (size_t)w.n_wg * 16;
  w.x = w.e + lanes * 4;
  w.wgx = w.x + lanes * 4;
  w.bytes = w.wgx + (size_t)w.n_wg * 8;
  return w;
}

}  // namespace

extern "C" int pm_jpeg_decode(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals,
                              const int* frames, int n_frames, const unsigned char* huff, int n_huff, const int* quant, int n_quant,
                              const unsigned char* fallback, long fallback_bytes, const long long* fallback_table, int n_fallback,
                              short* coef, unsigned char* planes, long blocks, long pixels, unsigned char* out, long out_bytes,
                              void* stream) {
  if (n_intervals < 0 || n_frames < 0 || n_huff < 0 || n_quant < 0 || n_fallback < 0 || n_fallback > 65535 || entropy_bytes < 0 ||
      fallback_bytes < 0 || blocks < 0 || pixels < 0 || out_bytes < 0)
    return PM_ESHAPE;
  if (entropy_bytes % 16 != 0 || reinterpret_cast<uintptr_t>(entropy) % 16 != 0) return PM_EALIGN;
  if ((n_frames > 0 || n_fallback > 0) && !out) return PM_EINVAL;
  if (n_frames > 0 && (!frames || (n_intervals > 0 && (!intervals || !entropy || !huff)) || (blocks > 0 && (!coef || !planes || !quant))))
    return PM_EINVAL;
  if (n_fallback > 0 && (!fallback_table || (fallback_bytes > 0 && !fallback))) return PM_EINVAL;
  hipStream_t s = pm_stream(stream);
  if (n_frames > 0 && blocks > 0) {
    if (hipMemsetAsync(coef, 0, (size_t)blocks * 64 * sizeof(short), s) != hipSuccess) return PM_ELAUNCH;
    if (n_intervals > 0) {
      const dim3 grid((n_intervals + 63) / 64);
      const HuffTable* t = reinterpret_cast<const HuffTable*>(huff);
      const unsigned* w = reinterpret_cast<const unsigned*>(entropy);
      if (n_huff <= kLdsTables)
        hipLaunchKernelGGL(jpeg_huff_kernel<true>, grid, dim3(64), 0, s, w, entropy_bytes / 4, intervals, n_intervals, frames,
                           n_frames, t, n_huff, coef, blocks, nullptr, nullptr, 0, nullptr);
      else
        hipLaunchKernelGGL(jpeg_huff_kernel<false>, grid, dim3(64), 0, s, w, entropy_bytes / 4, intervals, n_intervals, frames,
                           n_frames, t, n_huff, coef, blocks, nullptr, nullptr, 0, nullptr);
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, coef, planes, blocks, frames,
                       n_frames, quant, n_quant);
    if (pixels > 0)
      hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, planes, blocks, frames, n_frames,
                         pixels, out, out_bytes);
  }
  if (n_fallback > 0)
    hipLaunchKernelGGL(jpeg_copy_kernel, dim3(64, n_fallback), dim3(256), 0, s, fallback, fallback_bytes, fallback_table, out,
                       out_bytes);
  if (hipGetLastError() != hipSuccess) return PM_ELAUNCH;
  return PM_OK;
}

extern "C" int pm_jpeg_decode_workspace(int n_intervals, int n_subseq, size_t* bytes) {
  if (n_intervals < 0 || n_subseq < 0) return PM_ESHAPE;
  if (!bytes) return PM_EINVAL;
  *bytes = parallel_ws(n_intervals, n_subseq).bytes;
  return PM_OK;
}

// the entropy stage parallel inside an interval + the inverse DCT: coefficients -> component planes.  Arguments as validated by the
// two entries below; ws: the layout of `workspace`
static int parallel_to_planes(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals,
                              const int* frames, int n_frames, const unsigned char* huff, int n_huff, const int* quant, int n_quant,
                              short* coef, unsigned char* planes, long blocks, const int* subseq, int n_subseq, int sync_rounds,
                              unsigned char* wsb, const ParallelWs& ws, hipStream_t s) {
  unsigned* counters = reinterpret_cast<unsigned*>(wsb);
  int* bad = reinterpret_cast<int*>(wsb + ws.bad);
  if (hipMemsetAsync(wsb, 0, ws.acc, s) != hipSuccess) return PM_ELAUNCH;  // the counters and bad[]
  if (n_frames > 0 && blocks > 0) {
    if (hipMemsetAsync(coef, 0, (size_t)blocks * 64 * sizeof(short), s) != hipSuccess) return PM_ELAUNCH;
    const HuffTable* t = reinterpret_cast<const HuffTable*>(huff);
    const unsigned* w = reinterpret_cast<const unsigned*>(entropy);
    const long n_words = entropy_bytes / 4;
    const bool lds = n_huff <= kLdsTables;
    if (n_subseq > 0) {
      uint4* acc = reinterpret_cast<uint4*>(wsb + ws.acc);
      uint4* tails = reinterpret_cast<uint4*>(wsb + ws.tails);
      unsigned* E = reinterpret_cast<unsigned*>(wsb + ws.e);
      unsigned* X = reinterpret_cast<unsigned*>(wsb + ws.x);
      unsigned* wgx = reinterpret_cast<unsigned*>(wsb + ws.wgx);
      const dim3 grid(ws.n_wg), block(kWg);
      for (int r = 0; r <= sync_rounds; ++r) {
        if (lds)
          hipLaunchKernelGGL(jpeg_sync_kernel<true>, grid, block, 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                             n_huff, blocks, subseq, n_subseq, r, ws.n_wg, E, X, acc, wgx, counters);
        else
          hipLaunchKernelGGL(jpeg_sync_kernel<false>, grid, block, 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                             n_huff, blocks, subseq, n_subseq, r, ws.n_wg, E, X, acc, wgx, counters);
      }
      hipLaunchKernelGGL(jpeg_verify_kernel, grid, block, 0, s, n_words, intervals, n_intervals, frames, n_frames, n_huff, blocks,
                         subseq, n_subseq, E, X, acc, tails, bad);
      if (lds)
        hipLaunchKernelGGL(jpeg_write_kernel<true>, grid, block, 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                           n_huff, blocks, subseq, n_subseq, E, acc, tails, bad, coef);
      else
        hipLaunchKernelGGL(jpeg_write_kernel<false>, grid, block, 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                           n_huff, blocks, subseq, n_subseq, E, acc, tails, bad, coef);
    }
    if (n_intervals > 0) {  // the sequential way out: intervals that are not converged (or have no subsequences)
      const dim3 grid((n_intervals + 63) / 64);
      if (lds)
        hipLaunchKernelGGL(jpeg_huff_kernel<true>, grid, dim3(64), 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                           n_huff, coef, blocks, bad, subseq, n_subseq, counters);
      else
        hipLaunchKernelGGL(jpeg_huff_kernel<false>, grid, dim3(64), 0, s, w, n_words, intervals, n_intervals, frames, n_frames, t,
                           n_huff, coef, blocks, bad, subseq, n_subseq, counters);
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, coef, planes, blocks, frames,
                       n_frames, quant, n_quant);
  }
  return PM_OK;
}

extern "C" int pm_jpeg_decode_parallel(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals,
                                       const int* frames, int n_frames, const unsigned char* huff, int n_huff, const int* quant,
                                       int n_quant, const unsigned char* fallback, long fallback_bytes,
                                       const long long* fallback_table, int n_fallback, short* coef, unsigned char* planes, long blocks,
                                       long pixels, unsigned char* out, long out_bytes, const int* subseq, int n_subseq,
                                       int sync_rounds, void* workspace, size_t ws_bytes, int* stats, void* stream) {
  if (n_intervals < 0 || n_frames < 0 || n_huff < 0 || n_quant < 0 || n_fallback < 0 || n_fallback > 65535 || entropy_bytes < 0 ||
      fallback_bytes < 0 || blocks < 0 || pixels < 0 || out_bytes < 0 || n_subseq < 0 || sync_rounds < 0 || sync_rounds > 8)
    return PM_ESHAPE;
  if (entropy_bytes % 16 != 0 || reinterpret_cast<uintptr_t>(entropy) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
    return PM_EALIGN;
  if ((n_frames > 0 || n_fallback > 0) && !out) return PM_EINVAL;
  if (n_frames > 0 && (!frames || (n_intervals > 0 && (!intervals || !entropy || !huff)) || (blocks > 0 && (!coef || !planes || !quant))))
    return PM_EINVAL;
  if (n_fallback > 0 && (!fallback_table || (fallback_bytes > 0 && !fallback))) return PM_EINVAL;
  if (n_subseq > 0 && (!subseq || !intervals || !entropy || !huff || n_intervals == 0)) return PM_EINVAL;
  const ParallelWs ws = parallel_ws(n_intervals, n_subseq);
  if (!workspace || ws_bytes < ws.bytes) return PM_EINVAL;
  hipStream_t s = pm_stream(stream);
  unsigned char* wsb = static_cast<unsigned char*>(workspace);
  const int st = parallel_to_planes(entropy, entropy_bytes, intervals, n_intervals, frames, n_frames, huff, n_huff, quant, n_quant, coef,
                                    planes, blocks, subseq, n_subseq, sync_rounds, wsb, ws, s);
  if (st != PM_OK) return st;
  if (n_frames > 0 && blocks > 0 && pixels > 0)
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, planes, blocks, frames, n_frames,
                       pixels, out, out_bytes);
  if (n_fallback > 0)
    hipLaunchKernelGGL(jpeg_copy_kernel, dim3(64, n_fallback), dim3(256), 0, s, fallback, fallback_bytes, fallback_table, out,
                       out_bytes);
  if (stats)
    hipLaunchKernelGGL(jpeg_stats_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<const unsigned*>(wsb), n_subseq, n_intervals, stats);
  if (hipGetLastError() != hipSuccess) return PM_ELAUNCH;
  return PM_OK;
}

extern "C" int pm_jpeg_decode_planes(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals,
                                     const int* frames, int n_frames, const unsigned char* huff, int n_huff, const int* quant,
                                     int n_quant, short* coef, unsigned char* planes, long blocks, const int* subseq, int n_subseq,
                                     int sync_rounds, void* workspace, size_t ws_bytes, int* stats, void* stream) {
  if (n_intervals < 0 || n_frames < 0 || n_huff < 0 || n_quant < 0 || entropy_bytes < 0 || blocks < 0 || n_subseq < 0 ||
      sync_rounds < 0 || sync_rounds > 8)
    return PM_ESHAPE;
  if (entropy_bytes % 16 != 0 || reinterpret_cast<uintptr_t>(entropy) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
    return PM_EALIGN;
  if (n_frames > 0 && (!frames || (n_intervals > 0 && (!intervals || !entropy || !huff)) || (blocks > 0 && (!coef || !planes || !quant))))
    return PM_EINVAL;
  if (n_subseq > 0 && (!subseq || !intervals || !entropy || !huff || n_intervals == 0)) return PM_EINVAL;
  const ParallelWs ws = parallel_ws(n_intervals, n_subseq);
  if (!workspace || ws_bytes < ws.bytes) return PM_EINVAL;
  hipStream_t s = pm_stream(stream);
  unsigned char* wsb = static_cast<unsigned char*>(workspace);
  const int st = parallel_to_planes(entropy, entropy_bytes, intervals, n_intervals, frames, n_frames, huff, n_huff, quant, n_quant, coef,
                                    planes, blocks, subseq, n_subseq, sync_rounds, wsb, ws, s);
  if (st != PM_OK) return st;
  if (stats)
    hipLaunchKernelGGL(jpeg_stats_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<const unsigned*>(wsb), n_subseq, n_intervals, stats);
  if (hipGetLastError() != hipSuccess) return PM_ELAUNCH;
  return PM_OK;
}
