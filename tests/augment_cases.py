"""The frames, factors, shapes and live-Pillow references of the input-pipeline edge tests (not a test module), shared by
tests/test_augment_edges_cpu.py (oracle/augment_ref.py against Pillow) and tests/test_gpu_augment_edges.py (csrc/pm_augment.hip against
Pillow, or against the oracle where Pillow has no such routine).  Pillow is called the way tests/golden/make_augment_fixtures.py calls it,
i.e. the way torchvision 0.10's functional_pil wrappers do.  Everything is compared as bytes / f32 bit patterns: no tolerance here."""
import itertools
import math

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter, ImageStat


def noise(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


# ---- ColorJitter -----------------------------------------------------------------------------------------------------------------
def all_colours():
    """uint8 [4096, 4096, 3]: every RGB value exactly once (R the slowest, B the fastest)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v & 255).astype(np.uint8)], -1).reshape(4096, 4096, 3)


# (hue factor, the uint8 shift np.uint8(factor * 255) it becomes): +-0.01 are the ends of the train transform's interval; shift 0 is the
# pure HSV round trip, which is not the identity; 128 is the far side of the wheel
HUE = ((0.0, 0), (0.005, 1), (0.01, 2), (0.503, 128), (-0.01, 254))
SATURATION = (0.0, 0.75, 0.8, 1.0, 1.2, 1.25, 2.0)
TWENTIETHS = tuple(k / 20 for k in range(41))   # both blend branches, both interval ends, the extrapolating side with its clamp;
#                                                 short decimals: the factors at which a fused multiply-add changes a byte


def hue_shift_of(factor):
    return int(np.int64(factor * 255)) & 0xFF   # functional_pil.adjust_hue: np.uint8(hue_factor * 255), a C cast that wraps


def pil_hsv(a):
    return np.asarray(Image.fromarray(a).convert("HSV"))


def pil_hue(a, shift):
    h, s, v = Image.fromarray(a).convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        nh += np.uint8(shift)
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))


def pil_brightness(a, f):
    return np.asarray(ImageEnhance.Brightness(Image.fromarray(a)).enhance(f))


def pil_contrast(a, f):
    return np.asarray(ImageEnhance.Contrast(Image.fromarray(a)).enhance(f))


def pil_saturation(a, f):
    return np.asarray(ImageEnhance.Color(Image.fromarray(a)).enhance(f))


def pil_jitter(a, order, brightness, contrast, saturation, hue):
    """One frame through the ops of `order` (0 brightness, 1 contrast, 2 saturation, 3 hue; -1 skips), each a Pillow call."""
    for op in order:
        if op == 0:
            a = pil_brightness(a, brightness)
        elif op == 1:
            a = pil_contrast(a, contrast)
        elif op == 2:
            a = pil_saturation(a, saturation)
        elif op == 3:
            a = pil_hue(a, hue_shift_of(hue))
    return a


def oracle_jitter(R, a, order, brightness, contrast, saturation, hue):
    x = a[None]
    for op in order:
        if op >= 0:
            x = (R.adjust_brightness, R.adjust_contrast, R.adjust_saturation, R.adjust_hue)[op](x, (brightness, contrast, saturation, hue)[op])
    return x[0]


def jitter_records(order, brightness, contrast, saturation, hue):
    """pm_aug_jitter records, int32 [B, 8], as DeviceAugmenter packs them; every argument per sample."""
    B = len(order)
    jit = np.zeros((B, 8), dtype=np.int32)
    jit[:, :4] = order
    jit[:, 4:7] = np.stack([np.asarray(v, dtype=np.float32) for v in (brightness, contrast, saturation)], 1).view(np.int32)
    jit[:, 7] = [hue_shift_of(float(h)) for h in hue]
    return jit


def brightness_frame():
    """uint8 [48, 64, 3]: all 256 values in every channel (a ramp, offset per channel), the rest noise."""
    a = noise((48 * 64, 3), 5)
    ramp = np.arange(256)
    a[:256] = np.stack([ramp, (ramp + 85) & 255, 255 - ramp], 1)
    return a.reshape(48, 64, 3)


CONTRAST_HW = (32, 64)


def _grey(values):
    return np.repeat(np.asarray(values, dtype=np.uint8).reshape(CONTRAST_HW + (1,)), 3, axis=2)   # r = g = b = v: rgb2l gives v


def grey_frame_with_sum(total):
    """A grey 32 x 64 frame whose 2048 luminances sum to `total`.  Where the sum allows it (a mean of 15.94 ... 239.06) the frame holds
    all 256 values: a ramp plus 1792 fillers of two neighbouring values; nearer the ends, three values m - d, m, m + d."""
    n = CONTRAST_HW[0] * CONTRAST_HW[1]
    fill = total - 32640
    if 0 <= fill <= 255 * (n - 256):
        q, rem = divmod(fill, n - 256)
        v = np.concatenate([np.arange(256), np.full(n - 256 - rem, q), np.full(rem, min(q + 1, 255))])
    else:
        m, rem = divmod(total, n)
        d = min(m, 255 - m)
        v = np.concatenate([np.full(n // 2, m), np.full(n // 4, m - d), np.full(n // 4, m + d)])
        v[:rem] += 1      # (rem pixels of m become m + 1; m < 255 wherever rem > 0)
    assert int(v.sum()) == total and v.min() >= 0 and v.max() <= 255
    # interleave, so that every 256-thread block of the luminance sum sees a mixture
    return _grey(v[np.random.Generator(np.random.PCG64(total)).permutation(n)])


def contrast_frames():
    """uint8 [264, 32, 64, 3]: for every degenerate value m = 0 ... 255 one grey frame whose mean luminance is exactly m, plus eight
    frames whose mean sits exactly on m + 1/2 (ImageStat's int(mean + 0.5) rounds it up) or one 2048th below it."""
    n = CONTRAST_HW[0] * CONTRAST_HW[1]
    sums = [m * n for m in range(256)] + [m * n + n // 2 - e for m in (17, 100, 201, 238) for e in (0, 1)]
    return np.stack([grey_frame_with_sum(s) for s in sums])


def pil_mean_luminance(a):
    im = Image.fromarray(a).convert("L")
    return int(ImageStat.Stat(im).mean[0] + 0.5)   # ImageEnhance.Contrast.__init__


def contrast_coverage(frames):
    """(the set of degenerate values that occur, the set of those that occur in a frame holding all 256 pixel values), by Pillow."""
    means = [pil_mean_luminance(f) for f in frames]
    full = {m for m, f in zip(means, frames) if len(np.unique(f)) == 256}
    return set(means), full


# all 24 orders of the four ops, one per sample, so that 0, 1, 2 and 3 ops run before the contrast inside the luminance pre-pass; then the
# evaluation rows' order, an order without contrast (the pre-pass returns early) and all-skip (identity), each for a whole batch
PERMUTATIONS = tuple(itertools.permutations(range(4)))
EXTRA_ORDERS = ((0, 1, -1, -1), (0, 2, 3, -1), (-1, -1, -1, -1), (-1, 1, -1, 0))
ORDER_HW = ((37, 53), (1, 1), (5, 7))   # odd; one pixel; fewer pixels than one workgroup has threads


def order_factors(B):
    """Short decimal factors per sample, both sides of 1 for every blend."""
    b = [(0.6, 0.7, 1.3, 1.4, 0.85)[i % 5] for i in range(B)]
    c = [(0.7, 1.45, 0.6, 1.3, 0.55, 1.15, 0.9)[i % 7] for i in range(B)]
    s = [(0.8, 1.2, 0.9, 1.1)[i % 4] for i in range(B)]
    h = [(0.01, -0.01, 0.005, 0.0)[(i // 2) % 4] for i in range(B)]
    return b, c, s, h


# ---- GaussianBlur (torchvision's tensor path: no Pillow routine; the oracle is the reference) -----------------------------------------
BLUR_HW = ((13, 13), (13, 40), (40, 13), (14, 15))   # 13: the smallest legal side for 25 taps -- every tap of a border pixel reflects
BLUR_SIGMAS = (0.001, 0.1, 2.0, 10.0)
BLUR_KSIZES = (25, 3, 1)


def blur_batch(H, W):
    """uint8 [6, H, W, 3] and the per-sample sigmas: four noise frames, a frame of zeros and a frame of 255 (the f32 taps do not sum to
    exactly 1: the rint and the clamp decide)."""
    x = noise((6, H, W, 3), 100 * H + W)
    x[4], x[5] = 0, 255
    return x, BLUR_SIGMAS + (2.0, 10.0)


# ---- flips + rotation ----------------------------------------------------------------------------------------------------------------
GEOM_HW = ((29, 13), (13, 29), (1, 7), (7, 1), (2, 2), (97, 131))
ANGLES = (0.0, 90.0, -90.0, 270.0, 180.0, -180.0, 45.0, 135.0, 0.001, -0.001, 89.999, 90.001, 179.999, 360.0, -360.0, 450.0, 33.3, -123.4)
GEOM_MEAN, GEOM_STD = (0.31, 0.52, 0.73), (0.11, 0.27, 0.43)   # not ImageNet's, different per channel


def geom_cases():
    """(angle, flips) per sample: every angle under every flip combination (bit 0 horizontal, bit 1 vertical)."""
    return [(a, f) for a in ANGLES for f in range(4)]


def pil_flip_rotate(a, angle, flips):
    if flips & 1:
        a = a[:, ::-1]
    if flips & 2:
        a = a[::-1]
    return np.asarray(Image.fromarray(np.ascontiguousarray(a)).rotate(angle, Image.NEAREST, expand=False, center=None, fillcolor=0))


def oracle_flip_rotate(R, a, angle, flips):
    if flips & 1:
        a = a[:, ::-1]
    if flips & 2:
        a = a[::-1]
    return R.rotate_nearest(np.ascontiguousarray(a)[None], angle)[0]


# ---- resampling -----------------------------------------------------------------------------------------------------------------------
# (Hs, Ws, out): from one pixel / one line, many taps, just above and at twice the output, one axis unchanged
RESIZE = ((1, 1, 224), (1, 5, 224), (5, 1, 224), (2, 3, 224), (3, 2, 32), (1500, 2000, 224), (225, 223, 224), (447, 449, 224),
          (448, 448, 224), (224, 300, 224), (300, 224, 224))
CROP_HW = (300, 400)
CROP_BOXES = ((0, 0, 1, 1), (299, 399, 1, 1), (0, 0, 300, 1), (0, 0, 1, 400), (0, 0, 300, 400), (150, 200, 2, 3), (10, 10, 224, 224),
              (7, 9, 225, 223))   # (top, left, h, w)
CROP_OUT = (224, 16)   # the whole frame at 16: the largest tap count the workspace formula has to hold
RAGGED_HW = ((1, 1), (300, 400), (17, 250), (250, 17))
_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def coeff_pairs():
    """(in, out) of every axis of RESIZE and of the crops."""
    pairs = {(n, out) for (h, w, out) in RESIZE for n in (h, w)}
    pairs |= {(n, out) for (_, _, h, w) in CROP_BOXES for n in (h, w) for out in CROP_OUT}
    return sorted(pairs)


def pil_resize(a, out_h, out_w, filt="bilinear"):
    return np.asarray(Image.fromarray(a).resize((out_w, out_h), _FILTER[filt]))


def pil_resized_crop(a, box, out, filt):
    t, l, h, w = (int(v) for v in box)
    return np.asarray(Image.fromarray(a).crop((l, t, l + w, t + h)).resize((out, out), _FILTER[filt]))


def drawn_boxes(B, H, W, seed):
    """B crop boxes inside an H x W frame, any aspect (not RandomResizedCrop's distribution: the kernels take any box), the last one the
    whole frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h, w = rng.integers(1, H + 1, B), rng.integers(1, W + 1, B)
    boxes = np.stack([rng.integers(0, H - h + 1), rng.integers(0, W - w + 1), h, w], 1).astype(np.int32)
    boxes[-1] = (0, 0, H, W)
    return boxes


# Image.resize runs the VERTICAL pass first when the frame is more than 100 times as tall as wide and the height shrinks (found by
# bisection against Pillow 12.2: tests/test_augment_edges_cpu.py); otherwise horizontal first.  (Hs, Ws, out_h, out_w), each with the
# order Pillow takes there: the last shapes on the horizontal-first side, the first on the other.
ORDER_EDGE = (((3000, 30, 224, 224), "h"), ((3001, 30, 224, 224), "v"), ((900, 9, 224, 224), "h"), ((901, 9, 224, 224), "v"),
              ((200, 2, 16, 16), "h"), ((201, 2, 16, 16), "v"), ((30, 4000, 224, 224), "h"), ((9, 1200, 224, 224), "h"),
              ((300, 2, 300, 224), "h"), ((300, 2, 301, 16), "h"), ((300, 2, 299, 16), "v"))


# ---- flat-grid wrap: more than 8192 x 256 = 2,097,152 outputs per launch --------------------------------------------------------------
WRAP_HW = (1024, 704)   # x 3 frames = 2,162,688 pixels
WRAP_ANGLES = ((33.3, 1), (90.0, 2), (-123.4, 3))   # (angle, flips); 90 degrees on a non-square frame: the fixed-point path
WRAP_BOX_SIGMAS = (1.5, None, 12.0)    # None: the sample is copied (radius < 0)
WRAP_RESIZE = (700, 900, 1024)


def pil_gaussian_blur(a, sigma):
    return np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=sigma)))


def assert_same_bytes(got, want, what):
    """np.array_equal with a report that says where and how much."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at {i}: got {got[i]}, want {want[i]}")


def f32_bits(t):
    """f32 array -> its bit patterns (so that -0.0 != 0.0 and a NaN equals itself)."""
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view(np.int32)


assert math.isclose(TWENTIETHS[12], 0.6)
