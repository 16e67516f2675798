"""References for ssl4polyp_amd/timm_aug.py and csrc/pm_timm_aug.hip.  TEST INFRASTRUCTURE ONLY.

  pil_apply   one RandAugment op done by Pillow's own calls, exactly as timm's auto_augment.py makes them: the yardstick.
  np_apply    the DEVICE arithmetic of the same op restated in numpy from a pm_randaug_op record (integers, f32 blends, f64
              bicubic, nothing fused: numpy rounds after every operation).  tests/test_randaug_cpu.py holds it to pil_apply byte
              for byte and shows that three wrong variants do not pass; the GPU tests hold the kernels to pil_apply directly.
  erase_*     the words and the float64 Box-Muller normals of pm_random_erase_f32."""
import math

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

from oracle.noise_ref import philox4x32_10
from ssl4polyp_amd import timm_aug as TA

FILL = (124, 116, 104)   # min(255, round(255 * mean)) of the ImageNet mean
ERASE_SEED, ERASE_COUNTER = 0x0123456789ABCDEF, (7 << 32) | 11   # the fixed key of the erasing tests (checked on the CPU first)


# ------------------------------------------------------------------------------------------------------------ Pillow itself
def pil_apply(frame: np.ndarray, name: str, arg=None, fill=FILL) -> np.ndarray:
    """frame uint8 [H, W, 3] -> the op `name` (timm's names; "TranslateX" / "TranslateY" take pixels, the "Rel" forms a fraction of
    the side) by the calls of timm 0.4.12 auto_augment.py with resample = BICUBIC and fillcolor = fill."""
    img = Image.fromarray(frame, "RGB")
    kw = dict(resample=Image.BICUBIC, fillcolor=tuple(fill))
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    if base == "Identity":
        out = img
    elif base == "AutoContrast":
        out = ImageOps.autocontrast(img)
    elif base == "Equalize":
        out = ImageOps.equalize(img)
    elif base == "Invert":
        out = ImageOps.invert(img)
    elif base == "Posterize":
        out = img if arg >= 8 else ImageOps.posterize(img, arg)
    elif base == "Solarize":
        out = ImageOps.solarize(img, arg)
    elif base == "SolarizeAdd":
        lut = [min(255, i + arg) if i < 128 else i for i in range(256)]
        out = img.point(lut + lut + lut)
    elif base in ("Color", "Contrast", "Brightness", "Sharpness"):
        out = getattr(ImageEnhance, base)(img).enhance(arg)
    elif base == "ShearX":
        out = img.transform(img.size, Image.AFFINE, (1, arg, 0, 0, 1, 0), **kw)
    elif base == "ShearY":
        out = img.transform(img.size, Image.AFFINE, (1, 0, 0, arg, 1, 0), **kw)
    elif base in ("TranslateX", "TranslateXRel"):
        out = img.transform(img.size, Image.AFFINE, (1, 0, arg * img.size[0] if base.endswith("Rel") else arg, 0, 1, 0), **kw)
    elif base in ("TranslateY", "TranslateYRel"):
        out = img.transform(img.size, Image.AFFINE, (1, 0, 0, 0, 1, arg * img.size[1] if base.endswith("Rel") else arg), **kw)
    elif base == "Rotate":
        out = img.rotate(arg, **kw)
    else:
        raise ValueError(name)
    return np.asarray(out).copy()


def pil_sequence(frame: np.ndarray, steps, hflip=False, fill=FILL) -> np.ndarray:
    """timm's order: RandomHorizontalFlip, then the ops of `steps` = [(name, arg), ...]."""
    if hflip:
        frame = np.asarray(Image.fromarray(frame, "RGB").transpose(Image.FLIP_LEFT_RIGHT)).copy()
    for name, arg in steps:
        frame = pil_apply(frame, name, arg, fill)
    return frame


# ------------------------------------------------------------------------------------------------ the device arithmetic in numpy
def _rgb2l(f):
    f = f.astype(np.int64)
    return (f[..., 0] * 19595 + f[..., 1] * 38470 + f[..., 2] * 7471 + 0x8000) >> 16


def _blend(deg, img, a):
    """Blend.c ImagingBlend(degenerate, image, alpha) in C float: truncation inside [0, 1], clipping outside."""
    a = np.float32(a)
    d, v = deg.astype(np.float32), img.astype(np.float32)
    t = d + a * (v - d)
    assert t.dtype == np.float32
    if 0.0 <= a <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def _smooth(f):
    """Filter.c ImagingFilter3x3 with ImageFilter.SMOOTH: kernel / 13 in float, sum from offset + 0.5 over the row below, the row,
    the row above; border copied."""
    k1, k5 = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    v = f.astype(np.float32)
    out = f.copy()
    if f.shape[0] < 3 or f.shape[1] < 3:
        return out
    ss = np.full(v[1:-1, 1:-1].shape, np.float32(0.5), dtype=np.float32)
    for rows, mid in ((slice(2, None), k1), (slice(1, -1), k5), (slice(0, -2), k1)):
        r = v[rows]
        ss = ss + ((r[:, :-2] * k1 + r[:, 1:-1] * mid) + r[:, 2:] * k1)
    assert ss.dtype == np.float32
    out[1:-1, 1:-1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int64))).astype(np.uint8)
    return out


def _fma(a, b, c):
    """a * b + c with ONE rounding to f64 (product and sum held in x87 extended precision first): what a contracted build does."""
    return (np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble) + np.asarray(c, np.longdouble)).astype(np.float64)


def _bicubic(v1, v2, v3, v4, d, fused):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    if fused:
        return _fma(d, _fma(d, _fma(d, p4, p3), p2), p1)
    return p1 + d * (p2 + d * (p3 + d * p4))


def _affine(f, a, fill, variant):
    """Geometry.c ImagingGenericTransform + affine_transform + bicubic_filter32RGB, all double."""
    H, W, _ = f.shape
    half = 0.0 if variant == "no_half" else 0.5
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + half, np.arange(H, dtype=np.float64) + half)
    xin = a[0] * xs + a[1] * ys + a[2]
    yin = a[3] * xs + a[4] * ys + a[5]
    inside = ~((xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - x, yin - y
    x, y = x - 1, y - 1
    cols = [np.clip(x + i, 0, W - 1) for i in range(4)]
    v = f.astype(np.float64)
    out = np.empty_like(f)
    out[...] = np.asarray(fill, dtype=np.uint8)
    fused = variant == "fma"
    for c in range(3):
        ch = v[..., c]
        rows = []
        for r in range(4):
            yy = y + r
            ok = (yy >= 0) & (yy < H)
            yc = np.clip(yy, 0, H - 1)
            val = _bicubic(ch[yc, cols[0]], ch[yc, cols[1]], ch[yc, cols[2]], ch[yc, cols[3]], dx, fused)
            rows.append(val if r == 0 else np.where(ok, val, rows[r - 1]))
        t = _bicubic(rows[0], rows[1], rows[2], rows[3], dy, fused)
        px = np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, t.astype(np.int64))).astype(np.uint8)
        out[..., c] = np.where(inside, px, out[..., c])
    return out


def _lut(rec, hist, variant):
    op, iarg = int(rec["op"]), int(rec["iarg"])
    i = np.arange(256, dtype=np.int64)
    if op == TA.OP_INVERT:
        one = 255 - i
    elif op == TA.OP_POSTERIZE:
        one = i & ~((1 << (8 - min(max(iarg, 0), 8))) - 1)
    elif op == TA.OP_SOLARIZE:
        one = np.where(i < iarg, i, 255 - i)
    elif op == TA.OP_SOLARIZE_ADD:
        one = np.where(i < 128, np.minimum(255, i + iarg), i)
    else:
        lut = np.empty((3, 256), dtype=np.int64)
        for c in range(3):
            h = hist[c]
            nz = np.nonzero(h)[0]
            if op == TA.OP_AUTOCONTRAST:
                lo, hi = int(nz[0]), int(nz[-1])
                if hi <= lo:
                    lut[c] = i
                else:
                    scale = 255.0 / (hi - lo)
                    offset = -lo * scale
                    lut[c] = np.clip((i.astype(np.float64) * scale + offset).astype(np.int64), 0, 255)
            else:   # Equalize
                step = (int(h.sum()) - int(h[nz[-1]])) // 255
                if len(nz) <= 1 or step == 0:
                    lut[c] = i
                else:
                    n = 0 if variant == "equalize_no_half_step" else step // 2
                    for k in range(256):
                        lut[c, k] = min(255, n // step)
                        n += int(h[k])
        return lut
    return np.stack([one, one, one])


def np_apply(frame: np.ndarray, rec, fill=FILL, hflip=False, variant=None) -> np.ndarray:
    """What pm_randaug_stats + pm_randaug_apply compute for one frame and one pm_randaug_op record.  variant: None, or a WRONG
    variant the CPU tests show to differ from Pillow: "no_half" (source coordinate without the + 0.5), "fma" (bicubic polynomial
    with fused multiply-adds), "equalize_no_half_step" (n starts at 0)."""
    f = frame[:, ::-1].copy() if hflip else frame
    op = int(rec["op"])
    H, W, _ = f.shape
    if op in (TA.OP_AUTOCONTRAST, TA.OP_EQUALIZE, TA.OP_INVERT, TA.OP_POSTERIZE, TA.OP_SOLARIZE, TA.OP_SOLARIZE_ADD):
        hist = [np.bincount(f[..., c].reshape(-1), minlength=256) for c in range(3)]
        lut = _lut(rec, hist, variant)
        return np.stack([lut[c][f[..., c]] for c in range(3)], axis=-1).astype(np.uint8)
    if op in (TA.OP_COLOR, TA.OP_CONTRAST, TA.OP_BRIGHTNESS, TA.OP_SHARPNESS):
        if op == TA.OP_COLOR:
            deg = np.repeat(_rgb2l(f)[..., None], 3, axis=-1)
        elif op == TA.OP_CONTRAST:
            deg = np.full(f.shape, int(float(int(_rgb2l(f).sum())) / float(H * W) + 0.5), dtype=np.int64)
        elif op == TA.OP_BRIGHTNESS:
            deg = np.zeros(f.shape, dtype=np.int64)
        else:
            deg = _smooth(f)
        return _blend(deg, f, rec["farg"])
    if op == TA.OP_AFFINE:
        return _affine(f, [float(v) for v in rec["a"]], fill, variant)
    if op == TA.OP_TRANSPOSE:
        mode = int(rec["iarg"])
        if mode == 2:
            return f[::-1, ::-1].copy()
        if mode in (3, 4) and H == W:
            return np.rot90(f, k=1 if mode == 3 else 3).copy()
    return f.copy()


def np_sequence(frame, records, fill=FILL, hflip=False):
    for l, rec in enumerate(records):
        frame = np_apply(frame, rec, fill, hflip and l == 0)
    if hflip and not len(records):
        frame = frame[:, ::-1].copy()
    return frame


# ------------------------------------------------------------------------------------------------------------------ frames
def frames(h: int, w: int):
    """name -> uint8 [h, w, 3]: random, constant, two-level, ramp, and a frame with a constant channel and one outlier pixel."""
    rng = np.random.RandomState(1000 * h + w)
    out = {"random": rng.randint(0, 256, (h, w, 3)).astype(np.uint8),
           "constant": np.broadcast_to(np.array([37, 200, 101], np.uint8), (h, w, 3)).copy()}
    two = np.zeros((h, w, 3), np.uint8)
    two[:, w // 3:] = (255, 180, 3)
    two[h // 2:, :, 2] = 250
    out["two_level"] = two
    ramp = np.zeros((h, w, 3), np.uint8)
    ramp[..., 0] = (np.arange(w) * 255 // max(w - 1, 1))[None, :]
    ramp[..., 1] = (np.arange(h) * 255 // max(h - 1, 1))[:, None]
    ramp[..., 2] = ((np.arange(w)[None, :] + np.arange(h)[:, None]) * 3) % 256
    out["ramp"] = ramp
    outlier = rng.randint(90, 130, (h, w, 3)).astype(np.uint8)
    outlier[..., 1] = 77                     # a constant channel
    outlier[h // 2, w // 2, 0] = 255         # one outlier pixel
    outlier[1, 2, 2] = 0
    out["outlier"] = outlier
    return out


def op_cases(w: int, h: int):
    """(name, arg) for every op at the arguments the level functions can reach at their ends and at m = 9, and a few beside."""
    cases = [("Identity", None), ("AutoContrast", None), ("Equalize", None), ("Invert", None)]
    cases += [("Rotate", a) for a in (0, 0.3, -0.3, 27, -27, 30, -30, 90, 180)]
    cases += [(n, a) for n in ("ShearX", "ShearY") for a in (0, 0.27, -0.27, 0.3, -0.3)]
    cases += [(n, a) for n in ("TranslateXRel", "TranslateYRel") for a in (0, 0.405, -0.405, 0.45, -0.45)]
    cases += [("Posterize", b) for b in (0, 1, 4)] + [("Solarize", t) for t in (0, 26, 256)]
    cases += [("SolarizeAdd", a) for a in (0, 99, 110)]
    cases += [(n, f) for n in ("Color", "Contrast", "Brightness", "Sharpness") for f in (0.1, 0.19, 1.0, 1.81, 1.9)]
    return cases


# ------------------------------------------------------------------------------------------------------------------ erasing
def erase_words(seed: int, counter: int, sid: int, n: int):
    """uint32 [n, 2]: the word pair (w0, w1) behind normal e = 0 .. n - 1 of stream sid (include/polypmae.h pm_random_erase_f32)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10([q, np.full_like(q, sid), np.full_like(q, counter & 0xFFFFFFFF), np.full_like(q, (counter >> 32) & 0xFFFFFFFF)],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    w = np.stack(w, axis=1)                                   # [blocks, 4]
    pairs = np.repeat(w.reshape(-1, 2, 2), 2, axis=1)         # element 4 q + j reads pair j // 2
    return pairs.reshape(-1, 2)[:n]


def erase_normals64(seed: int, counter: int, sid: int, n: int):
    """float64 Box-Muller of the same words -> (z, radius): z[e] = sqrt(-2 ln u1) * (cos, sin)[e % 2](2 pi u2)."""
    w = erase_words(seed, counter, sid, n)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * math.pi * u2
    odd = (np.arange(n) & 1).astype(bool)
    return np.where(odd, rad * np.sin(ang), rad * np.cos(ang)), rad
