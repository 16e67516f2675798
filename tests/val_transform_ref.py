"""The validation transform of the MAE recipes -- torchvision's Resize(resize, bicubic) + CenterCrop(crop) on a PIL image, as
mae_recipe._ValFrames runs it -- restated in numpy the way the device computes it (csrc/pm_augment.hip, center_crop_*): Pillow's
Resample.c 8bpc bicubic taps are built for the FULL resized size (nw, nh), only the window's `crop` columns and rows are evaluated,
and the horizontal pass is rounded to uint8 before the vertical pass.  The resized nw x nh frame never exists; the result is
Image.resize((nw, nh), BICUBIC).crop(window) byte for byte (tests/test_val_transform_cpu.py holds it to Pillow with ==, and shows
that each of the five `variant`s below -- plausible mistakes -- differs from Pillow on at least one shape).

SMALL / LARGE: the (h, w, resize, crop) shapes the tests run."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2

SMALL = [(37, 53, 32, 28), (53, 37, 32, 28), (32, 32, 32, 28), (32, 41, 32, 28), (20, 70, 32, 28), (300, 17, 32, 28), (64, 65, 32, 27),
         (33, 32, 32, 29), (7, 9, 32, 32)]
LARGE = [(375, 500, 256, 224), (100, 300, 256, 224), (257, 256, 256, 224), (1080, 1350, 256, 224)]
VARIANTS = ("taps_for_crop_size", "window_from_zero", "offset_half_up", "round_long_side", "vertical_first")


def noise_frame(h: int, w: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def window(h: int, w: int, resize: int, crop: int, variant: str = None):
    """(nh, nw, top, left): torchvision Resize(int) acts on the shorter side, the other is int(resize * other / shorter) (truncated;
    no resize when the shorter side already equals `resize`); center_crop's origin is int(round((n - crop) / 2.0)), Python's
    round-half-to-even."""
    nh, nw = h, w
    if (w <= h and w != resize) or (h <= w and h != resize):
        long_side = (lambda v: int(round(v))) if variant == "round_long_side" else int
        nh, nw = (long_side(resize * h / w), resize) if w <= h else (resize, long_side(resize * w / h))
    if variant == "offset_half_up":
        return nh, nw, int(np.floor((nh - crop) / 2.0 + 0.5)), int(np.floor((nw - crop) / 2.0 + 0.5))
    return nh, nw, int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def taps(in_size: int, out_size: int, first: int, count: int):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the output indices first .. first + count - 1 of an axis resampled
    from in_size to out_size -> [(xmin, int taps [n])], in the C source's double arithmetic."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        out.append((xmin, np.array(k, dtype=np.int64)))
    return out


def _clip8(ss: np.ndarray) -> np.ndarray:
    return np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(img: np.ndarray, table, axis: int) -> np.ndarray:
    """One 8bpc pass along axis 0 (vertical) or 1 (horizontal) of an [H, W, 3] image: one output line per table entry."""
    img = img.astype(np.int64)
    lines = []
    for lo, k in table:
        src = img[lo:lo + len(k)] if axis == 0 else img[:, lo:lo + len(k)]
        kk = k[:, None, None] if axis == 0 else k[None, :, None]
        lines.append(_clip8((1 << (PRECISION_BITS - 1)) + (src * kk).sum(axis=axis)))
    return np.stack(lines, axis=axis)


def resize_center_crop(frame: np.ndarray, resize: int, crop: int, variant: str = None) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [crop, crop, 3].  variant: None (Pillow's result) or one of VARIANTS."""
    h, w = frame.shape[:2]
    nh, nw, top, left = window(h, w, resize, crop, variant)
    if variant == "taps_for_crop_size":      # the taps of a resize to crop x crop
        tx, ty = taps(w, crop, 0, crop), taps(h, crop, 0, crop)
    elif variant == "window_from_zero":      # the taps of the first `crop` outputs instead of the window's
        tx, ty = taps(w, nw, 0, crop), taps(h, nh, 0, crop)
    else:
        tx, ty = taps(w, nw, left, crop), taps(h, nh, top, crop)
    if variant == "vertical_first":
        return _pass(_pass(frame, ty, 0), tx, 1)
    # only the source rows the window's vertical taps read go through the horizontal pass
    row0, row1 = ty[0][0], ty[-1][0] + len(ty[-1][1])
    mid = _pass(frame[row0:row1], tx, 1)
    return _pass(mid, [(lo - row0, k) for lo, k in ty], 0)


def pillow_resize_center_crop(frame: np.ndarray, resize: int, crop: int) -> np.ndarray:
    """mae_recipe._ValFrames.__getitem__ on a decoded frame: the authority."""
    from PIL import Image
    img = Image.fromarray(frame)
    w, h = img.size
    if (w <= h and w != resize) or (h <= w and h != resize):
        nw, nh = (resize, int(resize * h / w)) if w <= h else (int(resize * w / h), resize)
        img = img.resize((nw, nh), Image.BICUBIC)
        w, h = nw, nh
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    return np.asarray(img.crop((left, top, left + crop, top + crop)))
