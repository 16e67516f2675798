"""The two stages of timm's training transform the MAE fine-tune recipe uses beyond crop / flip / normalise
(mae/util/datasets.py:37-47: create_transform(is_training=True, auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic',
re_prob=0.25, re_mode='pixel', re_count=1)): RandAugment on the cropped uint8 frames and RandomErasing on the normalised tensor.
The host draws what is random and per sample -- which ops, their arguments, the boxes -- into small record arrays; the pixels
are touched on the device only (csrc/pm_timm_aug.hip: pm_randaug_stats / pm_randaug_apply / pm_random_erase_f32), byte for byte
what Pillow does for the same record (tests/randaug_ref.py).

The PROTOCOL -- which ops exist, their probabilities, how a magnitude becomes an argument, how the erasing boxes are found -- is
timm 0.4.12's auto_augment.py and random_erasing.py RESTATED from their published source.  timm is not installed where this was
written, so, like mixup.Mixup's draw order, it has not been checked against timm itself: tests/test_randaug_cpu.py pins it to
hand-computed values.  timm draws from Python's `random` and numpy's global generator inside DataLoader workers; those streams
are not reproduced.  Here every draw of an epoch comes from one numpy RandomState seeded from (seed, epoch) (TrainAugment.reseed),
in the fixed order documented at RandAugment.draw and RandomErasing.draw, so a resumed run continues as the uninterrupted one."""
from __future__ import annotations

import math
import re
from typing import Optional, Sequence

import numpy as np

# csrc/pm_timm_aug.hip op ids (include/polypmae.h pm_randaug_op)
OP_IDENTITY, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD = 0, 1, 2, 3, 4, 5, 6
OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS, OP_SHARPNESS, OP_AFFINE, OP_TRANSPOSE = 7, 8, 9, 10, 11, 12
STATS_OPS = (OP_AUTOCONTRAST, OP_EQUALIZE, OP_CONTRAST)   # need pm_randaug_stats first
OP_DTYPE = np.dtype([("op", "<i4"), ("iarg", "<i4"), ("farg", "<f4"), ("reserved", "<i4"), ("a", "<f8", (6,))])   # pm_randaug_op
assert OP_DTYPE.itemsize == 64

MAX_LEVEL = 10.0   # auto_augment._MAX_LEVEL
# auto_augment._RAND_TRANSFORMS and _RAND_INCREASING_TRANSFORMS: the same fifteen slots, six of them "Increasing" with inc1
RAND_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
                   "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RAND_INCREASING_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing",
                              "SolarizeAdd", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing",
                              "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
TRANSLATE_PCT = 0.45   # hparams.get('translate_pct', 0.45)
_SIGNED = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "ColorIncreasing", "ContrastIncreasing",
           "BrightnessIncreasing", "SharpnessIncreasing")   # ops whose level function calls _randomly_negate


def level_to_arg(name: str, magnitude: float, negate: bool = False):
    """auto_augment's level functions: the op's argument at this magnitude (already clipped to [0, 10]); `negate` is the outcome of
    _randomly_negate for the ops that have a sign.  Translations come back as a FRACTION of the frame side."""
    level = magnitude / MAX_LEVEL
    sign = -1.0 if negate else 1.0
    if name == "Rotate":
        return sign * (level * 30.0)
    if name in ("ShearX", "ShearY"):
        return sign * (level * 0.3)
    if name in ("TranslateXRel", "TranslateYRel"):
        return sign * (level * TRANSLATE_PCT)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return level * 1.8 + 0.1
    if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        return 1.0 + sign * (level * 0.9)
    if name == "Posterize":
        return int(level * 4)
    if name == "PosterizeIncreasing":
        return 4 - int(level * 4)
    if name == "Solarize":
        return int(level * 256)
    if name == "SolarizeIncreasing":
        return 256 - int(level * 256)
    if name == "SolarizeAdd":
        return int(level * 110)
    if name in ("AutoContrast", "Equalize", "Invert", "Identity"):
        return None
    raise ValueError(f"unknown RandAugment op {name!r}")


def rotation_matrix(angle_deg: float, w: int, h: int):
    """Image.rotate(angle, expand=False, center=None, translate=None): ("transpose", mode) for its early returns (0 -> mode 1 =
    copy, 180 -> 2, 90 / 270 on a square frame -> 3 / 4), else ("affine", the six coefficients) computed as Image.rotate does --
    sin / cos rounded to 15 decimals, the centre carried through the matrix."""
    ang = angle_deg % 360.0
    if ang == 0:
        return "transpose", 1
    if ang == 180:
        return "transpose", 2
    if ang in (90, 270) and w == h:
        return "transpose", 3 if ang == 90 else 4
    rad = -math.radians(ang)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    cx, cy = w / 2, h / 2
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return "affine", m


def op_record(name: str, arg, w: int, h: int) -> np.ndarray:
    """One pm_randaug_op (a 0-d record of OP_DTYPE) for the timm op `name` with its level argument on a w x h frame.  `name` is
    one of RAND_TRANSFORMS / RAND_INCREASING_TRANSFORMS (an "Increasing" op is the same pixel routine), "Identity", or
    "TranslateX" / "TranslateY" with the shift in pixels."""
    rec = np.zeros((), dtype=OP_DTYPE)
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    affine = None
    if base == "Identity":
        rec["op"] = OP_IDENTITY
    elif base in ("AutoContrast", "Equalize", "Invert"):
        rec["op"] = {"AutoContrast": OP_AUTOCONTRAST, "Equalize": OP_EQUALIZE, "Invert": OP_INVERT}[base]
    elif base == "Posterize":   # auto_augment.posterize: bits_to_keep >= 8 returns the image
        rec["op"], rec["iarg"] = (OP_IDENTITY, 0) if int(arg) >= 8 else (OP_POSTERIZE, int(arg))
    elif base == "Solarize":
        rec["op"], rec["iarg"] = OP_SOLARIZE, int(arg)
    elif base == "SolarizeAdd":
        rec["op"], rec["iarg"] = OP_SOLARIZE_ADD, int(arg)
    elif base in ("Color", "Contrast", "Brightness", "Sharpness"):
        rec["op"] = {"Color": OP_COLOR, "Contrast": OP_CONTRAST, "Brightness": OP_BRIGHTNESS, "Sharpness": OP_SHARPNESS}[base]
        rec["farg"] = np.float32(arg)   # Image.blend takes a C float
    elif base == "ShearX":
        affine = (1.0, float(arg), 0.0, 0.0, 1.0, 0.0)
    elif base == "ShearY":
        affine = (1.0, 0.0, 0.0, float(arg), 1.0, 0.0)
    elif base in ("TranslateXRel", "TranslateX"):
        affine = (1.0, 0.0, float(arg) * w if base.endswith("Rel") else float(arg), 0.0, 1.0, 0.0)
    elif base in ("TranslateYRel", "TranslateY"):
        affine = (1.0, 0.0, 0.0, 0.0, 1.0, float(arg) * h if base.endswith("Rel") else float(arg))
    elif base == "Rotate":
        kind, val = rotation_matrix(float(arg), w, h)
        if kind == "affine":
            affine = val
        elif val == 1:
            rec["op"] = OP_IDENTITY
        else:
            rec["op"], rec["iarg"] = OP_TRANSPOSE, val
    else:
        raise ValueError(f"unknown RandAugment op {name!r}")
    if affine is not None:
        rec["op"], rec["a"] = OP_AFFINE, affine
    return rec


class RandAugment:
    """timm's rand_augment_transform(config_str, hparams) for 'rand-m<int>[-n<int>][-mstd<float>][-inc1]': n ops per image (default
    2) drawn with replacement and uniform weights from the fifteen of _RAND_TRANSFORMS (inc1: _RAND_INCREASING_TRANSFORMS), each
    applied with probability 0.5 at magnitude gauss(m, mstd) clipped to [0, 10]; fill colour min(255, round(255 mean)) per channel.
    Restated from timm 0.4.12; NOT checked against timm itself (see the module docstring).

    Refused, naming the gap: `w<int>` (weighted choice), `inc0` (timm reads it as bool("0"), i.e. True -- not decidable here
    without timm), any other key, mstd = inf (uniform magnitudes), an interpolation other than bicubic."""

    def __init__(self, config_str: str, img_mean: Sequence[float], interpolation: str = "bicubic"):
        if interpolation != "bicubic":
            raise NotImplementedError(f"RandAugment interpolation {interpolation!r}: only Pillow's bicubic transform filter is built "
                                      "(bilinear / random interpolation inside the policy is not)")
        parts = config_str.split("-")
        if parts[0] != "rand":
            raise NotImplementedError(f"auto-augment policy {config_str!r}: only RandAugment ('rand-...') is built, not AutoAugment "
                                      "or AugMix")
        self.magnitude, self.num_layers, self.magnitude_std, self.increasing = MAX_LEVEL, 2, 0.0, False
        for c in parts[1:]:
            cs = re.split(r"(\d.*)", c)
            if len(cs) < 2:
                continue   # (timm skips a section without a number)
            key, val = cs[:2]
            if key == "mstd":
                self.magnitude_std = float(val)
                if math.isinf(self.magnitude_std):
                    raise NotImplementedError("RandAugment mstd = inf (uniform magnitudes) is not built")
            elif key == "inc":
                if val != "1":
                    raise NotImplementedError(f"RandAugment 'inc{val}': timm reads it as bool({val!r}); only 'inc1' (or no inc key) "
                                              "is taken here")
                self.increasing = True
            elif key == "m":
                self.magnitude = int(val)
            elif key == "n":
                self.num_layers = int(val)
            elif key == "w":
                raise NotImplementedError("RandAugment 'w<int>' (weighted op choice) is not built")
            else:
                raise NotImplementedError(f"RandAugment config key {key!r} in {config_str!r} is not known")
        if self.num_layers < 1:
            raise ValueError("RandAugment needs at least one layer")
        self.config_str = config_str
        self.ops = RAND_INCREASING_TRANSFORMS if self.increasing else RAND_TRANSFORMS
        self.prob = 0.5
        self.fill = tuple(min(255, round(255 * x)) for x in img_mean)

    def draw(self, B: int, rng, size=224) -> np.ndarray:
        """The plan of a batch: a record array [B, n] of OP_DTYPE for frames of size = (w, h) (an int: square).  Draw order, per
        sample: the n op indices (rng.randint(0, 15, n)); then per op, ALWAYS three draws -- rng.random_sample() (> 0.5: the layer is
        skipped), rng.normal(m, mstd) (the magnitude; at mstd = 0 it is m), rng.random_sample() (> 0.5: the argument is negated,
        for the ops that have a sign)."""
        w, h = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        plan = np.zeros((B, self.num_layers), dtype=OP_DTYPE)
        for b in range(B):
            idx = rng.randint(0, len(self.ops), self.num_layers)
            for l in range(self.num_layers):
                skip = rng.random_sample() > self.prob
                mag = rng.normal(self.magnitude, self.magnitude_std)
                negate = rng.random_sample() > 0.5
                if skip:
                    continue   # (zeros: OP_IDENTITY)
                name = self.ops[int(idx[l])]
                mag = min(MAX_LEVEL, max(0.0, float(mag)))
                plan[b, l] = op_record(name, level_to_arg(name, mag, negate and name in _SIGNED), w, h)
        return plan

    def apply(self, x, plan, hflip=None, scratch=None):
        """x: uint8 [B, H, W, 3] on the device -> the augmented frames (a scratch buffer: valid until the next call).  hflip: uint8
        / bool [B] or None -- the flip timm applies BEFORE the policy, fused into the first layer.  Two launches per layer, one when
        no sample's op needs the frame's statistics."""
        import torch
        from . import _lib
        from .data import _Scratch, _check_u8_frames
        _check_u8_frames(x, "RandAugment.apply")
        B, H, W, _ = x.shape
        plan = np.ascontiguousarray(plan)
        if plan.dtype != OP_DTYPE or plan.ndim != 2 or plan.shape[0] != B:
            raise ValueError("plan must be a [B, n] record array of timm_aug.OP_DTYPE")
        sc = scratch if scratch is not None else self.__dict__.setdefault("_scratch", _Scratch(x.device))
        lib, st = _lib.load(), torch.cuda.current_stream(x.device).cuda_stream
        n = plan.shape[1]
        plan_d = sc.upload("ra_plan", plan.view(np.uint8).reshape(B, n * OP_DTYPE.itemsize))
        flip_d = sc.upload("ra_flip", np.asarray(hflip).astype(np.uint8).reshape(B)) if hflip is not None else None
        ws_bytes = _lib.workspace_bytes("pm_randaug_workspace", B)
        stats = sc.grow("ra_stats", ws_bytes // 8, torch.int64)
        bufs = [sc.exact("ra_a", (B, H, W, 3), torch.uint8), sc.exact("ra_b", (B, H, W, 3), torch.uint8)]
        cur = x
        for l in range(n):
            ops_ptr = plan_d.data_ptr() + l * OP_DTYPE.itemsize
            need = bool(np.isin(plan["op"][:, l], STATS_OPS).any())
            if need:
                _lib.check(lib.pm_randaug_stats(cur.data_ptr(), ops_ptr, n, stats.data_ptr(), ws_bytes, B, H, W, st), "pm_randaug_stats")
            dst = bufs[l & 1]
            _lib.check(lib.pm_randaug_apply(cur.data_ptr(), dst.data_ptr(), ops_ptr, n,
                                            flip_d.data_ptr() if (flip_d is not None and l == 0) else None,
                                            stats.data_ptr() if need else None, ws_bytes if need else 0, B, H, W, *self.fill, st),
                       "pm_randaug_apply")
            cur = dst
        return cur


ERASE_MODES = {"const": 0, "rand": 1, "pixel": 2}


class RandomErasing:
    """timm's RandomErasing (random_erasing.py), restated from timm 0.4.12 and NOT checked against timm itself (see the module
    docstring): per sample, with probability `probability`, `count` boxes (a draw in [min_count, max_count]) of area
    uniform(min_area, max_area) * H W / count and aspect exp(uniform(log min_aspect, log max_aspect)), each found in at most 10
    attempts, filled with zeros ('const'), one normal per channel ('rand') or one per element ('pixel').  `num_splits` (--resplit)
    is refused."""

    def __init__(self, probability: float = 0.5, mode: str = "pixel", min_count: int = 1, max_count: Optional[int] = None,
                 min_area: float = 0.02, max_area: float = 1 / 3, min_aspect: float = 0.3, max_aspect: Optional[float] = None,
                 num_splits: int = 0):
        if num_splits:
            raise NotImplementedError("RandomErasing num_splits / --resplit (a clean first split of the batch) is not built")
        if mode not in ERASE_MODES:
            raise ValueError(f"RandomErasing mode {mode!r}: one of {sorted(ERASE_MODES)}")
        self.probability, self.mode = float(probability), mode
        self.min_count, self.max_count = int(min_count), int(max_count or min_count)
        if not 1 <= self.min_count <= self.max_count <= 64:
            raise ValueError("RandomErasing needs 1 <= min_count <= max_count <= 64")
        self.min_area, self.max_area = float(min_area), float(max_area)
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))

    def draw(self, B: int, chw, rng) -> np.ndarray:
        """int32 [B, max_count, 4] = (top, left, h, w) per box, zeros where there is none.  Draw order, per sample:
        rng.random_sample() (> probability: no box); rng.randint(min_count, max_count + 1) when the two differ; per box up to 10
        attempts of rng.uniform(min_area, max_area), rng.uniform(log min_aspect, log max_aspect), and for the attempt whose
        h = int(round(sqrt(a r))) < H and w = int(round(sqrt(a / r))) < W: rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)."""
        _, img_h, img_w = chw
        boxes = np.zeros((B, self.max_count, 4), dtype=np.int32)
        area = img_h * img_w
        for b in range(B):
            if rng.random_sample() > self.probability:
                continue
            count = self.min_count if self.min_count == self.max_count else int(rng.randint(self.min_count, self.max_count + 1))
            for k in range(count):
                for _attempt in range(10):
                    target_area = rng.uniform(self.min_area, self.max_area) * area / count
                    aspect_ratio = math.exp(rng.uniform(*self.log_aspect_ratio))
                    h = int(round(math.sqrt(target_area * aspect_ratio)))
                    w = int(round(math.sqrt(target_area / aspect_ratio)))
                    if w < img_w and h < img_h:
                        top = int(rng.randint(0, img_h - h + 1))
                        left = int(rng.randint(0, img_w - w + 1))
                        boxes[b, k] = (top, left, h, w)
                        break
        return boxes

    def apply(self, x, boxes, key, scratch=None):
        """x: f32 [B, C, H, W] on the device, erased IN PLACE (and returned).  key = (seed, counter): the 64-bit Philox key and the
        64-bit counter words that make the normals of this call a function of (seed, epoch and step, sample, box, element).  No
        launch, and no upload, when no sample drew a box."""
        import torch
        from . import _lib
        from .data import _Scratch
        if x.dtype != torch.float32 or x.ndim != 4 or not x.is_contiguous():
            raise ValueError("RandomErasing.apply takes a contiguous float32 [B, C, H, W] tensor")
        if not x.is_cuda:
            raise _lib.PolypMaeError("RandomErasing.apply runs on the GPU only (no CPU fallback)")
        B, C, H, W = x.shape
        boxes = np.ascontiguousarray(boxes, dtype=np.int32)
        if boxes.ndim != 3 or boxes.shape[0] != B or boxes.shape[2] != 4:
            raise ValueError("boxes must be int32 [B, max_count, 4]")
        if not ((boxes[..., 2] > 0) & (boxes[..., 3] > 0)).any():
            return x
        sc = scratch if scratch is not None else self.__dict__.setdefault("_scratch", _Scratch(x.device))
        box_d = sc.upload("re_boxes", boxes)
        seed, counter = key
        _lib.check(_lib.load().pm_random_erase_f32(x.data_ptr(), box_d.data_ptr(), boxes.shape[1], ERASE_MODES[self.mode],
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF, B, C, H, W,
                                                   torch.cuda.current_stream(x.device).cuda_stream), "pm_random_erase_f32")
        return x


class TrainAugment:
    """The RandAugment and the RandomErasing of one training transform (either may be None), with the host generator and the
    erasing key of the current epoch.  reseed(seed, epoch) makes both a function of (seed, epoch) alone; every batch then takes
    the next step of the key."""

    def __init__(self, rand_augment: Optional[RandAugment] = None, random_erasing: Optional[RandomErasing] = None):
        self.rand_augment, self.random_erasing = rand_augment, random_erasing
        self.reseed(0, 0)

    def reseed(self, seed: int, epoch: int) -> None:
        self.seed, self.epoch, self.step = int(seed), int(epoch), 0
        # (a third word keeps these draws apart from main_finetune_mae.mix_rng's, which is seeded from the same pair)
        self.rng = np.random.RandomState([int(seed) & 0x7FFFFFFF, int(epoch), 0x7A])

    def next_key(self):
        """(seed, counter) of the next batch's erasing normals: counter = epoch << 32 | step."""
        key = (self.seed & 0xFFFFFFFFFFFFFFFF, ((self.epoch & 0xFFFFFFFF) << 32) | (self.step & 0xFFFFFFFF))
        self.step += 1
        return key
