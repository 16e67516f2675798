"""Device-side tail of the input pipeline.

The reference decodes, resizes and augments with PIL on DataLoader workers and hands float32 NCHW batches to the GPU
(classification/data/transforms.py:225-253, mae/main_pretrain.py:156-191).  Here the workers stop at decoded uint8
HWC frames; `DevicePrefetcher` stages them through pinned host buffers, copies them on a dedicated stream while the
previous step computes (a uint8 batch is a quarter of the float32 bytes on PCIe) and runs the last three transform
stages on the device in one HBM-bound kernel (`pm_preprocess_u8`): optional horizontal / vertical flip, ToTensor,
Normalize -- bit-exact with torchvision's float32 arithmetic.  `DeviceAugmenter` (round 3) moves the rest of the train transform
there as well -- Resize, ColorJitter, GaussianBlur((25, 25)), flips, RandomRotation(180) -- with Pillow's own integer / float
arithmetic (`pm_aug_*`, csrc/pm_augment.hip), so the workers are left with JPEG decoding only.  A batch of frames of different
decoded sizes (an image folder) travels as one `RaggedFrames` -- the frames packed back to back plus an offset and a size table --
and its first device stage (the Resize, or the MAE transform's RandomResizedCrop) is a per-sample resized crop that reads each
frame where it lies (`pm_aug_resized_crop_ragged_u8`); the folder dataset and its loader are in folder.py.
"""
from __future__ import annotations

import concurrent.futures
import math
from typing import Iterable, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN: Sequence[float] = (0.485, 0.456, 0.406)   # transforms.py:16
IMAGENET_STD: Sequence[float] = (0.229, 0.224, 0.225)    # transforms.py:17


def _check_u8_frames(frames: torch.Tensor, who: str, host_error=_lib.PolypMaeError) -> None:
    """A uniform batch: contiguous uint8 [B, H, W, 3] on the GPU (`host_error`: what a host tensor raises)."""
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 [B, H, W, 3] tensor")
    if not frames.is_cuda:
        raise host_error(f"{who} runs on the GPU only (no CPU fallback)")


def preprocess_u8(frames: torch.Tensor, flips: Optional[torch.Tensor] = None, mean: Sequence[float] = IMAGENET_MEAN,
                  std: Sequence[float] = IMAGENET_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames: uint8 [B, H, W, 3] on the GPU; flips: uint8 [B] (bit 0 horizontal, bit 1 vertical) or None.
    Returns float32 [B, 3, H, W] = Normalize(mean, std)(ToTensor(frame)) of the (flipped) frames."""
    _check_u8_frames(frames, "preprocess_u8")
    B, H, W, _ = frames.shape
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=frames.device)
    if flips is not None and (flips.dtype != torch.uint8 or flips.numel() != B or flips.device != frames.device):
        raise ValueError("flips must be uint8 [B] on the frames' device")
    lib = _lib.load()
    st = lib.pm_preprocess_u8(frames.data_ptr(), flips.data_ptr() if flips is not None else None, out.data_ptr(), B, H, W,
                              float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]), float(std[2]),
                              torch.cuda.current_stream(frames.device).cuda_stream)
    _lib.check(st, "pm_preprocess_u8")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# train-time augmentation on the device (classification/data/transforms.py:234-246)
# ---------------------------------------------------------------------------------------------------------------------
def _resample_coeffs(in_size: int, out_size: int):
    """Pillow Resample.c precompute_coeffs (bilinear filter, support 1, antialiased) + normalize_coeffs_8bpc: for every output
    index the first source index, the tap count and the 22-bit fixed-point taps.  Double arithmetic, as in the C source."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)], dtype=np.float64)
        ww = 0.0
        for v in w:   # (the C loop's summation order)
            ww += v
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    taps = np.where(kk < 0, (-0.5 + kk * (1 << 22)).astype(np.int64), (0.5 + kk * (1 << 22)).astype(np.int64)).astype(np.int32)
    return bounds, taps, ksize


def _gaussian_taps(ksize: int, sigma):
    """torchvision functional_tensor._get_gaussian_kernel1d in float32, one row per sigma."""
    half = (ksize - 1) * 0.5
    x = np.linspace(-half, half, ksize, dtype=np.float32)
    rows = []
    for sg in sigma:
        pdf = np.exp(np.float32(-0.5) * (x / np.float32(sg)) ** 2).astype(np.float32)
        rows.append((pdf / pdf.sum(dtype=np.float32)).astype(np.float32))
    return np.stack(rows)


def _rotation_geom(angle_deg: float, w: int, h: int, flips: int):
    """Image.rotate(angle, NEAREST, expand=False, center=None) -> the pm_aug_geom record: Pillow's inverse affine map about the
    image centre (coefficients rounded to 15 decimals, then FIX(v) = floor(v * 65536 + 0.5), half-pixel offsets folded into
    a2 / a5 as Geometry.c affine_fixed does), or one of its transpose fast paths."""
    ang = angle_deg % 360.0
    if ang == 0:
        return (1, 0, 0, 0, 0, 0, 0, flips)
    if ang == 180:
        return (2, 0, 0, 0, 0, 0, 0, flips)
    if ang in (90, 270) and w == h:
        return (3 if ang == 90 else 4, 0, 0, 0, 0, 0, 0, flips)
    rad = -math.radians(ang)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return (0, fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[3] * 0.5 + m[4] * 0.5), flips)


def draw_train_params(B: int, generator: Optional[torch.Generator] = None, brightness=0.4, contrast=0.5, saturation=0.25, hue=0.01,
                      sigma=(0.001, 2.0), flip_p=0.5, degrees=180.0) -> dict:
    """The random draws of the reference's train transform for B samples (transforms.py:238-245; torchvision 0.10 get_params:
    ColorJitter -> a permutation of the four ops + one uniform factor each, GaussianBlur -> sigma ~ U(0.001, 2),
    RandomHorizontal/VerticalFlip -> rand < 0.5, RandomRotation -> angle ~ U(-180, 180)).  The reference draws per image inside
    its DataLoader workers; here one host generator serves the batch (the streams differ, the distributions do not)."""
    g = generator
    u = lambda lo, hi: torch.empty(B, dtype=torch.float64).uniform_(lo, hi, generator=g)
    order = torch.stack([torch.randperm(4, generator=g) for _ in range(B)])
    return {"order": order.numpy(), "brightness": u(max(0.0, 1 - brightness), 1 + brightness).numpy(),
            "contrast": u(max(0.0, 1 - contrast), 1 + contrast).numpy(), "saturation": u(max(0.0, 1 - saturation), 1 + saturation).numpy(),
            "hue": u(-hue, hue).numpy(), "sigma": u(sigma[0], sigma[1]).numpy(),
            "hflip": (torch.rand(B, generator=g) < flip_p).numpy(), "vflip": (torch.rand(B, generator=g) < flip_p).numpy(),
            "angle": u(-degrees, degrees).numpy()}


class RaggedFrames:
    """A batch of decoded HWC uint8 frames of different sizes, packed back to back: `data` uint8 [total], frame b is the
    hw[b] = (H_b, W_b) image starting at byte offset[b] (`offset` int64 [B], `hw` int32 [B, 2], on the device of `data`).  A host
    copy of the two tables travels with the object, so callers on the device side (box draws, validation, workspace sizes) never
    read them back.  Build one with `from_frames`; `ragged_collate` does so in DataLoader workers."""

    def __init__(self, data: torch.Tensor, offset: torch.Tensor, hw: torch.Tensor, _host=None):
        if data.dtype != torch.uint8 or data.ndim != 1 or not data.is_contiguous():
            raise ValueError("RaggedFrames.data must be a contiguous 1-D uint8 tensor")
        if offset.dtype != torch.int64 or hw.dtype != torch.int32 or offset.ndim != 1 or tuple(hw.shape) != (offset.numel(), 2) \
                or offset.device != data.device or hw.device != data.device or not offset.is_contiguous() or not hw.is_contiguous():
            raise ValueError("RaggedFrames needs offset int64 [B] and hw int32 [B, 2] on the device of the data")
        if _host is None:
            _host = (offset.cpu().numpy().astype(np.int64), hw.cpu().numpy().astype(np.int64))
        off_h, hw_h = _host
        if len(off_h) == 0 or (hw_h <= 0).any() or (off_h < 0).any() or \
                (off_h + hw_h[:, 0] * hw_h[:, 1] * 3 > data.numel()).any():
            raise ValueError("RaggedFrames: every frame must be non-empty and lie inside the packed data")
        self.data, self.offset, self.hw, self._host = data, offset, hw, (off_h, hw_h)

    @classmethod
    def from_frames(cls, frames) -> "RaggedFrames":
        """frames: a sequence of HWC uint8 arrays or tensors [H_b, W_b, 3] -> one packed host batch (one copy of the pixels)."""
        arrs = [f.numpy() if torch.is_tensor(f) else np.asarray(f) for f in frames]
        if not arrs or any(a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 for a in arrs):
            raise ValueError("RaggedFrames.from_frames takes a non-empty sequence of uint8 [H, W, 3] frames")
        hw = np.array([a.shape[:2] for a in arrs], dtype=np.int64)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offset = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs]))
        return cls(data, torch.from_numpy(offset.copy()), torch.from_numpy(hw.astype(np.int32)), _host=(offset, hw))

    def __len__(self) -> int:
        return len(self._host[0])

    @property
    def sizes(self):
        """numpy int64 [B, 2] = (H_b, W_b), host side."""
        return self._host[1]

    @property
    def offsets(self):
        """numpy int64 [B], host side."""
        return self._host[0]

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    def is_pinned(self) -> bool:
        return self.data.is_pinned() and self.offset.is_pinned() and self.hw.is_pinned()

    def to(self, device, non_blocking: bool = False) -> "RaggedFrames":
        return RaggedFrames(self.data.to(device, non_blocking=non_blocking), self.offset.to(device, non_blocking=non_blocking),
                            self.hw.to(device, non_blocking=non_blocking), _host=self._host)

    def pin_memory(self, device=None) -> "RaggedFrames":
        """(called by DataLoader(pin_memory=True) in its pin thread)"""
        return RaggedFrames(self.data.pin_memory(), self.offset.pin_memory(), self.hw.pin_memory(), _host=self._host)

    def frame(self, b: int) -> torch.Tensor:
        """A [H_b, W_b, 3] view of frame b."""
        o, (h, w) = int(self._host[0][b]), (int(v) for v in self._host[1][b])
        return self.data[o:o + h * w * 3].view(h, w, 3)


def _check_ragged_on_device(frames: "RaggedFrames", who: str) -> None:
    if not frames.is_cuda:
        raise _lib.PolypMaeError(f"{who} runs on the GPU only (no CPU fallback): move the RaggedFrames to the device first")


def draw_rrc_boxes(B: int, height, width, generator: Optional[torch.Generator] = None, scale=(0.2, 1.0),
                   ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision 0.10 RandomResizedCrop.get_params for B frames -> int32 [B, 4] = (top, left, h, w) (mae/main_pretrain.py:157:
    scale (0.2, 1.0), default ratio): up to ten tries of area ~ U(scale) x aspect ~ logU(ratio), then the central-crop fallback.
    height / width: one size for the batch, or one per frame (box b is get_params of frame b; one generator serves the batch in
    frame order, so equal per-frame sizes draw exactly what the scalar form draws)."""
    g = generator
    hs = [int(v) for v in height] if isinstance(height, (Sequence, np.ndarray, torch.Tensor)) else [int(height)] * B
    ws = [int(v) for v in width] if isinstance(width, (Sequence, np.ndarray, torch.Tensor)) else [int(width)] * B
    if len(hs) != B or len(ws) != B:
        raise ValueError("height / width: a scalar or one value per frame")
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    out = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        height, width = hs[b], ws[b]
        area = height * width
        for _ in range(10):
            target = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
            aspect = math.exp(torch.empty(1).uniform_(lr0, lr1, generator=g).item())
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                i = torch.randint(0, height - h + 1, (1,), generator=g).item()
                j = torch.randint(0, width - w + 1, (1,), generator=g).item()
                out[b] = (i, j, h, w)
                break
        else:
            in_ratio = width / height
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            out[b] = ((height - h) // 2, (width - w) // 2, h, w)
    return out


def draw_linprobe_boxes(B: int, height, width, generator: Optional[torch.Generator] = None, scale=(0.08, 1.0),
                        ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """mae/util/crop.py RandomResizedCrop.get_params (the linear probe's training crop, main_linprobe.py:146) for B frames -> int32
    [B, 4] = (top, left, h, w).  Not torchvision's sampler (draw_rrc_boxes): one draw, no retry loop and no central-crop fallback;
    a box that does not fit is clamped to the frame, and the aspect ratio is exp of an f32 uniform between the f32 logs of `ratio`,
    evaluated in f32 as the reference's torch.exp does.  One generator serves the batch in frame order (None: torch's global one,
    as the reference uses it)."""
    g = generator
    hs = [int(v) for v in height] if isinstance(height, (Sequence, np.ndarray, torch.Tensor)) else [int(height)] * B
    ws = [int(v) for v in width] if isinstance(width, (Sequence, np.ndarray, torch.Tensor)) else [int(width)] * B
    if len(hs) != B or len(ws) != B:
        raise ValueError("height / width: a scalar or one value per frame")
    log_ratio = torch.log(torch.tensor(ratio))
    out = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        height, width = hs[b], ws[b]
        target = height * width * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
        w = min(int(round(math.sqrt(target * aspect))), width)
        h = min(int(round(math.sqrt(target / aspect))), height)
        i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
        j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
        out[b] = (i, j, h, w)
    return out


def _check_boxes(boxes, hw) -> np.ndarray:
    """Crop boxes (top, left, h, w), one per frame, each non-empty and inside its own frame -- hw: int [B, 2] = (H_b, W_b), a
    uniform batch's one size broadcast -- as the int32 C-contiguous [B, 4] table the crop kernels read."""
    boxes = np.ascontiguousarray(boxes, dtype=np.int32)
    if boxes.shape != (len(hw), 4) or (boxes[:, 2:] <= 0).any() or (boxes[:, :2] < 0).any() or \
            (boxes[:, :2] + boxes[:, 2:] > hw).any():
        raise ValueError("crop boxes must be (top, left, h, w) inside their own frame, one per sample")
    return boxes


def _whole_frame_boxes(hw) -> np.ndarray:
    """The boxes (0, 0, H_b, W_b) that make a resized crop the Resize of the whole frame."""
    boxes = np.zeros((len(hw), 4), dtype=np.int32)
    boxes[:, 2:] = hw
    return boxes


def center_crop_windows(hw, resize: int, crop: int) -> np.ndarray:
    """torchvision Resize(resize) + CenterCrop(crop) of frames of sizes hw [B, 2] = (H_b, W_b) -> int32 [B, 4] = (nh, nw, top, left):
    the full resized size and the crop window's origin in it, in the arithmetic of mae_recipe._ValFrames.  Resize(int) brings the
    shorter side to `resize` and the other to int(resize * other / shorter), and does nothing when the shorter side already equals
    `resize`; center_crop's origin is int(round((n - crop) / 2.0)), Python's round-half-to-even."""
    resize, crop = int(resize), int(crop)
    if crop < 1 or crop > resize:
        raise ValueError(f"crop must be in 1..resize (torchvision pads a crop of {crop} out of a resize to {resize}: not built)")
    out = np.zeros((len(hw), 4), dtype=np.int32)
    for b, (h, w) in enumerate(hw):
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise ValueError("frames must be non-empty")
        if (w <= h and w != resize) or (h <= w and h != resize):
            h, w = (int(resize * h / w), resize) if w <= h else (resize, int(resize * w / h))
        out[b] = (h, w, int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0)))
    return out


class _Scratch:
    """The device buffers one object keeps across calls, by name (`bufs`), so that a steady stream of batches allocates nothing."""

    def __init__(self, device):
        self.device, self.bufs = torch.device(device), {}

    def exact(self, name: str, shape, dtype) -> torch.Tensor:
        """A tensor of this shape and dtype, reallocated when either differs from the last call's."""
        t = self.bufs.get(name)
        if t is None or t.shape != torch.Size(shape) or t.dtype != dtype:
            t = self.bufs[name] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    def grow(self, name: str, n: int, dtype) -> torch.Tensor:
        """A flat tensor of at least n elements, reallocated only when a call needs more than it holds (callers take a view of
        its front: a workspace follows the largest batch seen)."""
        t = self.bufs.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self.bufs[name] = torch.empty(max(int(n), 1), dtype=dtype, device=self.device)
        return t

    def upload(self, name: str, arr) -> torch.Tensor:
        """numpy -> device through a pinned staging tensor kept per name (non-blocking; rewritten only after a host sync of the
        previous copy's event)."""
        host = torch.from_numpy(np.ascontiguousarray(arr))
        slot = self.bufs.get("pin_" + name)
        if slot is None or slot[0].shape != host.shape or slot[0].dtype != host.dtype:
            slot = self.bufs["pin_" + name] = [torch.empty(host.shape, dtype=host.dtype).pin_memory(), None]
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(host)
        dev = self.exact("dev_" + name, host.shape, host.dtype)
        dev.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        return dev


class DeviceAugmenter:
    """The reference's whole train transform after decoding, on the device: [Resize ->] ColorJitter -> GaussianBlur(25) -> flips
    -> RandomRotation(180) -> ToTensor -> Normalize, six launches over a uint8 batch (pm_aug_*), f32 NCHW out.  The host does
    what is scalar and per sample: the random draws, Pillow's resample taps (cached per size pair), the blur taps, the rotation's
    fixed-point matrix -- a few hundred bytes per batch, uploaded from pinned memory on the caller's stream."""

    KSIZE = 25  # transforms.py:239

    def __init__(self, device, size: int = 224, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD):
        self.device, self.size, self.mean, self.std = torch.device(device), int(size), tuple(mean), tuple(std)
        self._coeffs = {}
        self._scratch = _Scratch(self.device)

    def _resized_crop(self, frames, boxes: np.ndarray, bicubic: bool, name: str) -> torch.Tensor:
        """pm_aug_resized_crop_u8 / pm_aug_resized_crop_ragged_u8: frames uint8 [B, Hs, Ws, 3] or a RaggedFrames, on the device;
        boxes as _check_boxes returns them.  The workspace follows the largest frame seen; `name` keeps the box upload and the
        output of the Resize apart from those of the RandomResizedCrop."""
        B, S, sc = len(frames), self.size, self._scratch
        lib = _lib.load()
        if isinstance(frames, RaggedFrames):
            fn, src = lib.pm_aug_resized_crop_ragged_u8, (frames.data.data_ptr(), frames.offset.data_ptr(), frames.hw.data_ptr())
            Hmax, Wmax = (int(v) for v in frames.sizes.max(0))
        else:
            fn, src = lib.pm_aug_resized_crop_u8, (frames.data_ptr(),)
            Hmax, Wmax = frames.shape[1:3]
        ws = sc.grow("crop_ws", int(lib.pm_aug_resized_crop_workspace_bytes(B, Hmax, Wmax, S)), torch.uint8)
        box_d = sc.upload(name + "_box", boxes)
        out = sc.exact(name + "_out", (B, S, S, 3), torch.uint8)
        _lib.check(fn(*src, box_d.data_ptr(), out.data_ptr(), 1 if bicubic else 0, B, Hmax, Wmax, S, ws.data_ptr(), ws.numel(),
                      torch.cuda.current_stream(self.device).cuda_stream), fn.__name__)
        return out

    def resize(self, frames) -> torch.Tensor:
        """uint8 [B, Hs, Ws, 3] -> uint8 [B, size, size, 3] (T.Resize((size, size)) on PIL images).  A device-resident RaggedFrames
        goes through the ragged resized crop with the whole frame as the box and the bilinear filter (the same taps)."""
        if isinstance(frames, RaggedFrames):
            _check_ragged_on_device(frames, "DeviceAugmenter")
            return self._resized_crop(frames, _whole_frame_boxes(frames.sizes), False, "rs")
        B, Hs, Ws, _ = frames.shape
        S = self.size
        if (Hs, Ws) == (S, S):
            return frames
        key = (Hs, Ws, S)
        c = self._coeffs.get(key)
        if c is None:
            bx, tx, kx = _resample_coeffs(Ws, S)
            by, ty, ky = _resample_coeffs(Hs, S)
            c = self._coeffs[key] = tuple(torch.from_numpy(a).to(self.device) for a in (bx, tx, by, ty)) + (kx, ky)
        bx, tx, by, ty, kx, ky = c
        tmp = self._scratch.exact("rs_tmp", (B, Hs, S, 3), torch.uint8)
        out = self._scratch.exact("rs_out", (B, S, S, 3), torch.uint8)
        lib = _lib.load()
        _lib.check(lib.pm_aug_resize_u8(frames.data_ptr(), tmp.data_ptr(), out.data_ptr(), bx.data_ptr(), tx.data_ptr(), kx,
                                        by.data_ptr(), ty.data_ptr(), ky, B, Hs, Ws, S, S,
                                        torch.cuda.current_stream(self.device).cuda_stream), "pm_aug_resize_u8")
        return out

    def resize_center_crop(self, frames: "RaggedFrames", resize: int = 256, crop: Optional[int] = None) -> torch.Tensor:
        """A device-resident RaggedFrames -> uint8 [B, crop, crop, 3] (crop=None: self.size): the validation transform of the MAE
        recipes, Resize(resize, bicubic) + CenterCrop(crop) as torchvision runs it on PIL images, byte for byte
        (pm_aug_resize_center_crop_ragged_u8; the windows are center_crop_windows of the frames' sizes).  crop > resize raises
        ValueError: torchvision pads there, which is not built."""
        if not isinstance(frames, RaggedFrames):
            raise TypeError("resize_center_crop takes a RaggedFrames")
        _check_ragged_on_device(frames, "DeviceAugmenter")
        B, R, C, sc = len(frames), int(resize), int(self.size if crop is None else crop), self._scratch
        win = center_crop_windows(frames.sizes, R, C)
        Hmax, Wmax = (int(v) for v in frames.sizes.max(0))
        ws = sc.grow("center_ws", _lib.workspace_bytes("pm_aug_resize_center_crop_workspace", B, Hmax, Wmax, R, C), torch.uint8)
        win_d = sc.upload("center_win", win)
        out = sc.exact("center_out", (B, C, C, 3), torch.uint8)
        _lib.check(_lib.load().pm_aug_resize_center_crop_ragged_u8(
            frames.data.data_ptr(), frames.offset.data_ptr(), frames.hw.data_ptr(), win_d.data_ptr(), out.data_ptr(), B, Hmax, Wmax, R,
            C, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream), "pm_aug_resize_center_crop_ragged_u8")
        return out

    def random_resized_crop(self, frames, boxes=None, generator: Optional[torch.Generator] = None,
                            bicubic: bool = True) -> torch.Tensor:
        """uint8 [B, Hs, Ws, 3] or a device-resident RaggedFrames -> uint8 [B, size, size, 3]: RandomResizedCrop(size,
        scale=(0.2, 1.0), interpolation=bicubic) of the MAE pre-train transform (main_pretrain.py:157), one crop box per sample
        (drawn here unless given, for a ragged batch from each frame's own size)."""
        if isinstance(frames, RaggedFrames):
            _check_ragged_on_device(frames, "DeviceAugmenter")
            hw = frames.sizes
        else:
            _check_u8_frames(frames, "DeviceAugmenter.random_resized_crop", host_error=ValueError)
            hw = np.broadcast_to(frames.shape[1:3], (len(frames), 2))
        if boxes is None:
            boxes = draw_rrc_boxes(len(frames), hw[:, 0], hw[:, 1], generator)
        return self._resized_crop(frames, _check_boxes(boxes, hw), bicubic, "rrc")

    def mae_transform(self, frames, boxes=None, hflip=None, generator: Optional[torch.Generator] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The MAE pre-train transform after decoding (main_pretrain.py:156-160): RandomResizedCrop(bicubic) -> RandomHorizontalFlip
        -> ToTensor -> Normalize, f32 [B, 3, size, size].  frames: uint8 [B, H, W, 3] or a device-resident RaggedFrames; the
        generator draws the boxes first, then the flips."""
        return self.mae_tail(self.random_resized_crop(frames, boxes, generator), hflip, generator, out)

    def mae_tail(self, x: torch.Tensor, hflip=None, generator: Optional[torch.Generator] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What mae_transform does after its crop: RandomHorizontalFlip -> ToTensor -> Normalize of an already cropped uint8 batch
        [B, size, size, 3] (the crop may come from elsewhere, e.g. DeviceJpegDecoder.resized_crop)."""
        if hflip is None:
            hflip = (torch.rand(len(x), generator=generator) < 0.5)
        flips = self._scratch.upload("mae_flips", torch.as_tensor(hflip).to(torch.uint8).numpy())
        return preprocess_u8(x, flips, self.mean, self.std, out=out)

    def timm_tail(self, x: torch.Tensor, train_aug, plan=None, boxes=None, hflip=None, generator: Optional[torch.Generator] = None,
                  rng=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What timm's create_transform(is_training=True, auto_augment=..., re_prob=...) does after its crop, to an already cropped
        uint8 batch [B, size, size, 3]: RandomHorizontalFlip -> RandAugment -> ToTensor -> Normalize -> RandomErasing, f32
        [B, 3, size, size].  train_aug: a timm_aug.TrainAugment (either stage may be None).  The flips come from `generator` exactly
        as mae_tail draws them; the plan and the boxes, unless given, from `rng` (default: train_aug.rng) in that order; the erasing
        normals are keyed by train_aug.next_key().  With a RandAugment the flip is part of its first layer (the ops see timm's
        flipped frame); without one this is mae_tail followed by the erasing."""
        B = len(x)
        if hflip is None:
            hflip = (torch.rand(B, generator=generator) < 0.5)
        hflip = torch.as_tensor(hflip).to(torch.uint8).numpy()
        rng = train_aug.rng if rng is None else rng
        ra, re = train_aug.rand_augment, train_aug.random_erasing
        if ra is not None:
            _check_u8_frames(x, "DeviceAugmenter.timm_tail")
            if plan is None:
                plan = ra.draw(B, rng, (x.shape[2], x.shape[1]))
            x = ra.apply(x, plan, hflip=hflip, scratch=self._scratch)
            res = preprocess_u8(x, None, self.mean, self.std, out=out)
        else:
            res = preprocess_u8(x, self._scratch.upload("mae_flips", hflip), self.mean, self.std, out=out)
        if re is not None:
            if boxes is None:
                boxes = re.draw(B, tuple(res.shape[1:]), rng)
            re.apply(res, boxes, train_aug.next_key(), scratch=self._scratch)
        return res

    def __call__(self, frames, params: Optional[dict] = None, generator: Optional[torch.Generator] = None,
                 to_f32: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames uint8 [B, H, W, 3] or a RaggedFrames, on the device.  Returns f32 [B, 3, size, size] (normalised) or, with
        to_f32=False, the augmented uint8 frames [B, size, size, 3] (written into `out` when given).  After the Resize every frame
        is size x size, so a ragged batch continues down the uniform chain."""
        if isinstance(frames, RaggedFrames):
            _check_ragged_on_device(frames, "DeviceAugmenter")
        else:
            _check_u8_frames(frames, "DeviceAugmenter")
        lib = _lib.load()
        st = torch.cuda.current_stream(self.device).cuda_stream
        up, buf = self._scratch.upload, self._scratch.exact
        x = self.resize(frames)
        B, H, W, _ = x.shape
        p = params if params is not None else draw_train_params(B, generator)
        # -- ColorJitter
        jit = np.zeros((B, 8), dtype=np.int32)
        jit[:, :4] = np.asarray(p["order"], dtype=np.int32)
        jit[:, 4:7] = np.stack([np.asarray(p[k], dtype=np.float32) for k in ("brightness", "contrast", "saturation")], 1).view(np.int32)
        jit[:, 7] = [int(np.int64(float(h) * 255)) & 0xFF for h in p["hue"]]   # np.uint8(hue_factor * 255): C cast, wraps
        jit_d = up("jit", jit)
        lsum = buf("lsum", (B,), torch.int64)
        a = buf("aug_a", (B, H, W, 3), torch.uint8)
        _lib.check(lib.pm_aug_color_jitter_u8(x.data_ptr(), a.data_ptr(), jit_d.data_ptr(), lsum.data_ptr(), B, H, W, st),
                   "pm_aug_color_jitter_u8")
        # -- GaussianBlur((25, 25))
        taps_d = up("taps", _gaussian_taps(self.KSIZE, p["sigma"]))
        tmp = buf("blur_tmp", (B, H, W, 3), torch.float32)
        b = buf("aug_b", (B, H, W, 3), torch.uint8)
        _lib.check(lib.pm_aug_gaussian_blur_u8(a.data_ptr(), tmp.data_ptr(), b.data_ptr(), taps_d.data_ptr(), self.KSIZE, B, H, W,
                                               st), "pm_aug_gaussian_blur_u8")
        # -- flips + rotation (+ ToTensor + Normalize)
        geom = np.array([_rotation_geom(float(p["angle"][i]), W, H, int(bool(p["hflip"][i])) | (int(bool(p["vflip"][i])) << 1))
                         for i in range(B)], dtype=np.int32)
        geom_d = up("geom", geom)
        want = (B, 3, H, W) if to_f32 else (B, H, W, 3)
        if out is None:
            out = torch.empty(want, dtype=torch.float32 if to_f32 else torch.uint8, device=self.device)
        elif tuple(out.shape) != want or out.dtype != (torch.float32 if to_f32 else torch.uint8) or not out.is_contiguous():
            raise ValueError("`out` has the wrong shape / dtype")
        m, s = self.mean, self.std
        _lib.check(lib.pm_aug_geometry_u8(b.data_ptr(), geom_d.data_ptr(), out.data_ptr(), 1 if to_f32 else 0, B, H, W, float(m[0]),
                                          float(m[1]), float(m[2]), float(s[0]), float(s[1]), float(s[2]), st),
                   "pm_aug_geometry_u8")
        return out


# ------------------------------------------------------------------------------------------------------------------------------------
# Eval-time perturbations (classification/data/transforms.py:21-203): what PerRowPerturbations does to the resized PIL image of a
# row of an Exp-5A / 5B pack, planned on the host from the row's metadata and applied to the uint8 batch on the device
# ------------------------------------------------------------------------------------------------------------------------------------
DEFAULT_HMAC_KEY = b"ssl4polyp"   # transforms.py:18
_UNSET = (None, "", -1, "-1")
_UNSET_F = (None, "", -1, "-1", "-1.0")


def _variant_number(token: str):
    """A number as the variant names spell it (transforms.py:30-40): 'p' is the decimal point, 'minus' / 'neg' the sign."""
    t = token.strip().lower()
    if not t:
        return None
    t = t.replace("minus", "-").replace("neg", "-").replace("p", ".")
    try:
        return float(t)
    except ValueError:
        return None


def _last_number(variant: str):
    """The last '_'-separated token that reads as a number (transforms.py:43-49)."""
    for part in reversed(variant.split("_")):
        v = _variant_number(part)
        if v is not None:
            return v
    return None


def _row_seed(row, key: bytes) -> int:
    """transforms.py:123-140: HMAC-SHA256 over five metadata fields, first 8 bytes big-endian."""
    import hashlib
    import hmac
    msg = "|".join(str(row.get(f, "")) for f in ("frame_path", "frame_id", "case_id", "variant", "perturbation_id"))
    return int.from_bytes(hmac.new(key, msg.encode("utf-8"), hashlib.sha256).digest()[:8], "big", signed=False)


def occlusion_rect(area_fraction: float, seed: int, width: int, height: int):
    """transforms.py:99-120: the black rectangle of an "occ" row as (x0, y0, x1, y1), corners inclusive as ImageDraw.rectangle draws
    them, or None.  The draws come from Python's own random.Random(seed), in the reference's order."""
    import random
    a = max(0.0, min(float(area_fraction), 1.0))
    if a <= 0:
        return None
    rng = random.Random(seed)
    occ_area = max(1.0, a * (width * height))
    aspect = rng.uniform(0.5, 2.0)
    ow = max(1, min(width, int(round(math.sqrt(occ_area * aspect)))))
    oh = max(1, min(height, int(round(math.sqrt(occ_area / aspect)))))
    max_x, max_y = max(0, width - ow), max(0, height - oh)
    x0 = rng.randint(0, max_x) if max_x > 0 else 0
    y0 = rng.randint(0, max_y) if max_y > 0 else 0
    return x0, y0, min(width, x0 + ow), min(height, y0 + oh)


def perturbation_plan(row, key: bytes = DEFAULT_HMAC_KEY):
    """What PerRowPerturbations.__call__ (transforms.py:149-203) would do for this row, as a tuple:
    ("none",) | ("blur", sigma) | ("jpeg", quality) | ("bc", brightness or None, contrast or None) | ("occ", area_fraction, seed).
    Field values win over what the variant name spells; a variant whose number does not parse leaves the frame alone, as there."""
    if not row:
        return ("none",)
    flag = row.get("render_in_pipeline", True)
    if flag is None or not (flag if isinstance(flag, bool) else str(flag).strip().lower() in {"1", "true", "yes", "y"}):
        return ("none",)
    variant = str(row.get("variant") or row.get("perturbation_id") or "").strip()
    if not variant or variant.lower() == "clean":
        return ("none",)
    v = variant.lower()
    if v.startswith("blur"):
        f = row.get("blur_sigma")
        sigma = float(f) if f not in _UNSET_F else _last_number(v)
        return ("blur", sigma) if sigma is not None and sigma > 0 else ("none",)
    if v.startswith("jpeg"):
        f = row.get("jpeg_q")
        q = float(f) if f not in _UNSET else _last_number(v)
        if q is not None and f in _UNSET:
            q = float(int(round(q)))          # (_parse_quality rounds once, the caller once more)
        return ("jpeg", max(1, min(int(round(q)), 100))) if q is not None else ("none",)
    if v.startswith("bc"):
        fb, fc = row.get("brightness"), row.get("contrast")
        b = float(fb) if fb not in _UNSET_F else None
        c = float(fc) if fc not in _UNSET_F else None
        pb = pc = None
        for part in v.split("_"):
            if part.startswith("b"):
                pb = _variant_number(part[1:])
            elif part.startswith("c"):
                pc = _variant_number(part[1:])
        return ("bc", b if b is not None else pb, c if c is not None else pc)
    if v.startswith("occ"):
        f = row.get("bbox_area_frac")
        if f not in _UNSET_F:
            area = float(f)
        else:
            area = _variant_number(v.split("a", 1)[1] if "a" in v else v.split("_")[-1])
        if area is None or area <= 0:
            return ("none",)
        rs = row.get("rng_seed")
        return ("occ", area, int(rs) if rs not in _UNSET else _row_seed(row, key))
    return ("none",)


def pil_box_blur_params(sigma: float, passes: int = 3):
    """(radius, ww, fw) of Pillow's ImagingGaussianBlur for ImageFilter.GaussianBlur(radius=sigma) (BoxBlur.c: _gaussian_blur_radius, then
    ImagingHorizontalBoxBlur's fixed-point weights), in the float32 / UINT32 arithmetic of the C code.  radius = -1: nothing to blur."""
    f32 = np.float32
    s = f32(sigma)
    s2 = f32(s * s / f32(passes))
    big_l = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(big_l) - 1.0) / 2.0))
    a = f32((f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * s2))
    a = f32(a / f32(f32(6) * (s2 - (l + f32(1)) * (l + f32(1)))))
    r = f32(l + a)
    if not r > 0:
        return -1, 0, 0
    radius = int(r)
    ww = int(np.uint32(f32(16777216.0) / f32(r * f32(2) + f32(1))))
    fw = ((1 << 24) - (radius * 2 + 1) * ww) // 2
    return radius, ww, fw & 0xFFFFFFFF


class DevicePerturber:
    """PerRowPerturbations (transforms.py:143-203) for a whole uint8 batch on the device: blur (Pillow's box-blur GaussianBlur),
    brightness / contrast (ImageEnhance blends), occlusion and the JPEG round trip (libjpeg's integer pipeline without a bitstream:
    the entropy coding is lossless), each bit for bit what Pillow returns for the row's image.  `jpeg_fn(frame_u8_hwc_numpy, quality)
    -> numpy`, when given, replaces the device JPEG stage by a host codec (A/B and other codecs).
    Frames are the RESIZED images (the perturbation sits between Resize and ToTensor: transforms.py:249-256)."""

    PASSES = 3  # ImageFilter.GaussianBlur -> ImagingGaussianBlur(..., passes=3)

    def __init__(self, device, key: bytes = DEFAULT_HMAC_KEY, jpeg_fn=None):
        self.device, self.key, self.jpeg_fn = torch.device(device), key, jpeg_fn
        self._scratch = _Scratch(self.device)
        self._aug: Optional[DeviceAugmenter] = None   # (eval_transform's Resize)
        self._decoder: Optional["DeviceJpegDecoder"] = None   # (batches(): kept across batches once a JpegBatch arrives)

    def eval_transform(self, frames: torch.Tensor, rows=None, size: int = 224, mean: Sequence[float] = IMAGENET_MEAN,
                       std: Sequence[float] = IMAGENET_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ClassificationTransforms(stage="val" / "test", enable_perturbations=rows is not None) for a decoded uint8 batch
        [B, Hs, Ws, 3] of one frame size, or a device-resident RaggedFrames of mixed sizes (transforms.py:234-256):
        Resize((size, size)) -> [the rows' perturbations] -> ToTensor -> Normalize, f32 [B, 3, size, size] out; three to ten
        launches, nothing leaves the device.  `out`: the f32 tensor to write (as preprocess_u8 takes it)."""
        if self._aug is None or self._aug.size != size:
            self._aug = DeviceAugmenter(self.device, size=size)
        x = self._aug.resize(frames)
        if rows is not None:
            x = self(x, rows)
        return preprocess_u8(x, None, mean, std, out=out)

    def batches(self, loader: Iterable, size: int = 224) -> Iterator[Tuple]:
        """For the evaluation loop: `loader` yields (decoded uint8 frames [B, Hs, Ws, 3], a RaggedFrames or a jpeg.JpegBatch of
        compressed files -- decoded here on the device by a DeviceJpegDecoder this object keeps --, on the host, labels,
        rows) -- what PackDataset + pack_collate hand over before the transform (classification/data/packs.py:70-80) -- and this
        yields (f32 [B, 3, size, size] on the device, labels on the device, rows), i.e. what train.evaluate_cls iterates over, with
        the rows' perturbations rendered on the way (transforms.py:249-256)."""
        from .jpeg import JpegBatch
        for frames, labels, rows in loader:
            if isinstance(frames, JpegBatch):
                if self._decoder is None:
                    self._decoder = DeviceJpegDecoder(self.device)
                frames = self._decoder(frames.to(self.device, non_blocking=True))
            elif isinstance(frames, RaggedFrames):
                frames = frames.to(self.device, non_blocking=True)
            else:
                frames = torch.as_tensor(frames).to(self.device, non_blocking=True).contiguous()
            x = self.eval_transform(frames, rows, size=size)
            yield x, torch.as_tensor(labels).to(self.device, non_blocking=True), rows

    def __call__(self, frames: torch.Tensor, rows) -> torch.Tensor:
        """frames uint8 [B, H, W, 3] on the device, rows: one metadata mapping (or None) per frame.  Returns a new uint8 tensor."""
        _check_u8_frames(frames, "DevicePerturber")
        B, H, W, _ = frames.shape
        if len(rows) != B:
            raise ValueError("one row per frame")
        plans = [perturbation_plan(r, self.key) for r in rows]
        lib = _lib.load()
        st = torch.cuda.current_stream(self.device).cuda_stream
        up, buf = self._scratch.upload, self._scratch.exact
        out = frames.clone()
        kinds = {p[0] for p in plans}
        if "jpeg" in kinds:
            if self.jpeg_fn is not None:
                for i, p in enumerate(plans):
                    if p[0] == "jpeg":
                        out[i].copy_(torch.from_numpy(np.array(self.jpeg_fn(frames[i].cpu().numpy(), p[1]), dtype=np.uint8)))
            else:
                qual = np.array([p[1] if p[0] == "jpeg" else 0 for p in plans], dtype=np.int32)   # 0: the sample is copied
                _lib.check(lib.pm_aug_jpeg_roundtrip_u8(out.data_ptr(), out.data_ptr(), up("pt_jpeg", qual).data_ptr(), B, H, W, st),
                           "pm_aug_jpeg_roundtrip_u8")
        if "bc" in kinds:
            jit = np.zeros((B, 8), dtype=np.int32)
            jit[:, :4] = -1
            fac = np.ones((B, 3), dtype=np.float32)
            for i, p in enumerate(plans):
                if p[0] != "bc":
                    continue
                ops = []
                if p[1] is not None and p[1] > 0:   # transforms.py:92-96: brightness first, then contrast, each only if > 0
                    ops.append(0)
                    fac[i, 0] = p[1]
                if p[2] is not None and p[2] > 0:
                    ops.append(1)
                    fac[i, 1] = p[2]
                jit[i, :len(ops)] = ops
            jit[:, 4:7] = fac.view(np.int32)
            src = buf("pt_src", (B, H, W, 3), torch.uint8)
            src.copy_(out)
            _lib.check(lib.pm_aug_color_jitter_u8(src.data_ptr(), out.data_ptr(), up("pt_jit", jit).data_ptr(),
                                                  buf("pt_lsum", (B,), torch.int64).data_ptr(), B, H, W, st), "pm_aug_color_jitter_u8")
        if "blur" in kinds:
            prm = np.zeros((B, 3), dtype=np.uint32)
            prm[:, 0] = np.uint32(0xFFFFFFFF)   # radius -1: pass through
            for i, p in enumerate(plans):
                if p[0] == "blur":
                    r, ww, fw = pil_box_blur_params(p[1], self.PASSES)
                    prm[i] = (np.uint32(r & 0xFFFFFFFF), ww, fw)
            tmp = buf("pt_tmp", (B, H, W, 3), torch.uint8)
            _lib.check(lib.pm_aug_pil_gaussian_blur_u8(out.data_ptr(), tmp.data_ptr(), out.data_ptr(), up("pt_blur", prm.view(np.int32)).data_ptr(),
                                                       self.PASSES, B, H, W, st), "pm_aug_pil_gaussian_blur_u8")
        if "occ" in kinds:
            rects = np.zeros((B, 4), dtype=np.int32)
            rects[:, 2] = -1   # x1 < x0: nothing
            for i, p in enumerate(plans):
                if p[0] == "occ":
                    r = occlusion_rect(p[1], p[2], W, H)
                    if r is not None:
                        rects[i] = r
            _lib.check(lib.pm_aug_occlude_u8(out.data_ptr(), up("pt_rects", rects).data_ptr(), B, H, W, st), "pm_aug_occlude_u8")
        return out


class DeviceJpegDecoder:
    """Baseline JPEG decoding on the device (csrc/pm_jpeg.hip): `__call__(batch)` takes a jpeg.JpegBatch that is on the device and
    returns, on the current stream, the RaggedFrames that RaggedFrames.from_frames([folder.pil_loader(f) for f in files]) gives --
    `data`, `offset` and `hw` byte for byte.  Frames the device does not decode were decoded by the packer on the host and are
    copied into their slots.  The coefficient / plane workspace and the output only grow; the returned frames live in the output
    buffer until the next call enqueues its decode.
    mode="parallel" (pm_jpeg_decode_parallel): one lane per 128-byte subsequence of a restart interval, self-synchronising, with
    `sync_rounds` correction launches across workgroups; an interval whose lanes are not proven synchronised is decoded by one lane.
    mode="interval" (pm_jpeg_decode): one lane per restart interval.  Both return the same bytes.  `stats()` reads the counters
    of the last parallel call (one device read: tests and logging only)."""
    STATS = ("subsequences", "intervals", "sequential_intervals", "max_workgroup_steps", "rounds_changed")

    def __init__(self, device, mode: str = "parallel", sync_rounds: int = 2):
        if mode not in ("parallel", "interval"):
            raise ValueError("mode must be 'parallel' or 'interval'")
        if not 0 <= int(sync_rounds) <= 8:
            raise ValueError("sync_rounds must be in 0..8")
        self.device = torch.device(device)
        self.mode, self.sync_rounds = mode, int(sync_rounds)
        self._scratch = _Scratch(self.device)

    def stats(self) -> dict:
        """The counters of the last mode="parallel" call (synchronises with the device)."""
        t = self._scratch.bufs.get("stats")
        if t is None:
            raise _lib.PolypMaeError("DeviceJpegDecoder.stats(): no mode='parallel' call has been made")
        return dict(zip(self.STATS, t[:len(self.STATS)].tolist()))

    @staticmethod
    def _ptr(x: torch.Tensor):
        return x.data_ptr() if x.numel() else None

    @staticmethod
    def _check_batch(batch) -> None:
        from .jpeg import JpegBatch
        if not isinstance(batch, JpegBatch):
            raise TypeError("DeviceJpegDecoder takes a jpeg.JpegBatch")
        if not batch.is_cuda:
            raise _lib.PolypMaeError("DeviceJpegDecoder runs on the GPU only (no CPU fallback): move the JpegBatch to the device first")

    def _tables(self, batch) -> Tuple[tuple, torch.Tensor, torch.Tensor]:
        """What every decode entry takes first -- entropy, intervals, frames, huff and quant, each with its count -- and the
        grow-only coefficient and plane buffers."""
        t, n, ptr = batch.t, batch.meta["blocks"] * 64, self._ptr
        lead = (ptr(t["entropy"]), t["entropy"].numel(), ptr(t["intervals"]), t["intervals"].shape[0], ptr(t["frames"]),
                t["frames"].shape[0], ptr(t["huff"]), t["huff"].shape[0], ptr(t["quant"]), t["quant"].shape[0])
        return lead, self._scratch.grow("coef", n, torch.int16), self._scratch.grow("planes", n, torch.uint8)

    def _parallel_ws(self, batch) -> tuple:
        """What the parallel entries take last: subseq with its count, sync_rounds, the grow-only workspace with its size, `stats`."""
        t = batch.t
        need = _lib.workspace_bytes("pm_jpeg_decode_workspace", t["intervals"].shape[0], t["subseq"].numel())
        ws = self._scratch.grow("workspace", need, torch.uint8)
        stats = self._scratch.grow("stats", 8, torch.int32)
        return self._ptr(t["subseq"]), t["subseq"].numel(), self.sync_rounds, ws.data_ptr(), ws.numel(), stats.data_ptr()

    def resized_crop(self, batch, boxes, size: int, bicubic: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode straight into the resized crop: uint8 [B, size, size, 3] = DeviceAugmenter(size)._resized_crop(self(batch), boxes,
        bicubic) byte for byte, without the full-size RGB frames in between (no buffer of meta["nbytes"] is allocated).  The
        entropy stage and the inverse DCT are those of mode="parallel" (pm_jpeg_decode_planes); the crop's horizontal pass then
        reads the component planes -- or a host-decoded frame's bytes in `fallback` -- where they lie (pm_jpeg_resized_crop_u8).
        boxes: (top, left, h, w) int [B, 4], each inside its own frame (batch.meta["hw"])."""
        self._check_batch(batch)
        m, t, sc, ptr = batch.meta, batch.t, self._scratch, self._ptr
        B, S = len(batch), int(size)
        hw = m["hw"]
        if S <= 0:
            raise ValueError("size must be positive")
        boxes = _check_boxes(boxes, hw)
        if out is None:   # (grow-only, as the other buffers: a ragged last batch is a view of it)
            out = sc.grow("crop", B * S * S * 3, torch.uint8)[:B * S * S * 3].view(B, S, S, 3)
        elif tuple(out.shape) != (B, S, S, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != t["hw"].device:
            raise ValueError("`out` must be a contiguous uint8 [B, size, size, 3] tensor on the batch's device")
        # per sample: the frame row it is, or -1 - k for row k of the fallback table (both tables are in frame order)
        source = np.zeros(B, dtype=np.int32)
        on_host = np.zeros(B, dtype=bool)
        on_host[m["fallback"]] = True
        source[~on_host] = np.arange(B - int(on_host.sum()), dtype=np.int32)
        source[on_host] = -1 - np.arange(int(on_host.sum()), dtype=np.int32)
        box_d, src_d = sc.upload("crop_box", boxes), sc.upload("crop_source", source)
        lib = _lib.load()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        lead, coef, planes = self._tables(batch)
        _lib.check(lib.pm_jpeg_decode_planes(*lead, coef.data_ptr(), planes.data_ptr(), m["blocks"], *self._parallel_ws(batch), stream),
                   "pm_jpeg_decode_planes")
        Hmax, Wmax = (int(v) for v in hw.max(0))
        cws = sc.grow("crop_ws", _lib.workspace_bytes("pm_jpeg_resized_crop_workspace", B, Hmax, Wmax, S), torch.uint8)
        _lib.check(lib.pm_jpeg_resized_crop_u8(planes.data_ptr(), m["blocks"], ptr(t["frames"]), t["frames"].shape[0], ptr(t["fallback"]),
                                               t["fallback"].numel(), ptr(t["fallback_table"]), t["fallback_table"].shape[0],
                                               src_d.data_ptr(), t["hw"].data_ptr(), box_d.data_ptr(), out.data_ptr(),
                                               1 if bicubic else 0, B, Hmax, Wmax, S, cws.data_ptr(), cws.numel(), stream),
                   "pm_jpeg_resized_crop_u8")
        return out

    def __call__(self, batch) -> RaggedFrames:
        self._check_batch(batch)
        m, t, ptr = batch.meta, batch.t, self._ptr
        lead, coef, planes = self._tables(batch)
        out = self._scratch.grow("out", m["nbytes"], torch.uint8)
        args = lead + (ptr(t["fallback"]), t["fallback"].numel(), ptr(t["fallback_table"]), t["fallback_table"].shape[0],
                       coef.data_ptr(), planes.data_ptr(), m["blocks"], m["pixels"], out.data_ptr(), m["nbytes"])
        lib = _lib.load()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.mode == "interval":
            _lib.check(lib.pm_jpeg_decode(*args, stream), "pm_jpeg_decode")
        else:
            _lib.check(lib.pm_jpeg_decode_parallel(*args, *self._parallel_ws(batch), stream), "pm_jpeg_decode_parallel")
        return RaggedFrames(out[:m["nbytes"]], t["offset"], t["hw"], _host=(m["offset"], m["hw"]))


class DevicePrefetcher:
    """Wraps a loader that yields (frames, *rest) -- frames uint8 [B,H,W,3] or a RaggedFrames of mixed sizes, on the host --:
    copies batch i+1 to the device on a side stream (pinned staging, two slots) while batch i is consumed, and yields (imgs
    float32 [B,3,S,S] on the device, *rest on the device).  The yielded image tensor is a per-slot buffer that is refilled two
    batches later (consume it within the step, as a training loop does).  `flip_p > 0` draws per-sample horizontal / vertical flips
    (RandomHorizontalFlip / RandomVerticalFlip of the reference's train transform) from `generator`."""

    def __init__(self, loader: Iterable, device, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 flip_p: float = 0.0, generator: Optional[torch.Generator] = None, augment: Optional["DeviceAugmenter"] = None,
                 stream: str = "auto", transform: str = "train", perturb: Optional["DevicePerturber"] = None,
                 rest_to_device: bool = True, fused_decode: bool = False, eval_resize: int = 256):
        """augment: a DeviceAugmenter -> the loader may yield decoded frames of any size and a transform of the reference runs on
        the copy stream, drawing its parameters from `generator` (`flip_p` is then ignored):
          transform="train": the classification train transform (Resize, ColorJitter, GaussianBlur(25), flips,
                             RandomRotation(180), ToTensor, Normalize; classification/data/transforms.py:234-246);
          transform="mae":   the MAE pre-train transform (RandomResizedCrop(bicubic), RandomHorizontalFlip, ToTensor, Normalize;
                             mae/main_pretrain.py:156-160);
          transform="eval":  ClassificationTransforms(stage="val" / "test") (transforms.py:247-256): Resize((S, S)), the row
                             perturbations when a DevicePerturber is given as `perturb` (the rows are the LAST element of the
                             batch), ToTensor, Normalize -- into the slot's own f32 buffer; nothing random;
          transform="mae_eval": the validation transform of the MAE recipes (mae/main_linprobe.py:151-156): Resize(eval_resize,
                             bicubic) + CenterCrop(S) (DeviceAugmenter.resize_center_crop), ToTensor, Normalize -- no flips, nothing
                             random.  The batches are RaggedFrames or JpegBatch; fused_decode is refused (the variant that reads
                             the JPEG planes directly is not built).
        rest_to_device=False leaves the tensors after the frames (the labels) on the host: train.evaluate_cls reads the targets of
        every batch on the host, which is a device sync per batch when they were moved.
        fused_decode=True: a JpegBatch is not decoded to full-size RGB frames first; the decoder does the first stage of the
        transform itself (DeviceJpegDecoder.resized_crop: the whole-frame bilinear Resize of "train" and "eval", the
        RandomResizedCrop of "mae", its boxes drawn from the batch's sizes by the same generator calls in the same order), so every
        output byte equals fused_decode=False.  Other batches are not affected.
        Frames of mixed decoded sizes -- an image folder such as Hyperkvasir-unlabelled -- arrive as a RaggedFrames (see
        `ragged_collate`): one host-to-device copy of the packed bytes plus the two small offset / size tables, then the per-sample
        resized crop (pm_aug_resized_crop_ragged_u8: the Resize of "train" is a crop with the whole frame as its box) brings every
        frame to S x S on the device, and the rest of the chain is the uniform one.  A batch of compressed files (jpeg.JpegBatch,
        `folder_loader(..., decode="device")`) is decoded on the copy stream (DeviceJpegDecoder) into the RaggedFrames the ragged
        path then takes.  Every kind of batch is staged the same way (`_stage_tensors`), one copy per tensor: the pinned and device
        staging buffers are kept per slot and per name and only ever grow, and a batch that arrives pinned
        (DataLoader(pin_memory=True)) is copied from where it lies.  Without `augment`, uniform [B, H, W, 3] batches get the fused
        flips + ToTensor + Normalize of pm_preprocess_u8 only.
        stream: where the copies and the transform run -- "own": a stream of the prefetcher (a fourth busy stream beside the
        engine's three: one hardware queue each, fastest on a single GPU); "side": the engine's weight-gradient stream (idle
        during the forward pass, when the next batch is staged) -- for data-parallel ranks, where RCCL's stream is the fourth busy
        one and a fifth would share a queue with the main stream (13.9 instead of 11.6 ms per step measured);
        "auto": "side" when a torch.distributed process group is initialised, "own" otherwise."""
        if stream not in ("auto", "own", "side"):
            raise ValueError("stream must be 'auto', 'own' or 'side'")
        if transform not in ("train", "mae", "eval", "mae_eval"):
            raise ValueError("transform must be 'train', 'mae', 'eval' or 'mae_eval'")
        if transform == "mae_eval" and fused_decode:
            raise ValueError("transform='mae_eval' does not take fused_decode=True: the Resize + CenterCrop that reads the decoder's "
                             "component planes directly is not built; the batch is decoded to RGB frames first")
        if transform in ("mae", "eval", "mae_eval") and augment is None:
            raise ValueError(f"transform='{transform}' needs a DeviceAugmenter (augment=...)")
        if perturb is not None and transform != "eval":
            raise ValueError("perturb=... applies to transform='eval' only")
        self.stream_mode, self.transform = stream, transform
        self.perturb, self.rest_to_device, self.fused_decode = perturb, bool(rest_to_device), bool(fused_decode)
        self.loader, self.device = loader, torch.device(device)
        self.mean, self.std, self.flip_p, self.generator = mean, std, float(flip_p), generator
        self.augment, self.eval_resize = augment, int(eval_resize)
        self._pin = [{}, {}]        # per slot: pinned staging tensors by name, flat and grow-only
        self._dev = [{}, {}]        # per slot: device staging tensors by name, flat and grow-only
        self._out = [None, None]    # per slot: the float32 images
        self._decoder: Optional[DeviceJpegDecoder] = None
        self._consumed = [None, None]   # per slot: event recorded on the consumer's stream after it used the batch
        self._slot_copied = [None, None]  # per slot: event after the slot's host-to-device copies were enqueued
        self._stream: Optional[torch.cuda.Stream] = None

    def __len__(self):
        return len(self.loader)

    def _stage_tensors(self, slot: int, named: dict, pinned: bool) -> dict:
        """One host-to-device copy per tensor into this slot's grow-only device buffer of that name -- through the slot's grow-only
        pinned buffer of that name unless the batch arrived pinned (then it is copied from where it lies) -- and views of the
        device copies in the tensors' own shapes.  A name that held another dtype gets a new buffer.  Called on the copy stream."""
        def front(bufs: dict, name: str, like: torch.Tensor, device) -> torch.Tensor:   # (device None: pinned host memory)
            b, n = bufs.get(name), like.numel()
            if b is None or b.numel() < n or b.dtype != like.dtype:
                b = bufs[name] = torch.empty(max(n, 1), dtype=like.dtype, device=device, pin_memory=device is None)
            return b[:n].view(like.shape)

        staged = {}
        for name, t in named.items():
            if not pinned:
                host = front(self._pin[slot], name, t, None)
                host.copy_(t)
                t = host
            staged[name] = front(self._dev[slot], name, t, self.device)
            staged[name].copy_(t, non_blocking=True)
        return staged

    def _decode(self, batch):
        """A staged jpeg.JpegBatch -> the decoded RaggedFrames or, with fused_decode, the uint8 [B, S, S, 3] batch after the first
        stage of the transform, which the decoder then does itself.  Called on the copy stream."""
        if self._decoder is None:
            self._decoder = DeviceJpegDecoder(self.device)
        if not self.fused_decode:
            return self._decoder(batch)
        hw = batch.meta["hw"]
        if self.transform == "mae":   # (the draws of DeviceAugmenter.random_resized_crop)
            return self._decoder.resized_crop(batch, draw_rrc_boxes(len(batch), hw[:, 0], hw[:, 1], self.generator),
                                              self.augment.size, True)
        return self._decoder.resized_crop(batch, _whole_frame_boxes(hw), self.augment.size, False)   # (DeviceAugmenter.resize)

    def _transform(self, x, rest: Tuple, out: torch.Tensor, cropped: bool = False) -> torch.Tensor:
        """The slot's transform on the copy stream.  x: decoded frames (uniform or ragged) or, cropped=True, the uint8 [B, S, S, 3]
        batch a fused decode already brought through the first stage (the Resize of "train" / "eval" passes it on as it is)."""
        if self.transform == "mae":
            if cropped:
                return self.augment.mae_tail(x, generator=self.generator, out=out)
            return self.augment.mae_transform(x, generator=self.generator, out=out)
        if self.transform == "mae_eval":
            if not isinstance(x, RaggedFrames):
                raise ValueError("transform='mae_eval' takes RaggedFrames or JpegBatch batches")
            return preprocess_u8(self.augment.resize_center_crop(x, self.eval_resize), None, self.mean, self.std, out=out)
        if self.transform == "eval":
            x = self.augment.resize(x)
            if self.perturb is not None and rest[-1] is not None:
                x = self.perturb(x, rest[-1])
            return preprocess_u8(x, None, self.mean, self.std, out=out)
        return self.augment(x, generator=self.generator, out=out)

    def _rest(self, rest: Tuple) -> Tuple:
        if not self.rest_to_device:
            return rest
        return tuple(t.to(self.device, non_blocking=True) if torch.is_tensor(t) else t for t in rest)

    def _stage(self, slot: int, batch) -> Tuple:
        from .jpeg import JpegBatch
        frames, rest = batch[0], tuple(batch[1:])
        compressed, ragged = isinstance(frames, JpegBatch), isinstance(frames, RaggedFrames)
        if compressed or ragged:
            if self.augment is None:
                raise ValueError("a RaggedFrames or JpegBatch batch needs a DeviceAugmenter (augment=...) to bring its frames to one size")
            named = frames.t if compressed else {"data": frames.data, "offset": frames.offset, "hw": frames.hw}
        else:
            if frames.dtype != torch.uint8:
                raise ValueError("DevicePrefetcher expects uint8 HWC frames from the loader")
            named = {"frames": frames}
        B = len(frames)
        shape = (B, 3, self.augment.size, self.augment.size) if self.augment is not None else (B, 3) + tuple(frames.shape[1:3])
        f8 = None
        if self.flip_p > 0 and self.augment is None:
            r = torch.rand(2, B, generator=self.generator)
            f8 = ((r[0] < self.flip_p).to(torch.uint8) | ((r[1] < self.flip_p).to(torch.uint8) << 1))
        # the buffers are owned per slot and reused (no allocator traffic on the copy stream in the steady state): the copy stream
        # first waits until the consumer's work on the batch that last used this slot has been enqueued AND executed
        out = self._out[slot]
        if out is None or out.shape != shape:   # (allocated outside the copy stream: it is the consumer's stream that reads it last)
            out = self._out[slot] = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.stream(self._stream):
            if self._consumed[slot] is not None:
                self._stream.wait_event(self._consumed[slot])
            x = self._stage_tensors(slot, named, frames.is_pinned())   # (DataLoader(pin_memory=True): no staging copy)
            if compressed:
                x = self._decode(JpegBatch(x, frames.meta))
            elif ragged:
                x = RaggedFrames(x["data"], x["offset"], x["hw"], _host=frames._host)
            else:
                x = x["frames"]
            if self.augment is not None:
                imgs = self._transform(x, rest, out, cropped=compressed and self.fused_decode)
            else:   # (the flags go through pinned memory too: a pageable host-to-device copy is synchronous and would stall the
                # enqueue of the step)
                fl = self._stage_tensors(slot, {"flips": f8}, False)["flips"] if f8 is not None else None
                imgs = preprocess_u8(x, fl, self.mean, self.std, out=out)
            rest_dev = self._rest(rest)
            ev = torch.cuda.Event()
            ev.record(self._stream)
            self._slot_copied[slot] = ev
        return imgs, rest_dev, ev

    def __iter__(self) -> Iterator:
        if self.device.type != "cuda":
            raise _lib.PolypMaeError("DevicePrefetcher needs a GPU (the transform tail is a HIP kernel)")
        if self._stream is None:
            mode = self.stream_mode
            if mode == "auto":
                import torch.distributed as dist
                mode = "side" if dist.is_available() and dist.is_initialized() else "own"
            if mode == "side":
                from .engine import _shared_stream
                self._stream = _shared_stream(self.device, "side")
            else:
                self._stream = torch.cuda.Stream(device=self.device)
        it = iter(self.loader)
        # Staging runs on a worker thread: the pinned-memory copy and the host-to-device enqueue block their caller for
        # about as long as a CPU memcpy of the batch (1 ms per 64 frames measured), and the main thread must spend that
        # time enqueueing the training step instead.
        pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)

        def job(slot, batch):
            torch.cuda.set_device(self.device)
            # this slot's pinned buffers (frames and / or flip flags) were last read by the copies issued two batches ago,
            # which wait on the consumer's event and may not have executed yet: drain them before the host rewrites them
            if self._slot_copied[slot] is not None:
                self._slot_copied[slot].synchronize()
            return self._stage(slot, batch)

        try:
            slot = 0
            try:
                fut = pool.submit(job, slot, next(it))
            except StopIteration:
                return
            while fut is not None:
                imgs, rest, ev = fut.result()
                cur, slot = slot, slot ^ 1
                try:
                    fut = pool.submit(job, slot, next(it))
                except StopIteration:
                    fut = None
                main = torch.cuda.current_stream(self.device)
                main.wait_event(ev)
                for t in rest:
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(main)
                yield (imgs,) + rest
                # the consumer has enqueued its work on this batch: the slot's buffers may be refilled once that work ran
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self.device))
                self._consumed[cur] = done
        finally:
            pool.shutdown(wait=True)
