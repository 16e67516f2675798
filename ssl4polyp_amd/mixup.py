"""Batch mixing and its loss for the MAE fine-tune recipe (mae/main_finetune.py:240-247, 312-318; engine_finetune.py:53-58): the
call surface of timm 0.4.12's `Mixup` in mode "batch" and `SoftTargetCrossEntropy` over its targets, on the device.

The host draws one (lam, use_cutmix, box) per batch and writes it into a small device record through pinned memory with an
asynchronous copy; pm_mix_batch mixes the images in place from that record and pm_soft_ce builds the mixed, smoothed target row of
every sample on the fly from the int64 labels -- the [B, C] soft targets timm materialises never exist.  Nothing here reads a device
value back.

timm is not a dependency of this package and was not available when this was written: the draw order below (Mixup._params_per_batch,
rand_bbox, cutmix_bbox_and_lam with correct_lam) is RESTATED from timm 0.4.12's source and HAS NOT BEEN CHECKED AGAINST timm ITSELF
(no run of timm was recorded); tests/test_finetune_mae_cpu.py pins it to a hand-computed sequence from a seeded RandomState."""
from __future__ import annotations

import struct
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import _ptr, _stream


def rand_bbox(img_shape, lam: float, rng) -> Tuple[int, int, int, int]:
    """timm rand_bbox (margin 0): ratio = sqrt(1 - lam); cut = int(side * ratio); the centre cy = randint(0, H), then cx =
    randint(0, W); the box is centre -/+ cut // 2 clipped to the image.  -> (yl, yh, xl, xh)."""
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    cy = int(rng.randint(0, img_h))
    cx = int(rng.randint(0, img_w))
    yl = int(np.clip(cy - cut_h // 2, 0, img_h))
    yh = int(np.clip(cy + cut_h // 2, 0, img_h))
    xl = int(np.clip(cx - cut_w // 2, 0, img_w))
    xh = int(np.clip(cx + cut_w // 2, 0, img_w))
    return yl, yh, xl, xh


def cutmix_bbox_and_lam(img_shape, lam: float, rng, correct_lam: bool = True):
    """timm cutmix_bbox_and_lam without ratio_minmax: the box of rand_bbox and lam = 1 - area / (H W)."""
    yl, yh, xl, xh = rand_bbox(img_shape, lam, rng)
    if correct_lam:
        lam = 1.0 - (yh - yl) * (xh - xl) / float(img_shape[-2] * img_shape[-1])
    return (yl, yh, xl, xh), lam


class MixState:
    """The draw of one batch: `record` is the device copy (pm_mix_record: eight 4-byte words) the kernels read; lam / use_cutmix /
    box are the host's values of the same draw."""

    SLOTS = 4

    def __init__(self, device):
        self.device = torch.device(device)
        self.record = torch.zeros(8, dtype=torch.int32, device=self.device)
        self._pin = [torch.zeros(8, dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)] if self.device.type == "cuda" else None
        self._ev = [None] * self.SLOTS
        self._slot = 0
        self.lam, self.use_cutmix, self.box = 1.0, False, (0, 0, 0, 0)
        self.write(1.0, False, (0, 0, 0, 0))

    @staticmethod
    def pack(lam: float, use_cutmix: bool, box) -> np.ndarray:
        """The record's eight words: f32(lam), f32(1 - lam) -- each rounded from the double, as torch rounds a Python scalar --
        use_cutmix, yl, yh, xl, xh, 0."""
        yl, yh, xl, xh = (int(v) for v in box)
        return np.frombuffer(struct.pack("<ffiiiiii", float(lam), 1.0 - float(lam), 1 if use_cutmix else 0, yl, yh, xl, xh, 0),
                             dtype=np.int32).copy()

    def write(self, lam: float, use_cutmix: bool, box) -> None:
        """Host -> device without a sync: a pinned slot, an asynchronous copy on the current stream, one event per slot (a slot is
        rewritten only after its previous copy has run), as FusedAdamW.sync_hyper does."""
        self.lam, self.use_cutmix, self.box = float(lam), bool(use_cutmix), tuple(int(v) for v in box)
        words = torch.from_numpy(self.pack(lam, use_cutmix, box))
        if self._pin is None:
            self.record.copy_(words)
            return
        i = self._slot
        self._slot = (i + 1) % self.SLOTS
        if self._ev[i] is not None:
            self._ev[i].synchronize()
        self._pin[i].copy_(words)
        self.record.copy_(self._pin[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._ev[i] = ev

    @property
    def identity(self) -> bool:
        return self.lam == 1.0 and not self.use_cutmix


def mix_batch(x: torch.Tensor, state: MixState, enabled: Optional[bool] = None) -> torch.Tensor:
    """pm_mix_batch: x f32 [B, C, H, W] on the device, in place, from state.record.  enabled=None: launch unless the host's draw
    is the identity; True: always launch (a captured step, whose record changes between replays)."""
    if x.dtype != torch.float32 or x.device.type != "cuda" or x.ndim != 4 or not x.is_contiguous():
        raise _lib.PolypMaeError(f"mix_batch: needs a contiguous f32 [B, C, H, W] tensor on the GPU (got {x.dtype} {tuple(x.shape)} on {x.device})")
    B, C, H, W = x.shape
    if B % 2:
        raise ValueError("Batch size should be even when using this")   # timm's assertion
    on = (not state.identity) if enabled is None else bool(enabled)
    _lib.check(_lib.load().pm_mix_batch(_ptr(x), B, C, H, W, _ptr(state.record), 1 if on else 0, _stream()), "pm_mix_batch")
    return x


class Mixup:
    """timm 0.4.12 `Mixup(mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, mode, correct_lam, label_smoothing,
    num_classes)`, mode "batch" only.  `mixup(x, target) -> (x, target)`: x is mixed IN PLACE on the device, the int64 target comes
    back as it is, and `mixup.state` holds the draw for soft_target_ce (timm returns the [B, C] soft targets instead).

    Draw order per batch, from `rng` (a numpy.random.RandomState; None: numpy's global one, as timm): rand() < prob; if both
    alphas are > 0, rand() < switch_prob picks CutMix; beta(alpha, alpha) of the chosen kind; for CutMix rand_bbox (randint for cy,
    then cx) and lam = 1 - area / (H W).  This order is restated from timm's source and has not been checked against timm itself
    (see the module docstring).  Modes "pair" / "elem" and cutmix_minmax are not built: refused."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, cutmix_minmax=None, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", correct_lam: bool = True, label_smoothing: float = 0.1,
                 num_classes: int = 1000, rng=None):
        if mode != "batch":
            raise NotImplementedError(f"Mixup mode {mode!r}: only 'batch' is built (one draw per batch; 'pair' / 'elem' draw per sample "
                                      "and would need a per-sample device record)")
        if cutmix_minmax is not None:
            raise NotImplementedError("Mixup cutmix_minmax (timm's rand_bbox_minmax) is not built: use cutmix_alpha")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(prob), float(switch_prob)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.mode, self.correct_lam = mode, bool(correct_lam)
        self.mixup_enabled = True
        self.rng = rng
        self.state: Optional[MixState] = None

    def _params_per_batch(self) -> Tuple[float, bool]:
        rng = self.rng if self.rng is not None else np.random
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and rng.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(rng.rand() < self.switch_prob)
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam_mix = rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.0:
                use_cutmix = True
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                raise AssertionError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")
            lam = float(lam_mix)
        return lam, use_cutmix

    def draw(self, img_shape) -> Tuple[float, bool, Tuple[int, int, int, int]]:
        """(lam, use_cutmix, box) of the next batch: Mixup._mix_batch's host side.  lam == 1 from the first draw means no mixing of
        either kind (timm returns before the box is drawn)."""
        lam, use_cutmix = self._params_per_batch()
        box = (0, 0, 0, 0)
        if lam == 1.0:
            return 1.0, False, box
        if use_cutmix:
            box, lam = cutmix_bbox_and_lam(img_shape, lam, self.rng if self.rng is not None else np.random, self.correct_lam)
        return lam, use_cutmix, box

    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        if len(x) % 2:
            raise ValueError("Batch size should be even when using this")
        if self.state is None or self.state.device != x.device:
            self.state = MixState(x.device)
        self.state.write(*self.draw(x.shape))
        mix_batch(x, self.state)
        return x, target


def soft_ce_raw(logits, target, record: Optional[torch.Tensor], smoothing: float, scale: Optional[torch.Tensor], want_grad: bool):
    """pm_soft_ce -> (loss f32 [1], dlogits [B, C] x scale or None)."""
    if logits.dtype != torch.float32 or logits.device.type != "cuda" or logits.ndim != 2:
        raise _lib.PolypMaeError(f"soft_target_ce: logits must be f32 [B, C] on the GPU (got {logits.dtype} on {logits.device})")
    logits = logits.contiguous()
    B, C = logits.shape
    if target.dtype != torch.int64 or target.shape != (B,):
        raise _lib.PolypMaeError(f"soft_target_ce: targets must be int64 [{B}] (got {target.dtype} {tuple(target.shape)})")
    target = target.contiguous()
    lib = _lib.load()
    dev = logits.device
    ws = torch.empty((_lib.workspace_bytes("pm_soft_ce_workspace", B) + 3) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dlogits = torch.empty(B, C, dtype=torch.float32, device=dev) if want_grad else None
    _lib.check(lib.pm_soft_ce(_ptr(logits), _ptr(target), B, C, _ptr(record), float(smoothing), _ptr(scale), _ptr(loss), _ptr(dlogits),
                              _ptr(ws), ws.numel() * 4, _stream()), "pm_soft_ce")
    return loss, dlogits


class _SoftCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, record, smoothing, scale):
        loss, dlogits = soft_ce_raw(logits, target, record, smoothing, scale, ctx.needs_input_grad[0])
        ctx.dlogits = dlogits
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        # the gradient left by the forward already carries `scale`; `dloss` is the 1.0 of loss.backward() or, through
        # LossScaler.scale, the loss scale: a device scalar either way (pm_scale)
        d = ctx.dlogits
        out = torch.empty_like(d)
        dloss = dloss.reshape(1).contiguous().float()
        _lib.check(_lib.load().pm_scale(_ptr(d), _ptr(dloss), _ptr(out), d.numel(), _stream()), "pm_scale")
        ctx.dlogits = None
        return out, None, None, None, None


def soft_target_ce(logits: torch.Tensor, target: torch.Tensor, mix_state: Optional[MixState] = None, smoothing: float = 0.0,
                   scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """timm's SoftTargetCrossEntropy()(logits, mixup_target(target, C, lam, smoothing)) as a 0-d tensor, from the int64 labels and
    the draw in `mix_state` (None: lam = 1 -- LabelSmoothingCrossEntropy(smoothing), or plain cross-entropy at smoothing 0).
    `scale`: a device scalar the GRADIENT is multiplied by (1 / accum_iter); the returned loss is the undivided one, what the
    reference logs (so do not divide it by accum_iter again); the backward multiplies by the upstream gradient, so
    LossScaler.scale(loss).backward() carries the loss scale."""
    if scale is None:
        scale = torch.ones((), dtype=torch.float32, device=logits.device)
    return _SoftCeFn.apply(logits, target, mix_state.record if mix_state is not None else None, float(smoothing), scale)
