"""Linear probing of a frozen encoder (mae/main_linprobe.py) on the device: the global_pool feature, the BatchNorm1d + Linear head of
main_linprobe.py:244, softmax cross-entropy with the accuracy counts of engine_finetune.evaluate.  Each op is one call into
csrc/pm_probe.hip (f32, fixed summation order); a missing kernel is an error, there is no eager path.

The head, its loss and LARS (optim.FusedLARS) run in f32 in every precision mode; only the encoder follows the configured mode."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _lib
from .engine import _ptr, _stream

BN_EPS = 1e-6       # main_linprobe.py:244
BN_MOMENTUM = 0.1   # torch.nn.BatchNorm1d's default


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.device.type != "cuda":
        raise _lib.PolypMaeError(f"{what}: needs an f32 tensor on the GPU (got {t.dtype} on {t.device})")
    return t.contiguous()


def pool_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """models_vit.py:46-48 (global_pool): fc_norm(x[:, 1:, :].mean(dim=1)).  x f32 [B, N, D]: the last block's output, without the
    final norm.  Forward only."""
    x, gamma, beta = _f32(x.detach(), "pool_norm x"), _f32(gamma.detach(), "pool_norm weight"), _f32(beta.detach(), "pool_norm bias")
    B, N, D = x.shape
    lib = _lib.load()
    ws = torch.empty((_lib.workspace_bytes("pm_pool_norm_workspace", B, N, D) + 3) // 4, dtype=torch.float32, device=x.device)
    feat = torch.empty(B, D, dtype=torch.float32, device=x.device)
    _lib.check(lib.pm_pool_norm_fwd(_ptr(x), B, N, D, _ptr(gamma), _ptr(beta), float(eps), _ptr(feat), _ptr(ws), ws.numel() * 4,
                                    _stream()), "pm_pool_norm_fwd")
    return feat


def probe_head_fwd(feat, weight, bias, running_mean, running_var, num_batches_tracked, training: bool,
                   momentum: float = BN_MOMENTUM, eps: float = BN_EPS):
    """-> (logits [B, C], xhat [B, D]).  Training mode updates the three buffers in place, as torch.nn.BatchNorm1d does."""
    feat = _f32(feat, "probe head features")
    B, D = feat.shape
    C = weight.shape[0]
    if training and B < 2:  # torch: "Expected more than 1 value per channel when training"
        raise ValueError(f"probe head: training-mode BatchNorm needs more than 1 sample per batch (got B = {B})")
    if num_batches_tracked.dtype != torch.int64:
        raise _lib.PolypMaeError("probe head: num_batches_tracked must be int64")
    xhat = torch.empty(B, D, dtype=torch.float32, device=feat.device)
    logits = torch.empty(B, C, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().pm_probe_head_fwd(_ptr(feat), B, D, C, _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                                             _ptr(num_batches_tracked), 1 if training else 0, float(momentum), float(eps),
                                             _ptr(xhat), _ptr(logits), _stream()), "pm_probe_head_fwd")
    return logits, xhat


def probe_head_bwd(dlogits, xhat, dW, dbias) -> None:
    """dW += dlogits^T xhat, dbias += sum_b dlogits."""
    B, C = dlogits.shape
    _lib.check(_lib.load().pm_probe_head_bwd(_ptr(dlogits), _ptr(xhat), B, xhat.shape[1], C, _ptr(dW), _ptr(dbias), _stream()),
               "pm_probe_head_bwd")


def probe_ce_raw(logits, target, scale: Optional[torch.Tensor], want_grad: bool):
    """-> (loss f32 [1], dlogits [B, C] x scale or None, correct int64 [2]: at 1 and at min(5, C))."""
    logits = _f32(logits, "probe_ce logits")
    B, C = logits.shape
    if target.dtype != torch.int64 or target.shape != (B,):
        raise _lib.PolypMaeError(f"probe_ce: targets must be int64 [{B}] (got {target.dtype} {tuple(target.shape)})")
    target = target.contiguous()
    lib = _lib.load()
    dev = logits.device
    ws = torch.empty((_lib.workspace_bytes("pm_probe_ce_workspace", B) + 3) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    correct = torch.empty(2, dtype=torch.int64, device=dev)
    dlogits = torch.empty(B, C, dtype=torch.float32, device=dev) if want_grad else None
    _lib.check(lib.pm_probe_ce(_ptr(logits), _ptr(target), B, C, _ptr(scale), _ptr(loss), _ptr(dlogits), _ptr(correct), _ptr(ws),
                               ws.numel() * 4, _stream()), "pm_probe_ce")
    return loss, dlogits, correct


class _ProbeHeadFn(torch.autograd.Function):
    """features -> logits through BatchNorm1d(affine=False) + Linear.  The backward ADDS the two weight gradients into
    weight.grad / bias.grad (created as zeros when absent): the kernel's `+=` is what gradient accumulation relies on."""

    @staticmethod
    def forward(ctx, feat, head: "ProbeHead", weight, bias):  # (weight / bias: the graph edges autograd reaches the backward by)
        bn, lin = head[0], head[1]
        logits, xhat = probe_head_fwd(feat, lin.weight.detach(), lin.bias.detach(), bn.running_mean, bn.running_var,
                                      bn.num_batches_tracked, head.training, bn.momentum, bn.eps)
        ctx.head, ctx.xhat = head, xhat
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lin = ctx.head[1]
        for p in (lin.weight, lin.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        probe_head_bwd(dlogits.contiguous().float(), ctx.xhat, lin.weight.grad, lin.bias.grad)
        ctx.xhat = None
        return None, None, None, None


class _BatchStats(nn.Module):
    """The buffers of torch.nn.BatchNorm1d(affine=False): same names, same initial values."""

    def __init__(self, num_features: int, eps: float = BN_EPS, momentum: float = BN_MOMENTUM):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class ProbeHead(nn.Sequential):
    """main_linprobe.py:244: Sequential(BatchNorm1d(D, affine=False, eps=1e-6), Linear(D, C)), state-dict keys `0.running_mean`,
    `0.running_var`, `0.num_batches_tracked`, `1.weight`, `1.bias`; train() / eval() select the BatchNorm mode."""

    def __init__(self, linear: nn.Linear):
        super().__init__(_BatchStats(linear.in_features), linear)

    def forward(self, feat: torch.Tensor) -> torch.Tensor:
        if feat.requires_grad:
            raise _lib.PolypMaeError("probe head: the features require a gradient, but the linear probe has none with respect to "
                                     "its input (the encoder is frozen): detach them")
        lin = self[1]
        return _ProbeHeadFn.apply(feat, self, lin.weight, lin.bias)


class _ProbeCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, scale):
        loss, dlogits, correct = probe_ce_raw(logits, target, scale, ctx.needs_input_grad[0])
        ctx.dlogits = dlogits
        ctx.mark_non_differentiable(correct)
        return loss.reshape(()), correct

    @staticmethod
    def backward(ctx, dloss, _):
        # the gradient left by the forward already carries `scale`; `dloss` is the 1.0 of loss.backward()
        return ctx.dlogits, None, None


def probe_ce(logits: torch.Tensor, target: torch.Tensor, scale: Optional[torch.Tensor] = None):
    """torch.nn.CrossEntropyLoss()(logits, target) -> (loss, correct): the mean loss as a 0-d tensor and int64 [2], the samples
    correct at 1 and at min(5, C).  `scale`: a device scalar the GRADIENT is multiplied by (1 / accum_iter: engine_finetune divides
    the loss before backward); the returned loss is the undivided one, what the reference logs.  Call `loss.backward()` directly:
    the upstream gradient is taken as 1."""
    if scale is None:
        scale = torch.ones((), dtype=torch.float32, device=logits.device)
    return _ProbeCeFn.apply(logits, target, scale)
