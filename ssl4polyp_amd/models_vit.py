"""The ViT of the MAE linear-probe / fine-tune entry points (mae/models_vit.py) on the encoder runtime of this package, and what
mae/main_linprobe.py does to it: the BatchNorm + Linear probe head and the loading of a pre-training checkpoint.  With the plain
Linear head it is built with, the model is the trainable classifier of mae/main_finetune.py (_VitFinetuneFn, csrc/pm_finetune.hip;
load_pretrained_for_finetune); what follows describes the probe.

State-dict keys are the reference's: cls_token, pos_embed, patch_embed.*, blocks.*, norm.* (cls token) or fc_norm.* (global_pool),
head.weight, head.bias -- and head.0.running_mean / running_var / num_batches_tracked, head.1.weight / bias after add_probe_head.
The features come from the existing forward-only path: with the cls token exactly what a `head=False` classifier of models.py
returns (the same op on the same kernels); with global_pool the block stack's output through pm_pool_norm_fwd.  The encoder is
frozen in this protocol, so the feature pass records nothing for a backward; the head, its loss and LARS run in f32 whatever the
encoder's precision mode."""
from __future__ import annotations

from functools import partial
from typing import Optional

import torch
from torch import nn

from . import _lib
from .engine import BlockStack, StackGeom, _ptr, _stream
from .models import (_DEFAULT_PRECISION, Block, PatchEmbed, _ClassifierBase, _EncoderFrontMixin, _Needs, _Runtime, _plan_grads,
                     _update_gate)
from .probe import ProbeHead, pool_norm


class VisionTransformer(_ClassifierBase):
    """mae/models_vit.py:20-53 (timm 0.4.12 VisionTransformer + global_pool), same seeded initialisation order as
    models.VisionTransformer_from_Any.  With the probe head (add_probe_head) forward(imgs) = head(forward_features(imgs)) over the
    frozen, forward-only encoder; with the plain Linear it is built with, forward is the trainable classifier of the fine-tune
    recipe (main_finetune.py), one autograd node over the engine.
    drop_path_rate: stochastic depth as the reference builds it (main_finetune.py:251; timm 0.4.12 DropPath): block i of `depth`
    drops each of its two residual branches per sample with probability drop_path_rates[i] = linspace(0, rate, depth)[i] while the
    model is in training mode, and scales the kept ones by 1 / (1 - p_i).  The trainable classifier only: the probe's forward-only
    feature path never drops.  Rate 0.0 (the default) and eval() run exactly the launches of a model built without the argument."""

    def __init__(self, img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_classes=1000, global_pool=False,
                 precision: Optional[str] = None, drop_path_rate: float = 0.0):
        super().__init__()
        drop_path_rate = float(drop_path_rate)
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1) (got {drop_path_rate})")
        self.drop_path_rate = drop_path_rate
        # timm 0.4.12 vision_transformer.py: dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.drop_path_rates = [float(v) for v in torch.linspace(0, drop_path_rate, depth)]
        self.last_drop_scales: Optional[torch.Tensor] = None   # the scale table of the last training forward (f32 [depth, 2, B])
        self._drop_rates_dev: Optional[torch.Tensor] = None
        norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.num_features = self.embed_dim = embed_dim
        self.global_pool = bool(global_pool)
        self.patch_embed = PatchEmbed(img_size, patch_size, 3, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, 4.0, qkv_bias=True, norm_layer=norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        for name, m in self.named_modules():
            if isinstance(m, nn.Linear):
                if name == "head":   # timm 0.4.12 _init_vit_weights: name.startswith('head') -> zeros
                    nn.init.zeros_(m.weight)
                else:
                    nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.zeros_(m.bias)
                nn.init.ones_(m.weight)
        if self.global_pool:   # models_vit.py:27-32
            self.fc_norm = norm_layer(embed_dim)
            del self.norm
        self.dense, self.out_token, self._learned_pos = None, "cls", True
        enc = StackGeom(embed_dim, num_heads, depth, int(embed_dim * 4))
        object.__setattr__(self, "_rt", _Runtime(self, precision or _DEFAULT_PRECISION, enc, None))

    @torch.no_grad()
    def forward_features(self, imgs: torch.Tensor) -> torch.Tensor:
        """f32 [B, D], detached: norm(x)[:, 0], or fc_norm(x[:, 1:].mean(1)) with global_pool.  Never drops a path, whatever
        drop_path_rate and the training flag say: the probe's encoder is frozen and forward-only."""
        rt = self._rt
        rt.ensure(imgs.device)
        assert imgs.shape[2] == self.patch_embed.img_size[0] and imgs.shape[3] == self.patch_embed.img_size[1]
        if not self.global_pool:
            from . import ops
            return torch.ops.polypmae.vit_forward(imgs, ops.register_runtime(rt), 0, False, list(rt.flat.params))
        f = rt.flat
        return pool_norm(self.forward_tokens(imgs), f.param_view("fc_norm.weight"), f.param_view("fc_norm.bias"), rt.eps)

    @torch.no_grad()
    def forward_tokens(self, imgs: torch.Tensor) -> torch.Tensor:
        """f32 [B, N, D]: the output of the last block, before any final norm (a copy: the workspace goes back to the pool).  Like
        forward_features it never drops a path."""
        rt = self._rt
        rt.ensure(imgs.device)
        k, g = rt.k, rt.enc_geom
        B, L = imgs.shape[0], self.patch_embed.num_patches
        _, x0 = _EncoderFrontMixin.front_fwd(rt, imgs.contiguous().float(), None, L)
        ws = rt.get_ws(g, B, L + 1, False)
        W, _ = rt.stack_weights("blocks.", g.depth)
        x = BlockStack(k, g).forward(ws, x0, W, before_block=_update_gate(rt, "blocks."), keep_from=g.depth, cls_top=False)
        rt.wait_updates()
        x = x.view(B, L + 1, g.dim).clone()
        rt.put_ws(g, ws)
        return x

    def no_weight_decay(self):
        """timm 0.4.12 VisionTransformer.no_weight_decay (main_finetune.py:306)."""
        return {"pos_embed", "cls_token"}

    @property
    def drop_path_active(self) -> bool:
        """Does the next forward of the trainable classifier draw a scale table?  In training mode at a rate above 0 only."""
        return bool(self.training and self.drop_path_rate > 0.0)

    def _draw_drop_scales(self, B: int, device) -> torch.Tensor:
        """The scale table f32 [depth, 2, B] of one training forward: depth * 2 * B uniforms from pm_mae_noise, keyed like
        MaskedAutoencoderViT._draw_noise (seed and running offset of torch's device generator, the offset advanced by the numbers
        drawn, rounded up to 4: re-seeding replays the tables, consecutive forwards differ), then pm_drop_path_scales: sample b keeps
        branch j of block i when fl32(keep_i + u) >= 1 and is scaled by fl32(1 / keep_i), as timm's drop_path computes it."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PolypMaeError("ViT forward with stochastic depth under stream capture: the drop-path draw would be baked into "
                                     "the graph (the same paths dropped at every replay) -- pass `drop_scales=` from a buffer the "
                                     "caller refills between replays")
        depth = len(self.drop_path_rates)
        n = depth * 2 * B
        index = device.index if device.index is not None else torch.cuda.current_device()
        gen = torch.cuda.default_generators[index]
        seed = int(gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        off = int(gen.get_offset())
        gen.set_offset(off + 4 * ((n + 3) // 4))   # (multiples of 4, as the generator requires)
        key = (seed ^ ((off >> 32) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
        lib = self._rt.k.lib
        rates = self._drop_rates_dev
        if rates is None or rates.device != device:
            rates = self._drop_rates_dev = torch.tensor(self.drop_path_rates, dtype=torch.float32, device=device)
        noise = torch.empty(depth, 2, B, dtype=torch.float32, device=device)
        scales = torch.empty_like(noise)
        _lib.check(lib.pm_mae_noise(_ptr(noise), n, key, off & 0xFFFFFFFF, _stream()), "pm_mae_noise")
        _lib.check(lib.pm_drop_path_scales(_ptr(noise), _ptr(rates), _ptr(scales), depth, B, _stream()), "pm_drop_path_scales")
        return scales

    def forward(self, imgs: torch.Tensor, drop_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Probe head (add_probe_head): head(forward_features(imgs)), the encoder frozen and forward-only.  Plain nn.Linear head
        (the fine-tune recipe, main_finetune.py): front, block stack, pooling and head as one autograd node (_VitFinetuneFn).
        Stochastic depth (training mode, drop_path_rate > 0): a scale table is drawn per forward (_draw_drop_scales) and blocks
        whose rate is above 0 run with it; `drop_scales` (f32 [depth, 2, B] on the device: the scale of sample b in the attention /
        MLP branch of block i) replaces the draw, as `noise=` does for the MAE -- every block then runs with the caller's table.
        The table of the last training forward stays in `last_drop_scales`."""
        if isinstance(self.head, ProbeHead):
            if drop_scales is not None:
                raise _lib.PolypMaeError("drop_scales: the probe's encoder is frozen and forward-only; it never drops a path")
            return self.head(self.forward_features(imgs))
        if not isinstance(self.head, nn.Linear):
            raise _lib.PolypMaeError(f"models_vit.VisionTransformer: the head must be the probe head or a plain nn.Linear "
                                     f"(got {type(self.head).__name__})")
        rt = self._rt
        rt.ensure(imgs.device)
        assert imgs.shape[2] == self.patch_embed.img_size[0] and imgs.shape[3] == self.patch_embed.img_size[1]
        from . import ops  # registers torch.ops.polypmae.* on first use
        rt.drop_path = None
        if self.drop_path_active:
            if drop_scales is None:
                rt.drop_path = (self._draw_drop_scales(imgs.shape[0], imgs.device), [p > 0.0 for p in self.drop_path_rates])
            else:
                want = (len(self.drop_path_rates), 2, imgs.shape[0])
                if (tuple(drop_scales.shape) != want or drop_scales.dtype != torch.float32 or drop_scales.device != imgs.device
                        or not drop_scales.is_contiguous()):
                    raise _lib.PolypMaeError(f"drop_scales must be a contiguous f32 {list(want)} tensor on the images' device "
                                             f"(got {drop_scales.dtype} {list(drop_scales.shape)} on {drop_scales.device})")
                rt.drop_path = (drop_scales, None)
            self.last_drop_scales = rt.drop_path[0]
        elif drop_scales is not None:
            raise _lib.PolypMaeError("drop_scales: stochastic depth is active in training mode at drop_path_rate > 0 only")
        return torch.ops.polypmae.vit_finetune_forward(imgs, ops.register_runtime(rt), list(rt.flat.params))


class _VitFinetuneFn(torch.autograd.Function):
    """imgs -> logits of models_vit.VisionTransformer with its plain Linear head (models_vit.py:34-53), one node, modelled on
    models._VitClsFn.  global_pool: the dense block stack, then pm_pool_norm_fwd_train / pm_pool_norm_bwd (fc_norm of the mean of the
    patch rows).  cls token: pm_vit_head_fwd / _bwd without their Linear (W = NULL / dfeat) -- D <= 1024 there, and the cls-row top
    block under _VitClsFn's own condition.  The head, the pool and the loss run in f32 in every precision mode."""

    @staticmethod
    def forward(ctx, rt: _Runtime, imgs: torch.Tensor, names, *params):
        k, f, mod, g = rt.k, rt.flat, rt.module, rt.enc_geom
        lib = k.lib
        B = imgs.shape[0]
        L = mod.patch_embed.num_patches
        N, D = L + 1, g.dim
        pool = mod.global_pool
        norm = "fc_norm" if pool else "norm"
        needs = ctx.needs_input_grad[3:] if rt.grad_enabled else (False,) * len(params)
        need = _Needs(names, needs, rt.unused)
        training = any(needs)
        below = any(nd for n, nd in zip(names, needs) if not n.startswith(("head.", norm + ".")))   # anything under the final norm
        imgs = imgs.contiguous().float()
        cols, x0 = _EncoderFrontMixin.front_fwd(rt, imgs, None, L)
        ws = rt.get_ws(g, B, N, below)
        W, _ = rt.stack_weights("blocks.", g.depth)
        drop_scales, drop_blocks = rt.drop_path if rt.drop_path is not None else (None, None)   # (this forward's alone)
        rt.drop_path = None
        # the cls-row top block is off under stochastic depth: its compact launches have no scaled form
        cls_top = (not pool) and k.SPARSE_TOP and N > 1 and (B % 8 == 0 or not training) and drop_scales is None
        x = BlockStack(k, g).forward(ws, x0, W, before_block=_update_gate(rt, "blocks."), keep_from=need.keep_from(g.depth),
                                     cls_top=cls_top, drop_scales=drop_scales, drop_blocks=drop_blocks)
        Nh = 1 if ws.cls_top else N
        rt.wait_updates()
        dev, f32 = imgs.device, torch.float32
        C = mod.head.weight.shape[0]
        feat = torch.empty(B, D, dtype=f32, device=dev)
        mean, rstd = torch.empty(B, dtype=f32, device=dev), torch.empty(B, dtype=f32, device=dev)
        pooled = None
        gamma, beta = f.param_view(norm + ".weight"), f.param_view(norm + ".bias")
        if pool:
            pooled = torch.empty(B, D, dtype=f32, device=dev)
            nbytes = _lib.workspace_bytes("pm_pool_norm_workspace", B, N, D)
            scratch = torch.empty((nbytes + 3) // 4, dtype=f32, device=dev)
            _lib.check(lib.pm_pool_norm_fwd_train(_ptr(x), B, N, D, _ptr(gamma), _ptr(beta), rt.eps, _ptr(feat), _ptr(pooled), _ptr(mean),
                                                  _ptr(rstd), _ptr(scratch), scratch.numel() * 4, _stream()), "pm_pool_norm_fwd_train")
        else:
            _lib.check(lib.pm_vit_head_fwd(_ptr(x), Nh, 0, _ptr(gamma), _ptr(beta), None, None, _ptr(feat), None, _ptr(mean), _ptr(rstd),
                                           None, B, D, 0, rt.eps, _stream()), "pm_vit_head_fwd")
        logits = torch.empty(B, C, dtype=f32, device=dev)
        _lib.check(lib.pm_linear_head_fwd(_ptr(feat), B, D, C, _ptr(f.param_view("head.weight")), _ptr(f.param_view("head.bias")),
                                          _ptr(logits), _stream()), "pm_linear_head_fwd")
        if training:
            ctx.rt, ctx.names, ctx.ws = rt, names, ws
            ctx.drop = (drop_scales, drop_blocks)
            xs = x
            if not below:   # nothing under the final norm trains: keep what its backward reads, release the stack's buffers
                xs = None if pool else x.view(B, Nh, D)[:, 0].clone()
                rt.put_ws(g, ws)
                ctx.ws = None
                cols = x0 = None
            ctx.saved = (cols, x0, xs, feat, pooled, mean, rstd)
            ctx.dims = (B, L, N, D, C, pool, below, Nh if below else 1)
        else:
            rt.put_ws(g, ws)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        rt, names, ws = ctx.rt, ctx.names, ctx.ws
        k, f, mod, g = rt.k, rt.flat, rt.module, rt.enc_geom
        lib = k.lib
        cols, x0, x, feat, pooled, mean, rstd = ctx.saved
        B, L, N, D, C, pool, below, x_rows = ctx.dims
        drop_scales, drop_blocks = ctx.drop
        norm = "fc_norm" if pool else "norm"
        needs = list(ctx.needs_input_grad[3:])
        need = _Needs(names, needs, rt.unused)
        accumulate = _plan_grads(rt, names, needs)
        dev, f32 = dlogits.device, torch.float32
        dlogits = dlogits.contiguous().float()
        # the head: dW / dbias are ONE addition into what the flat gradient held (pm_probe_head_bwd)
        if need("head.weight") or need("head.bias"):
            if not accumulate and need("head.weight"):
                f.grad_view("head.weight").zero_()   # (a matrix: _plan_grads zeroed the vectors only)
            dW = f.grad_view("head.weight") if need("head.weight") else torch.zeros(C, D, dtype=f32, device=dev)
            db = f.grad_view("head.bias") if need("head.bias") else torch.zeros(C, dtype=f32, device=dev)
            _lib.check(lib.pm_probe_head_bwd(_ptr(dlogits), _ptr(feat), B, D, C, _ptr(dW), _ptr(db), _stream()), "pm_probe_head_bwd")
        trainable = need.blocks("blocks.", g.depth)
        front = need.front(True)
        below_head = front or any(trainable)
        dgamma = f.grad_view(norm + ".weight") if need(norm + ".weight") else None
        dbeta = f.grad_view(norm + ".bias") if need(norm + ".bias") else None
        if below_head or dgamma is not None or dbeta is not None:
            dfeat = torch.empty(B, D, dtype=f32, device=dev)
            _lib.check(lib.pm_linear_head_dfeat(_ptr(dlogits), _ptr(f.param_view("head.weight")), B, D, C, _ptr(dfeat), _stream()),
                       "pm_linear_head_dfeat")
            if below_head and ws.cls_top:   # the head's gradient on the B cls rows only: what the cls-row top block takes
                tc = BlockStack.top_compact(ws, g, k.act_dtype, dev)
                dx, dx_act = tc["dx"], tc["dx_act"]
            else:
                dx = ws.dx[0] if below_head else None
                dx_act = ws.dx_act[0] if below_head else None
            gamma = f.param_view(norm + ".weight")
            # stochastic depth on the top block: the block makes the act copy of its incoming gradient itself (scaled per sample)
            top_dropped = drop_scales is not None and (drop_blocks is None or drop_blocks[-1])
            dx_act_out = None if top_dropped else dx_act
            if pool:
                nbytes = _lib.workspace_bytes("pm_pool_norm_bwd_workspace", B, N, D)
                scratch = torch.empty((nbytes + 3) // 4, dtype=f32, device=dev)
                _lib.check(lib.pm_pool_norm_bwd(_ptr(dfeat), _ptr(pooled), _ptr(mean), _ptr(rstd), _ptr(gamma), B, N, D, _ptr(dx),
                                                _ptr(dx_act_out), k.act, _ptr(dgamma), _ptr(dbeta), _ptr(scratch), scratch.numel() * 4,
                                                _stream()), "pm_pool_norm_bwd")
            else:
                _lib.check(lib.pm_vit_head_bwd(None, _ptr(dfeat), _ptr(x), x_rows, 0, _ptr(gamma), None, None, None, _ptr(mean),
                                               _ptr(rstd), _ptr(dx), _ptr(dx_act_out), k.act, None, None, _ptr(dgamma), _ptr(dbeta), B, D, 0,
                                               _stream()), "pm_vit_head_bwd")
        sync = rt.grad_sync
        if below_head:
            W, G = rt.stack_weights("blocks.", g.depth)
            cb = (lambda i: sync.block_done("blocks.", i)) if sync is not None else None
            dx0, _ = BlockStack(k, g).backward(ws, x0, W, G, dx, dx_act, False, trainable, front, lambda n, i: accumulate, cb,
                                               defer_join=True, drop_scales=drop_scales, drop_blocks=drop_blocks)
            if front and dx0 is not None:
                _EncoderFrontMixin.front_bwd(rt, dx0, cols, None, B, L, accumulate, need, True)
            BlockStack.join_deferred(ws)
        if sync is not None:
            sync.backward_done()
        if ws is not None:
            rt.put_ws(g, ws)
        ctx.saved = None
        grads = [None if (accumulate or not need(n)) else f.grad_view(n) for n in names]
        return (None, None, None, *grads)


def vit_base_patch16(num_classes=1000, global_pool=False, **kwargs):
    return VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, num_classes=num_classes, global_pool=global_pool,
                             **kwargs)


def vit_large_patch16(num_classes=1000, global_pool=False, **kwargs):
    return VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, num_classes=num_classes, global_pool=global_pool,
                             **kwargs)


def vit_huge_patch14(num_classes=1000, global_pool=False, **kwargs):
    return VisionTransformer(patch_size=14, embed_dim=1280, depth=32, num_heads=16, num_classes=num_classes, global_pool=global_pool,
                             **kwargs)


def add_probe_head(model: VisionTransformer) -> VisionTransformer:
    """main_linprobe.py:242-249: model.head becomes Sequential(BatchNorm1d(D, affine=False, eps=1e-6), head); every parameter is
    frozen but head.1.weight / head.1.bias.  The two stay nn.Parameters of the model (the engine's flat storage covers them like
    any other), so parallel.GradSync's trainable-range plan and the checkpoint code see them without change."""
    if not isinstance(model.head, ProbeHead):
        model.head = ProbeHead(model.head)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.head.parameters():
        p.requires_grad_(True)
    return model


def interpolate_pos_embed(model: VisionTransformer, checkpoint_model: dict) -> None:
    """mae/util/pos_embed.py:77-96 at equal grid size: nothing to do.  Another grid size would need the bicubic resize of the
    table, which is not part of this package: refused."""
    pe = checkpoint_model.get("pos_embed")
    if pe is not None and tuple(pe.shape) != tuple(model.pos_embed.shape):
        raise _lib.PolypMaeError(f"the checkpoint's pos_embed {tuple(pe.shape)} does not fit the model's {tuple(model.pos_embed.shape)}: "
                                 "position-embedding interpolation for another input size is not supported")


def _load_pretrained(model: VisionTransformer, checkpoint_model: dict, head_std: float):
    """The `["model"]` dict of a main_pretrain checkpoint into `model`: head keys of another shape are dropped, the rest loads
    non-strictly (the MAE's decoder and mask token are unexpected keys), the missing keys must be exactly the head (and fc_norm with
    global_pool), head.weight gets trunc-normal std `head_std`.  Returns load_state_dict's result."""
    checkpoint_model = dict(checkpoint_model)
    own = model.state_dict()
    for k in ("head.weight", "head.bias"):
        if k in checkpoint_model and checkpoint_model[k].shape != own[k].shape:
            print(f"Removing key {k} from pretrained checkpoint")
            del checkpoint_model[k]
    interpolate_pos_embed(model, checkpoint_model)
    msg = model.load_state_dict(checkpoint_model, strict=False)
    want = {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if model.global_pool else set())
    assert set(msg.missing_keys) == want, f"missing keys {sorted(msg.missing_keys)}; expected {sorted(want)}"
    nn.init.trunc_normal_(model.head.weight, std=head_std)
    return msg


def load_pretrained_for_probe(model: VisionTransformer, checkpoint_model: dict):
    """main_linprobe.py:216-240, BEFORE add_probe_head: _load_pretrained with the head at std 0.01 (following MoCo v3)."""
    return _load_pretrained(model, checkpoint_model, 0.01)


def load_pretrained_for_finetune(model: VisionTransformer, checkpoint_model: dict):
    """main_finetune.py:255-279: _load_pretrained with the head at std 2e-5 ("manually initialize fc layer")."""
    return _load_pretrained(model, checkpoint_model, 2e-5)
