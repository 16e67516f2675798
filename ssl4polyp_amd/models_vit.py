"""The ViT of the MAE linear-probe / fine-tune entry points (mae/models_vit.py) on the encoder runtime of this package, and what
mae/main_linprobe.py does to it: the BatchNorm + Linear probe head and the loading of a pre-training checkpoint.

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
from .engine import BlockStack, StackGeom
from .models import (_DEFAULT_PRECISION, Block, PatchEmbed, _ClassifierBase, _EncoderFrontMixin, _Runtime, _update_gate)
from .probe import ProbeHead, pool_norm


class VisionTransformer(_ClassifierBase):
    """mae/models_vit.py:20-53 (timm 0.4.12 VisionTransformer + global_pool), same seeded initialisation order as
    models.VisionTransformer_from_Any.  forward(imgs) = head(forward_features(imgs)); the head must be the probe head
    (add_probe_head): the plain Linear of the fine-tune recipe has no kernel here and is refused."""

    def __init__(self, img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_classes=1000, global_pool=False,
                 precision: Optional[str] = None):
        super().__init__()
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
        """f32 [B, D], detached: norm(x)[:, 0], or fc_norm(x[:, 1:].mean(1)) with global_pool."""
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
        """f32 [B, N, D]: the output of the last block, before any final norm (a copy: the workspace goes back to the pool)."""
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

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        if not isinstance(self.head, ProbeHead):
            raise _lib.PolypMaeError("models_vit.VisionTransformer runs with the linear-probe head only: call add_probe_head(model) "
                                     "first (the fine-tune recipe's plain Linear head is not built)")
        return self.head(self.forward_features(imgs))


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


def load_pretrained_for_probe(model: VisionTransformer, checkpoint_model: dict):
    """main_linprobe.py:216-240 on the `["model"]` dict of a main_pretrain checkpoint, BEFORE add_probe_head: head keys of another
    shape are dropped, the rest loads non-strictly (the MAE's decoder and mask token are unexpected keys), the missing keys must be
    exactly the head (and fc_norm with global_pool), head.weight gets trunc-normal std 0.01.  Returns load_state_dict's result."""
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
    nn.init.trunc_normal_(model.head.weight, std=0.01)   # following MoCo v3
    return msg
