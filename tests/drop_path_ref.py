"""Host restatement of stochastic depth (timm 0.4.12 DropPath as mae/main_finetune.py:251 switches it on) for the tests of
ssl4polyp_amd/csrc/pm_droppath.hip and models_vit.VisionTransformer(drop_path_rate=...).  TEST INFRASTRUCTURE ONLY.

  * the scale table: noise from oracle.noise_ref.mae_noise (Philox4x32-10, keyed by the device generator's seed and offset the way
    MaskedAutoencoderViT._draw_noise keys it), then timm's rule in f32: keep = 1 - p, a sample keeps a branch when
    fl32(keep + u) >= 1 (floor of a value in [keep, keep + 1)), and a kept branch is multiplied by fl32(1 / keep) (x.div(keep)
    by a Python scalar multiplies by the f32 reciprocal);
  * the float64 block x + s_attn * attn(LN x), then + s_mlp * mlp(LN .), composed from the oracle's attention / mlp / layer_norm, and
    the fine-tune model over it (tests/finetune_ref.py vit_finetune_logits with that block).

The model test's configuration lives here so that the CPU test can check, by construction, that its seed drops and keeps at
least one sample in every branch of every block above 0 -- the GPU test compares the device's table with this one exactly."""
import numpy as np
import torch

from oracle import noise_ref
from oracle import vit_mae_ref as O

MODEL = dict(embed_dim=64, depth=3, num_heads=2)   # TINY of tests/test_gpu_finetune_mae.py with a third block
MODEL_B, MODEL_C, MODEL_RATE = 8, 5, 0.5
MODEL_SEED = 5                                    # torch.manual_seed right before the forward: generator offset 0


def rates(rate: float, depth: int):
    """timm: dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]."""
    return [float(v) for v in torch.linspace(0, rate, depth)]


def draw_key(seed: int, offset: int):
    """(key, stream id) of pm_mae_noise for the device generator's (seed, offset): models.MaskedAutoencoderViT._draw_noise."""
    seed &= 0xFFFFFFFFFFFFFFFF
    return (seed ^ ((offset >> 32) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFF


def drawn(n: int) -> int:
    """What a draw of n numbers advances the generator's offset by."""
    return 4 * ((n + 3) // 4)


def scales_from_noise(noise: np.ndarray, drop_rates) -> np.ndarray:
    """noise f32 [depth, 2, B] -> scales f32 [depth, 2, B]."""
    noise = np.asarray(noise, dtype=np.float32)
    p = np.asarray(drop_rates, dtype=np.float32).reshape(-1, 1, 1)
    keep = (np.float32(1.0) - p).astype(np.float32)
    t = (keep + noise).astype(np.float32)
    inv = (np.float32(1.0) / keep).astype(np.float32)
    return np.where(t >= np.float32(1.0), np.broadcast_to(inv, noise.shape), np.float32(0.0)).astype(np.float32)


def scale_table(seed: int, offset: int, drop_rates, B: int) -> np.ndarray:
    """The table models_vit.VisionTransformer draws for a batch of B at generator state (seed, offset)."""
    depth = len(drop_rates)
    key, sid = draw_key(seed, offset)
    noise = noise_ref.mae_noise(depth * 2 * B, key, sid).reshape(depth, 2, B)
    return scales_from_noise(noise, drop_rates)


def arbitrary_table(depth: int, B: int) -> torch.Tensor:
    """Finite scales, distinct per sample, block and branch, a zero in every branch: what catches an index mix-up that a table of
    {0, c} can hide."""
    i = torch.arange(depth, dtype=torch.float32).view(depth, 1, 1)
    j = torch.arange(2, dtype=torch.float32).view(1, 2, 1)
    b = torch.arange(B, dtype=torch.float32).view(1, 1, B)
    t = 0.5 + 0.125 * b + 0.0625 * j + 0.015625 * i         # exact in f32, all different
    t[:, 0, 1] = 0.0
    t[:, 1, B - 2] = 0.0
    return t.contiguous()


def block(x, sd, pre: str, heads: int, s_attn, s_mlp):
    """timm Block.forward with a per-sample scale on each residual branch, in the dtype of x."""
    sa = s_attn.to(x.dtype).view(-1, 1, 1)
    sm = s_mlp.to(x.dtype).view(-1, 1, 1)
    x = x + sa * O.attention(O.layer_norm(x, sd, pre + "norm1."), sd, pre + "attn.", heads)
    return x + sm * O.mlp(O.layer_norm(x, sd, pre + "norm2."), sd, pre + "mlp.")


def vit_finetune_logits(sd, imgs, cfg, global_pool: bool, scales):
    """tests/finetune_ref.py vit_finetune_logits with `block` above; scales [depth, 2, B]."""
    w = sd["patch_embed.proj.weight"]
    x = O.patch_embed(imgs, w, sd["patch_embed.proj.bias"], cfg.patch_size)
    x = torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), x), dim=1) + sd["pos_embed"]
    for i in range(cfg.depth):
        x = block(x, sd, f"blocks.{i}.", cfg.num_heads, scales[i, 0], scales[i, 1])
    x = O.layer_norm(x[:, 1:].mean(1), sd, "fc_norm.") if global_pool else O.layer_norm(x, sd, "norm.")[:, 0]
    return torch.nn.functional.linear(x, sd["head.weight"], sd["head.bias"])
