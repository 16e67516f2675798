"""Float64 restatements of the fine-tune kernels (csrc/pm_finetune.hip) and the element-wise bounds of their outputs (not a test
module).  Built like tests/probe_ref.py, which it imports and does not edit: every reference takes the operands as the kernel sees
them (f32 tensors, the record's f32 lam and 1 - lam) and runs in plain torch float64; every bound is counted from the rounding points
of the kernel's arithmetic, u = 2^-24, no fitted factor.  tests/test_finetune_mae_cpu.py holds the bounds to f32 emulations and to
wrong variants; tests/test_gpu_finetune_mae.py holds the kernels to them.

Mixup: v = lam a + oml b from three roundings: u (|lam a| + |oml b|) + u |v|.  (On the device the kernel is held to torch's own
  three-op sequence bit for bit; the bound is what separates the record's f32(1 - lam) from an f32 subtraction 1.f - f32(lam).)
CutMix: data movement, exact.
Soft-target cross-entropy, per row with a_c = z_c - max z, S = sum_c exp(a_c), r_S = (max |a| + C + 3) u as in probe_ref.ce:
  t_c = lam v_c + oml w_c (v, w the two smoothed one-hot rows, f32 on / off as given): e_t = 3 u t_c (all terms >= 0);
  lse = max + log S: e_lse = r_S + 2 u |log S| + u |lse|;  d_c = lse - z_c >= 0: e_d = e_lse + u d_c;
  row = sum_c t_c d_c, C positive terms: sum_c (t_c e_d + d_c e_t + u t_c d_c) + (C + 1) u row;
  loss = mean of the rows: mean e_row + sum_bound(B + 1, mean row).
  dlogits = (p - t) g: g |p| ((|a_c| + 6) u + r_S) + g e_t + 5 u |dlogits|   (probe_ref.ce's chain with the target's own error).
Pool + fc_norm forward: probe_ref.pool_norm, plus the saved statistics: the mean moves by e_mean + mean_k d_k, rstd by rr relative.
Pool + fc_norm backward, from the f32 pooled / mean / rstd it is given: gg = dfeat gamma (u |gg|), xhat = (pooled - mean) rstd
  (2 u |xhat|), c1 = mean gg, c2 = mean gg xhat ((D + 1) u of the mean absolute term each, plus the terms' own errors),
  o = rstd (gg - c1 - xhat c2) / (N - 1): (e_gg + e_c1 + e_xh |c2| + |xhat| e_c2 + 3 u (|gg| + |c1| + |xhat c2|)) rstd / (N - 1)
  + 2 u |o|.  dx_act: rowops_ref.store_bound -- but the test holds it to the RNE rounding of dx exactly.
  dgamma: sum_bound(B + 3, T), dbeta: sum_bound(B + 1, T), the prior value one more term.
Linear head: rowops_ref._dot_bound.  dfeat = dlogits W: (C + 1) u |dlogits| |W|."""
import torch

import probe_ref as P
import rowops_ref as R
from rowops_ref import U32, ratio, store_bound, sum_bound  # noqa: F401


def f32(v: float) -> float:
    """A Python double rounded to f32 (what torch does to a Python scalar that meets an f32 tensor)."""
    return float(torch.tensor(v, dtype=torch.float64).float())


def record(lam: float):
    """(f32(lam), f32(1 - lam)): the record's two weights, both rounded from the host's doubles."""
    return f32(lam), f32(1.0 - lam)


# ------------------------------------------------------------------------------------------------ mixing
def mixup(x, lam32: float, oml32: float):
    """x [B, ...] -> (float64 lam x + oml x.flip(0), bound)."""
    a, b = x.double(), x.double().flip(0)
    v = lam32 * a + oml32 * b
    return v, U32 * ((lam32 * a).abs() + (oml32 * b).abs()) + U32 * v.abs()


def mixup_f32(x, lam32: float, oml32: float):
    """torch's three-op sequence in f32 (the kernel's arithmetic)."""
    x = x.clone().float()
    flipped = x.flip(0).mul_(oml32)
    return x.mul_(lam32).add_(flipped)


def cutmix(x, box):
    """x [B, C, H, W]: inside [yl:yh, xl:xh] the pair swaps its old values."""
    yl, yh, xl, xh = box
    out = x.clone()
    out[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    return out


# ------------------------------------------------------------------------------------------------ soft-target cross-entropy
def on_off(smoothing: float, C: int):
    off = smoothing / C
    return f32(1.0 - smoothing + off), f32(off)


def soft_targets(target, C: int, lam32: float, oml32: float, smoothing: float):
    """float64 [B, C]: lam onehot(y; on, off) + oml onehot(y.flip(0); on, off), on / off as f32 values."""
    on, off = on_off(smoothing, C)
    t = target.long()
    y1 = torch.full((t.numel(), C), off, dtype=torch.float64, device=t.device).scatter_(1, t[:, None], on)
    y2 = torch.full((t.numel(), C), off, dtype=torch.float64, device=t.device).scatter_(1, t.flip(0)[:, None], on)
    return lam32 * y1 + oml32 * y2


def soft_ce(logits, target, lam32=1.0, oml32=0.0, smoothing=0.0, scale=1.0, targets=None):
    """-> float64 loss, row_loss, dlogits and e_loss, e_dlogits.  targets: a [B, C] float64 target matrix to use instead (the wrong
    variants of the CPU test)."""
    z = logits.double()
    B, C = z.shape
    t = soft_targets(target, C, lam32, oml32, smoothing) if targets is None else targets
    e_t = 3 * U32 * t
    m = z.max(1, keepdim=True).values
    a = z - m
    S = a.exp().sum(1, keepdim=True)
    lse = m + S.log()
    r_S = (a.abs().max(1, keepdim=True).values + C + 3) * U32
    e_lse = r_S + 2 * U32 * S.log().abs() + U32 * lse.abs()
    d = lse - z
    e_d = e_lse + U32 * d
    row = (t * d).sum(1)
    e_row = (t * e_d + d * e_t + U32 * t * d).sum(1) + (C + 1) * U32 * row
    loss = row.mean()
    e_loss = e_row.mean() + sum_bound(B + 1, row.abs().mean())
    p = a.exp() / S
    g = float(scale) / B
    dl = (p - t) * g
    e_dl = abs(g) * (p * ((a.abs() + 6) * U32 + r_S) + e_t) + 5 * U32 * dl.abs()
    return dict(loss=loss, row_loss=row, dlogits=dl, e_loss=e_loss, e_dlogits=e_dl)


def soft_ce_f32(logits, t32, scale=1.0):
    """The kernel's arithmetic in f32 from an f32 target matrix -> (loss, dlogits)."""
    z = logits.float()
    B = z.shape[0]
    m = z.max(1, keepdim=True).values
    e = (z - m).exp()
    S = e.sum(1, keepdim=True)
    lse = m + S.log()
    row = (t32 * (lse - z)).sum(1)
    g = torch.tensor(scale, dtype=torch.float32) / B
    return row.sum() / B, (e * (1.0 / S) - t32) * g


# ------------------------------------------------------------------------------------------------ pool + fc_norm
def pool_fwd(x, gamma, beta, eps=R.LN_EPS):
    """probe_ref.pool_norm plus the statistics the training forward saves: mean / rstd [B] and e_mean, e_rstd."""
    out = P.pool_norm(x, gamma, beta, eps)
    D = x.shape[2]
    s = R.row_stats(out["pooled"], eps)
    d = out["e_pooled"]
    dm = d.mean(-1, keepdim=True)
    dev = (out["pooled"] - s["mean"]).abs()
    dvar = 2.0 / D * (dev * (d + dm)).sum(-1, keepdim=True) + (d.max(-1, keepdim=True).values + dm) ** 2
    rr = s["r_rstd"] + dvar / (2 * (s["var"] + eps))
    out.update(mean=s["mean"][:, 0], rstd=s["rstd"][:, 0], e_mean=(s["e_mean"] + dm)[:, 0], e_rstd=(s["rstd"] * rr)[:, 0])
    return out


def pool_bwd(dfeat, pooled, mean, rstd, gamma, N, prior=None, den=None, cls_row=False):
    """pm_pool_norm_bwd from its f32 operands -> float64 dx [B, N, D] with e_dx, dgamma / dbeta with t_* and n_*.
    den (default N - 1) and cls_row (default: row 0 is zero) exist for the wrong variants of the CPU test."""
    df, p, gam = dfeat.double(), pooled.double(), gamma.double()
    B, D = df.shape
    mu, rs = mean.double().reshape(B, 1), rstd.double().reshape(B, 1)
    den = float(N - 1 if den is None else den)
    gg = df * gam
    xh = (p - mu) * rs
    e_gg, e_xh = U32 * gg.abs(), 2 * U32 * xh.abs()
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    e_c1 = e_gg.mean(-1, keepdim=True) + (D + 1) * U32 * gg.abs().mean(-1, keepdim=True)
    e_c2 = (e_gg * xh.abs() + gg.abs() * e_xh + U32 * (gg * xh).abs()).mean(-1, keepdim=True) \
        + (D + 1) * U32 * (gg * xh).abs().mean(-1, keepdim=True)
    o = rs * (gg - c1 - xh * c2) / den
    e_o = rs / den * (e_gg + e_c1 + e_xh * c2.abs() + xh.abs() * e_c2 + 3 * U32 * (gg.abs() + c1.abs() + (xh * c2).abs())) + 2 * U32 * o.abs()
    dx = o[:, None].expand(B, N, D).clone()
    e_dx = e_o[:, None].expand(B, N, D).clone()
    if not cls_row:
        dx[:, 0] = 0.0
        e_dx[:, 0] = 0.0
    prior = prior or {}
    p0 = lambda n, like: prior[n].double() if prior.get(n) is not None else torch.zeros_like(like)
    dg, db = (df * xh).sum(0), df.sum(0)
    return dict(dx=dx, e_dx=e_dx, row=o, dgamma=p0("dgamma", dg) + dg, t_dgamma=p0("dgamma", dg).abs() + (df * xh).abs().sum(0),
                dbeta=p0("dbeta", db) + db, t_dbeta=p0("dbeta", db).abs() + df.abs().sum(0), n_dgamma=B + 3, n_dbeta=B + 1)


def pool_bwd_f32(dfeat, pooled, mean, rstd, gamma, N):
    """The kernel's arithmetic in f32 -> the row [B, D] every patch row of dx holds."""
    df, p, g = dfeat.float(), pooled.float(), gamma.float()
    B, D = df.shape
    mu, rs = mean.float().reshape(B, 1), rstd.float().reshape(B, 1)
    gg, xh = df * g, (p - mu) * rs
    c1 = gg.sum(-1, keepdim=True) / D
    c2 = (gg * xh).sum(-1, keepdim=True) / D
    return rs * (gg - c1 - xh * c2) / float(N - 1)


# ------------------------------------------------------------------------------------------------ the plain Linear head
def linear(feat, W, bias):
    """-> (float64 logits, bound): exact operands, D products and additions."""
    return R._dot_bound(feat.double(), torch.zeros_like(feat, dtype=torch.float64), W.double(), bias.double())


def dfeat(dlogits, W):
    dl, w = dlogits.double(), W.double()
    C = w.shape[0]
    return dl @ w, (C + 1) * U32 * (dl.abs() @ w.abs())


# ------------------------------------------------------------------------------------------------ the model
def vit_finetune_logits(sd, imgs, cfg, global_pool: bool):
    """mae/models_vit.py:34-53 on a state dict with its key names, composed from the oracle's patch_embed / block, in the dtype of
    `sd` (the tests pass float64): cls token + learned pos_embed, the blocks, then fc_norm(x[:, 1:].mean(1)) (global_pool) or
    norm(x)[:, 0], then head.  The patch embedding runs where its weight lives, everything behind it where cls_token lives (the
    ViT-B case keeps the convolution on the host and the float64 blocks on the device)."""
    from oracle import vit_mae_ref as O
    w = sd["patch_embed.proj.weight"]
    x = O.patch_embed(imgs.to(w.device), w, sd["patch_embed.proj.bias"], cfg.patch_size).to(sd["cls_token"].device)
    x = torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), x), dim=1) + sd["pos_embed"]
    for i in range(cfg.depth):
        x = O.block(x, sd, f"blocks.{i}.", cfg.num_heads)
    if global_pool:
        x = O.layer_norm(x[:, 1:].mean(1), sd, "fc_norm.")
    else:
        x = O.layer_norm(x, sd, "norm.")[:, 0]
    return torch.nn.functional.linear(x, sd["head.weight"], sd["head.bias"])


def soft_ce_autograd(logits, target, lam32=1.0, oml32=0.0, smoothing=0.0):
    """timm SoftTargetCrossEntropy over soft_targets, differentiable, in the dtype of `logits`."""
    t = soft_targets(target, logits.shape[1], lam32, oml32, smoothing).to(logits.dtype)
    return torch.sum(-t * torch.nn.functional.log_softmax(logits, dim=-1), dim=-1).mean()
