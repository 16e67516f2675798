"""Float64 restatements of the streaming "row" kernels (pm_layernorm.hip forward, pm_misc.hip, pm_mae.hip, pm_head.hip) and the
element-wise bounds of their outputs (not a test module).  Every reference takes the operands as the kernel sees them and runs in
plain torch on whichever device they live on.  tests/test_rowops_ref_cpu.py holds each bound to f32 emulations of the kernels (and
to wrong ones); the tests/test_gpu_*_edges.py files of these kernels hold the kernels to them.  u = 2^-24 throughout.

Three classes of output:

BIT-EXACT (torch.equal against torch's own f32 add or .to(dtype); NaN by NaN-ness): the kernel moves data, does one IEEE f32
operation per element, or one round-to-nearest-even conversion --
  im2col (zero padding included), pad_cast, unpad_add (both modes), assemble_tokens forward, demb of pm_assemble_tokens_bwd and
  pm_mae_unshuffle_bwd (three activation types), mae_unshuffle forward, gather_rows, scatter_rows_zero, cast, and masking's
  ids_shuffle / ids_restore / mask.

SUMS of n terms in f32, any order: |got - want| <= n u T, T the float64 sum of the absolute terms, what the output held before
counted as one more term (sum_bound) --
  dcls, dpos (n = B + 1: B additions into the prior value), dmask_token (n = masked positions + 1), head dW and dbias (n = B + 1:
  B - 1 additions, the product's rounding, the prior value), head dgamma (n = B + n_class + 4: in front of that, the n_class-term
  dot product behind every d feat and the three roundings of xhat; pooled: the saved xhat_mean is an operand, B + n_class + 1),
  head dbeta (n = B + n_class), patch_loss (n = PE + 3: difference, square, PE - 1 additions, the division; under norm_pix plus
  the target's own error, below) and the loss scalar (n = B L + 3, its terms patch_loss * mask, as given to pm_mae_loss_finish).
  It holds for the fixed-order reductions and the atomic fallbacks alike.

LAYERNORM-SHAPED (bounds from the rounding points, no safety factor): mean, rstd, y of pm_layernorm_fwd; the head's mean, rstd,
feat, xhat_mean, logits and dx; the norm_pix target inside patch_loss and dpred.  With a = mean_d |x_d|, var the float64 variance:
  e_mean  = D u a                          D - 1 additions and one division of terms of size |x_d|
  r_rstd  = (D/2 + 4) u + e_mean^2 / (2 (var + eps))
            the sum of squares carries (D + 2) u relative (subtract, square, add: all terms positive) + u for / D + u for + eps:
            half of that after the square root, + 2 u for rsqrtf itself; and a mean off by e shifts the variance by exactly e^2
            (the deviations from the true mean sum to zero), relative e^2 / (var + eps), half of it in rstd
  e_xhat  = |xhat| (r_rstd + 3 u) + rstd e_mean      x - mean (u, and the mean's error), * rstd (u, and its error)
  e_y     = |gamma| e_xhat + 2 u (|xhat gamma| + |beta|)     * gamma, + beta
16-bit stores add u_T |want| and, for fp16, the subnormal quantum 2^-24 (store_bound), as attention_ref.bound16 does.
The unbiased variant (ddof = 1: torch.var of the loss's norm_pix) shifts the variance by e^2 D / (D - 1) instead.
The head follows the same steps (head_fwd, head_bwd); its backward is fed the float64 mean / rstd rounded to f32, so their error
is part of the operands."""
import torch

from attention_ref import DTYPES, U, ratio, rel  # noqa: F401  (re-exported: the tests take them from here)

U32 = 2.0 ** -24
FP16_QUANTUM = 2.0 ** -24
LN_EPS = 1e-6


def sum_bound(n, T):
    return n * U32 * T


def store_bound(e, want, prec):
    """The bound of a value stored in the activation type: one more rounding of the f32 result."""
    if prec == "fp32":
        return e
    return e + U[prec] * want.abs() + (FP16_QUANTUM if prec == "fp16" else 0.0)


def equal_bits(got, want):
    """torch.equal with NaN == NaN (casts: NaN compares by NaN-ness only)."""
    g, w = got.float(), want.float()
    gn, wn = torch.isnan(g), torch.isnan(w)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(torch.where(gn, torch.zeros_like(g), g), torch.where(wn, torch.zeros_like(w), w))) \
        and bool(torch.equal(torch.signbit(g) | gn, torch.signbit(w) | wn))


# ------------------------------------------------------------------------------------------------ LayerNorm-shaped
def row_stats(x, eps=LN_EPS, ddof=0):
    """x [..., D] -> float64 mean, var, r = (var + eps)^-1/2, xhat and their bounds e_mean, e_r, e_xhat (keepdim)."""
    x = x.double()
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / (D - ddof)
    r = (var + eps) ** -0.5
    xhat = (x - mean) * r
    e_mean = D * U32 * x.abs().mean(-1, keepdim=True)
    rr = (D / 2 + 4) * U32 + e_mean ** 2 * (D / (D - ddof)) / (2 * (var + eps))
    return dict(mean=mean, var=var, rstd=r, xhat=xhat, e_mean=e_mean, r_rstd=rr, e_rstd=r * rr,
                e_xhat=xhat.abs() * (rr + 3 * U32) + r * e_mean)


def ln_fwd(x, gamma, beta, eps=LN_EPS):
    """pm_layernorm_fwd: x [M, D] (any row pitch: pass the strided view).  -> dict of float64 mean / rstd [M], y [M, D] and e_*."""
    s = row_stats(x, eps)
    g, b = gamma.double(), beta.double()
    y = s["xhat"] * g + b
    e_y = g.abs() * s["e_xhat"] + 2 * U32 * ((s["xhat"] * g).abs() + b.abs())
    return dict(mean=s["mean"][..., 0], rstd=s["rstd"][..., 0], y=y, e_mean=s["e_mean"][..., 0], e_rstd=s["e_rstd"][..., 0], e_y=e_y,
                xhat=s["xhat"], e_xhat=s["e_xhat"])


def ln_ratios(mean, rstd, y, ref, prec):
    return {"mean": ratio(mean, ref["mean"], ref["e_mean"]), "rstd": ratio(rstd, ref["rstd"], ref["e_rstd"]),
            "y": ratio(y, ref["y"], store_bound(ref["e_y"], ref["y"], prec))}


# ------------------------------------------------------------------------------------------------ token path
def im2col(imgs, p, ids_keep, ldcols, dtype):
    """pm_patch_im2col: imgs f32 [B, C, H, H] -> [B keep, ldcols] of `dtype`, element (c p + py) p + px of patch gy * grid + gx,
    columns past C p p zero."""
    B, C, H, _ = imgs.shape
    g = H // p
    cols = imgs.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * p * p)
    if ids_keep is not None:
        cols = torch.gather(cols, 1, ids_keep.long()[..., None].expand(-1, -1, C * p * p))
    out = torch.zeros(B * cols.shape[1], ldcols, dtype=dtype, device=imgs.device)
    out[:, :C * p * p] = cols.reshape(-1, C * p * p).to(dtype)
    return out


def assemble(emb, cls, pos, ids_keep, B, keep, D):
    """pm_assemble_tokens in torch's own f32 add: -> [B, 1 + keep, D]."""
    ids = ids_keep.long() if ids_keep is not None else torch.arange(keep, device=emb.device).expand(B, keep)
    x = torch.empty(B, keep + 1, D, dtype=torch.float32, device=emb.device)
    x[:, 0] = cls.reshape(D) + pos[0]
    x[:, 1:] = emb.reshape(B, keep, D) + pos[1:][ids]
    return x


def assemble_bwd(dx, ids_keep, B, keep, D, dcls0=None, dpos0=None):
    """pm_assemble_tokens_bwd: dx f32 [B, 1 + keep, D].  -> demb f32 [B keep, D] (exact: cast it), and float64 dcls / dpos with the
    sums of their absolute terms t_dcls / t_dpos (prior contents included); n = B + 1 for both."""
    dx64 = dx.double().reshape(B, keep + 1, D)
    ids = ids_keep.long() if ids_keep is not None else torch.arange(keep, device=dx.device).expand(B, keep)
    out = dict(demb=dx.reshape(B, keep + 1, D)[:, 1:].reshape(B * keep, D), n=B + 1)
    c0 = dcls0.double().reshape(D) if dcls0 is not None else torch.zeros(D, dtype=torch.float64, device=dx.device)
    out["dcls"], out["t_dcls"] = c0 + dx64[:, 0].sum(0), c0.abs() + dx64[:, 0].abs().sum(0)
    if dpos0 is not None:
        dpos, t = dpos0.double().clone(), dpos0.double().abs()
        idx = (1 + ids).reshape(-1)
        dpos.index_add_(0, idx, dx64[:, 1:].reshape(-1, D))
        t.index_add_(0, idx, dx64[:, 1:].reshape(-1, D).abs())
        dpos[0] += dx64[:, 0].sum(0)
        t[0] += dx64[:, 0].abs().sum(0)
        out["dpos"], out["t_dpos"] = dpos, t
    return out


# ------------------------------------------------------------------------------------------------ MAE
def masking(noise, len_keep):
    """pm_mae_masking: the stable ascending argsort (on the CPU: the reference of the test, not of the device)."""
    noise = noise.cpu()
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    mask = (ids_restore >= len_keep).float()
    return ids_shuffle.int(), ids_restore.int(), mask


def unshuffle(emb, mask_token, dpos, ids_restore, B, L, keep, D):
    """pm_mae_unshuffle in torch's own f32 add: emb [B, 1 + keep, D] -> [B, 1 + L, D]."""
    emb = emb.reshape(B, keep + 1, D)
    full = torch.cat([emb[:, 1:], mask_token.reshape(1, 1, D).expand(B, L - keep, D)], 1) if keep < L else emb[:, 1:]
    rows = torch.gather(full, 1, ids_restore.long()[..., None].expand(-1, -1, D))
    return torch.cat([emb[:, :1], rows], 1) + dpos.reshape(1, L + 1, D)


def unshuffle_bwd(dout, ids_shuffle, B, L, keep, D, dmask0):
    """pm_mae_unshuffle_bwd: -> demb f32 [B, 1 + keep, D] (exact), float64 dmask_token, its t_ and n = B (L - keep) + 1."""
    dout = dout.reshape(B, L + 1, D)
    rows = torch.gather(dout[:, 1:], 1, ids_shuffle.long()[..., None].expand(-1, -1, D))
    m = rows[:, keep:].double().reshape(-1, D)
    d0 = dmask0.double().reshape(D)
    return dict(demb=torch.cat([dout[:, :1], rows[:, :keep]], 1), dmask=d0 + m.sum(0), t_dmask=d0.abs() + m.abs().sum(0),
                n=B * (L - keep) + 1)


def patchify(imgs, p, order="nhwpqc"):
    """imgs [B, C, H, H] -> [B, L, p p C], element (py p + px) C + c ('nhwpqc', the loss's order)."""
    B, C, H, _ = imgs.shape
    g = H // p
    x = imgs.reshape(B, C, g, p, g, p)
    return torch.einsum("nchpwq->" + order, x).reshape(B, g * g, p * p * C)


def mae_loss(imgs, pred, mask, p, norm_pix, dloss=1.0, order="nhwpqc", ddof=1):
    """pm_mae_loss_fwd / _finish / _bwd.  pred [B, L, PE] (the patch rows, first PE columns), mask [B, L].  -> float64
      patch_loss [B, L] with e_patch; loss with e_loss (from the float64 patch_loss: chained errors are the caller's, see
      loss_finish); dpred [B, L, PE] with e_dpred (before the store)."""
    t = patchify(imgs.double(), p, order)
    PE = t.shape[-1]
    e_t = torch.zeros_like(t)
    if norm_pix:
        s = row_stats(t, 1e-6, ddof)
        t, e_t = s["xhat"], s["e_xhat"]
    d = pred.double() - t
    pl = (d * d).mean(-1)
    e_patch = sum_bound(PE + 3, pl) + 2 * (d.abs() * e_t).mean(-1)
    fin = loss_finish(pl, mask)
    g = dloss / fin["sum_mask"] * 2.0 / PE * mask.double()[..., None]
    dpred = g * d
    e_dpred = g.abs() * e_t + 6 * U32 * dpred.abs()   # the difference, * g, and g = dloss / sum * 2 / PE * mask: six roundings
    return dict(patch_loss=pl, e_patch=e_patch, loss=fin["loss"], e_loss=fin["e_loss"], dpred=dpred, e_dpred=e_dpred, target=t)


def loss_finish(patch_loss, mask):
    """pm_mae_loss_finish on the patch_loss it is given: loss = sum(pl mask) / sum(mask), n = B L + 3 (the products, the two sums --
    sum(mask) is a sum of ones and zeros, exact below 2^24 -- and the division)."""
    pl, m = patch_loss.double().reshape(-1), mask.double().reshape(-1)
    sm = m.sum()
    return dict(loss=(pl * m).sum() / sm, sum_mask=sm, e_loss=sum_bound(pl.numel() + 3, (pl * m).abs().sum() / sm))


# ------------------------------------------------------------------------------------------------ heads
def _dot_bound(a, e_a, w, bias):
    """sum_d a_d w_kd + bias_k over D terms: the error of a through |w|, (D + 2) u of the absolute terms."""
    D = a.shape[-1]
    val = a @ w.T + (bias if bias is not None else 0.0)
    e = e_a @ w.abs().T + (D + 2) * U32 * (a.abs() @ w.abs().T + (bias.abs() if bias is not None else 0.0))
    return val, e


def head_fwd(x, pool, gamma, beta, W, bias, eps=LN_EPS):
    """pm_vit_head_fwd: x [B, N, D].  -> float64 mean / rstd ([B] for pool 0, [B, N] with row 0 unwritten for pool 1), feat, logits,
    xhat_mean (pool 1) and e_*.  Pooled: xm = mean_n xhat_n over the N - 1 patch rows (N - 2 additions + the 1 / (N - 1) factor and
    its own rounding: (N + 1) u of the mean absolute term), feat = xm gamma + beta."""
    g, b = gamma.double(), beta.double()
    if pool == 0:
        s = row_stats(x[:, 0], eps)
        xm, e_xm = s["xhat"], s["e_xhat"]
        out = dict(mean=s["mean"][:, 0], rstd=s["rstd"][:, 0], e_mean=s["e_mean"][:, 0], e_rstd=s["e_rstd"][:, 0])
    else:
        N = x.shape[1]
        s = row_stats(x, eps)
        xm = s["xhat"][:, 1:].mean(1)
        e_xm = s["e_xhat"][:, 1:].mean(1) + (N + 1) * U32 * s["xhat"][:, 1:].abs().mean(1)
        out = dict(mean=s["mean"][..., 0], rstd=s["rstd"][..., 0], e_mean=s["e_mean"][..., 0], e_rstd=s["e_rstd"][..., 0],
                   xhat_mean=xm, e_xhat_mean=e_xm)
    out["feat"] = xm * g + b
    out["e_feat"] = g.abs() * e_xm + 2 * U32 * ((xm * g).abs() + b.abs())
    if W is not None:
        out["logits"], out["e_logits"] = _dot_bound(out["feat"], out["e_feat"], W.double(), bias.double() if bias is not None else None)
    return out


def head_bwd(dlogits, dfeat, x, pool, gamma, W, feat, xhat_mean, mean, rstd, prior=None):
    """pm_vit_head_bwd from its operands (mean / rstd / feat / xhat_mean f32 as given).  -> float64 dx [B, N, D] with e_dx, and the
    four sums with t_* and n_* (prior: dict of what dW / dbias / dgamma / dbeta held, default zeros).
    dx = rstd (gg - c1 - xhat c2), gg = g gamma (/ (N - 1) pooled), c1 = mean_d gg, c2 = mean_d gg xhat:
      e_g   = (n_class + 1) u sum_k |dlogits_k W_kd|   (0 when d feat is given)
      e_gg  = |gamma| e_g / (N - 1) + 3 u |gg|;   e_xh = 2 u |xhat|
      e_c1  = mean_d e_gg + (D + 1) u mean_d |gg|
      e_c2  = mean_d (e_gg |xhat| + |gg| e_xh + u |gg xhat|) + (D + 1) u mean_d |gg xhat|
      e_dx  = rstd (e_gg + e_c1 + e_xh |c2| + |xhat| e_c2 + 3 u (|gg| + |c1| + |xhat c2|)) + u |dx|"""
    B, N, D = x.shape
    gam = gamma.double()
    if dfeat is not None:
        g, ag, nk = dfeat.double(), dfeat.double().abs(), 0
        e_g = torch.zeros_like(g)
    else:
        nk = W.shape[0]
        g, ag = dlogits.double() @ W.double(), dlogits.double().abs() @ W.double().abs()
        e_g = (nk + 1) * U32 * ag
    x64 = x.double()
    if pool == 0:
        mu, rs = mean.double().reshape(B, 1, 1), rstd.double().reshape(B, 1, 1)
        rows, scale = x64[:, :1], 1.0
    else:
        mu, rs = mean.double().reshape(B, N, 1)[:, 1:], rstd.double().reshape(B, N, 1)[:, 1:]
        rows, scale = x64[:, 1:], 1.0 / (N - 1)
    xh = (rows - mu) * rs
    gg = (g * scale * gam)[:, None]
    e_gg = (gam.abs() * e_g * scale)[:, None] + 3 * U32 * gg.abs()
    e_xh = 2 * U32 * xh.abs()
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    e_c1 = e_gg.mean(-1, keepdim=True) + (D + 1) * U32 * gg.abs().mean(-1, keepdim=True)
    e_c2 = (e_gg * xh.abs() + gg.abs() * e_xh + U32 * (gg * xh).abs()).mean(-1, keepdim=True) + (D + 1) * U32 * (gg * xh).abs().mean(-1, keepdim=True)
    o = rs * (gg - c1 - xh * c2)
    e_o = rs * (e_gg + e_c1 + e_xh * c2.abs() + xh.abs() * e_c2 + 3 * U32 * (gg.abs() + c1.abs() + (xh * c2).abs())) + U32 * o.abs()
    dx, e_dx = torch.zeros_like(x64), torch.zeros_like(x64)
    if pool == 0:
        dx[:, :1], e_dx[:, :1] = o, e_o
    else:
        dx[:, 1:], e_dx[:, 1:] = o, e_o
    out = dict(dx=dx, e_dx=e_dx)
    prior = prior or {}
    p0 = lambda n, like: prior[n].double() if prior.get(n) is not None else torch.zeros_like(like)
    xa = xhat_mean.double() if pool == 1 else xh[:, 0]
    dg, db = (g * xa).sum(0), g.sum(0)
    out["dgamma"], out["t_dgamma"] = p0("dgamma", dg) + dg, p0("dgamma", dg).abs() + (ag * xa.abs()).sum(0)
    out["dbeta"], out["t_dbeta"] = p0("dbeta", db) + db, p0("dbeta", db).abs() + ag.sum(0)
    out["n_dgamma"], out["n_dbeta"] = B + nk + (1 if pool == 1 else 4), B + nk
    if dlogits is not None and feat is not None:
        dl, f = dlogits.double(), feat.double()
        dW, dbias = dl.T @ f, dl.sum(0)
        out["dW"], out["t_dW"] = p0("dW", dW) + dW, p0("dW", dW).abs() + dl.abs().T @ f.abs()
        out["dbias"], out["t_dbias"] = p0("dbias", dbias) + dbias, p0("dbias", dbias).abs() + dl.abs().sum(0)
        out["n_dW"] = out["n_dbias"] = B + 1
    return out
