"""The bounds of tests/rowops_ref.py are honest (CPU): f32 emulations of the row kernels -- in the kernel's own summation order and
strictly sequential -- stay within every bound at every case the GPU tests use (tests/rowops_cases.py), and the listed wrong
variants exceed one, or differ in bits, on at least one of them.  The cast test's tie table is checked against integer arithmetic and
numpy here, so the GPU test is not its own oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_cases as C
import rowops_ref as R

LANES = torch.arange(64)
f32 = torch.float32


# ---- summation orders ---------------------------------------------------------------------------
def seqsum(t, dim=-1):
    t = t.movedim(dim, -1)
    s = torch.zeros(t.shape[:-1], dtype=f32)
    for j in range(t.shape[-1]):
        s = s + t[..., j]
    return s


def butterfly(p):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 over the last dim of 64."""
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[..., LANES ^ o]
    return p[..., 0]


def pad_to(t, n):
    return F.pad(t, (0, n - t.shape[-1]))


def wave_vec_sum(t, quad):
    """One wave over a row held as f32x4 slots (lane + 64 i): each lane adds its slots in order -- a slot as (v0 + v1) + (v2 + v3)
    (quad) or element by element -- then the butterfly.  Zero padding adds exact zeros."""
    nv = (t.shape[-1] + 255) // 256
    tp = pad_to(t, nv * 256).reshape(*t.shape[:-1], nv, 64, 4)
    if quad:
        lane = seqsum((tp[..., 0] + tp[..., 1]) + (tp[..., 2] + tp[..., 3]), dim=-2)
    else:
        lane = seqsum(tp.transpose(-2, -3).reshape(*t.shape[:-1], 64, nv * 4))
    return butterfly(lane)


def block_thread_sum(t):
    """256 threads own columns tid, tid + 256, ...; wave butterflies; (w0 + w1) + (w2 + w3)."""
    J = (t.shape[-1] + 255) // 256
    th = seqsum(pad_to(t, J * 256).reshape(*t.shape[:-1], J, 256), dim=-2)
    w = butterfly(th.reshape(*t.shape[:-1], 4, 64))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def split_sum(terms, acc, order, variant=None):
    """cls_grad_kernel (acc = 4) / head_pgrad_kernel (acc = 2) over terms [B, ...]: wave w takes samples w, w + 4, ... with `acc`
    accumulators in the unrolled body and a scalar tail into accumulator 0; waves combined as (p0 + p1) + (p2 + p3)."""
    B = terms.shape[0]
    if order == "seq":
        return seqsum(terms, dim=0)
    parts = []
    for w in range(4):
        a = [torch.zeros(terms.shape[1:], dtype=f32) for _ in range(acc)]
        b = w
        while b + 4 * (acc - 1) < B:
            for k in range(acc):
                a[k] = a[k] + terms[b + 4 * k]
            b += 4 * acc
        while b < B and variant != "no_tail":
            a[0] = a[0] + terms[b]
            b += 4
        parts.append(a[0] if variant == "acc0" else ((a[0] + a[1]) + (a[2] + a[3]) if acc == 4 else a[0] + a[1]))
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


ORDERS = ("kernel", "seq")


# ---- LayerNorm forward --------------------------------------------------------------------------
def emu_stats(x, eps, order, variant=None, ddof=0):
    """mean, rstd of the rows of x as the kernels compute them (two-pass, f32)."""
    D = x.shape[-1]
    xs = x
    if variant == "drop_ragged":   # the statistics miss the ragged last slot
        xs = x[..., :(D // 256) * 256]
    rowsum = (lambda t, quad: wave_vec_sum(t, quad)) if order == "kernel" else (lambda t, quad: seqsum(t))
    mean = rowsum(xs, True) / torch.tensor(float(D), dtype=f32)
    div = torch.tensor(float(D - 1 if variant == "dm1" else D - ddof), dtype=f32)
    if variant == "one_pass":
        var = rowsum(xs * xs, False) / div - mean * mean
    else:
        d = xs - mean[..., None]
        var = rowsum(d * d, False) / div
    e = {"no_eps": 0.0, "eps1e-5": 1e-5}.get(variant, eps)
    return mean, torch.rsqrt(var + torch.tensor(e, dtype=f32))


def emu_ln(x, gamma, beta, order, variant=None):
    mean, rstd = emu_stats(x, R.LN_EPS, order, variant)
    return mean, rstd, (x - mean[:, None]) * rstd[:, None] * gamma + beta


def ln_worst(M, D, regime, order, variant=None):
    x = C.rows(M, D, regime)
    gamma, beta = C.affine(D)
    ref = R.ln_fwd(x, gamma, beta)
    mean, rstd, y = emu_ln(x, gamma, beta, order, variant)
    worst = {}
    for prec in C.PRECS:
        for k, v in R.ln_ratios(mean, rstd, y.to(R.DTYPES[prec]), ref, prec).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("order", ORDERS)
def test_layernorm_bound_holds(order):
    worst = {}
    for M, D, regime in C.LN_CASES + [(C.LN_GRID[0], C.LN_GRID[1], "random")] + [(5, D, r) for D in (32, 68, 768, 1280) for r in C.REGIMES]:
        for k, v in ln_worst(M, D, regime, order).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"layernorm fwd emulation ({order}): largest err/bound {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("variant,cases", [
    ("dm1", [(37, 768, "random"), (37, 68, "offset64"), (37, 68, "huge")]),
    ("one_pass", [(37, 768, "offset64"), (37, 68, "offset64")]),
    ("no_eps", [(37, 768, "const"), (37, 768, "tiny")]),
    ("eps1e-5", [(37, 768, "const"), (37, 768, "tiny")]),
    ("drop_ragged", [(5, 260, "random"), (5, 1028, "random")])])
def test_layernorm_wrong_variants_exceed(variant, cases):
    for M, D, regime in cases:
        assert (M, D, regime) in C.LN_CASES
        w = ln_worst(M, D, regime, "kernel", variant)
        print(f"layernorm {variant} at {(M, D, regime)}: {w}")
        assert max(w.values()) > 1.0 or not np.isfinite(max(w.values())), (variant, M, D, regime, w)


# ---- sums: dcls, dpos, dmask_token --------------------------------------------------------------
def _dx(B, keep, D, seed=31):
    return C.randn(B, keep + 1, D, seed=seed)


@pytest.mark.parametrize("order", ORDERS)
def test_cls_grad_bound_holds(order):
    worst = 0.0
    for B in C.CLS_B:
        for D in C.CLS_D:
            dx, prior = _dx(B, 2, D), C.randn(D, seed=32, scale=3.0)
            ref = R.assemble_bwd(dx, None, B, 2, D, dcls0=prior)
            got = prior + split_sum(dx[:, 0], 4, order)
            worst = max(worst, R.ratio(got, ref["dcls"], R.sum_bound(ref["n"], ref["t_dcls"])))
    print(f"dcls emulation ({order}): largest err/bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("variant", ["no_tail", "acc0"])
def test_cls_grad_wrong_variants_exceed(variant):
    worst = 0.0
    for B in C.CLS_B:
        dx = _dx(B, 2, 68)
        ref = R.assemble_bwd(dx, None, B, 2, 68)
        worst = max(worst, R.ratio(split_sum(dx[:, 0], 4, "kernel", variant), ref["dcls"], R.sum_bound(ref["n"], ref["t_dcls"])))
    assert worst > 1.0


def _dpos_case():
    B, keep, L, D = 6, 5, 8, 68
    ids = torch.stack([torch.randperm(L, generator=C.gen(40 + b))[:keep] for b in range(B)]).int()   # every id drawn by several samples
    return B, keep, L, D, ids, _dx(B, keep, D, seed=41), C.randn(L + 1, D, seed=42)


@pytest.mark.parametrize("variant", [None, "reverse", "overwrite"])
def test_dpos_bound(variant):
    B, keep, L, D, ids, dx, prior = _dpos_case()
    ref = R.assemble_bwd(dx, ids, B, keep, D, dpos0=prior)
    got = prior.clone()
    order = [(b, j) for b in range(B) for j in range(keep)]
    for b, j in (reversed(order) if variant == "reverse" else order):
        row = 1 + int(ids[b, j])
        got[row] = dx[b, 1 + j] if variant == "overwrite" else got[row] + dx[b, 1 + j]
    got[0] = got[0] + split_sum(dx[:, 0], 4, "kernel")
    r = R.ratio(got, ref["dpos"], R.sum_bound(ref["n"], ref["t_dpos"]))
    print(f"dpos emulation ({variant}): err/bound {r:.3f}")
    assert (r > 1.0) if variant == "overwrite" else (r <= 1.0)


@pytest.mark.parametrize("order", ORDERS)
def test_dmask_token_bound_holds(order):
    B, L, keep, D = 5, 64, 16, 68
    dout, prior = C.randn(B, L + 1, D, seed=43), C.randn(D, seed=44)
    ids = torch.stack([torch.randperm(L, generator=C.gen(45 + b)) for b in range(B)]).int()
    ref = R.unshuffle_bwd(dout, ids, B, L, keep, D, prior)
    rows = torch.gather(dout[:, 1:], 1, ids.long()[..., None].expand(-1, -1, D))[:, keep:].reshape(-1, D)
    if order == "kernel":   # one block row: four waves take every fourth position, (w0 + w1) + (w2 + w3)
        part = torch.stack([seqsum(rows[i::4], dim=0) for i in range(4)])
        got = prior + ((part[0] + part[1]) + (part[2] + part[3]))
    else:
        got = prior + seqsum(rows, dim=0)
    r = R.ratio(got, ref["dmask"], R.sum_bound(ref["n"], ref["t_dmask"]))
    print(f"dmask_token emulation ({order}): err/bound {r:.3f}")
    assert r <= 1.0


# ---- MAE loss -----------------------------------------------------------------------------------
def emu_loss(imgs, pred, mask, p, norm_pix, order, dloss=1.0, variant=None):
    t = R.patchify(imgs, p, "nchpwq" if variant == "nchpwq" else "nhwpqc")
    PE = t.shape[-1]
    rowsum = (lambda v: wave_vec_sum(v, False)) if order == "kernel" else seqsum
    if norm_pix:
        mean = rowsum(t) / torch.tensor(float(PE), dtype=f32)
        d = t - mean[..., None]
        var = rowsum(d * d) / torch.tensor(float(PE if variant == "biased" else PE - 1), dtype=f32)
        t = d * (1.0 / torch.sqrt(var + torch.tensor(1e-6, dtype=f32)))[..., None]
    d = pred - t
    pl = rowsum(d * d) / torch.tensor(float(PE), dtype=f32)
    flat_pl, flat_m = pl.reshape(-1), mask.reshape(-1)
    if order == "kernel":   # 1024 threads stride the patches, 16 wave butterflies, the 16 partials in order
        n = (flat_pl.numel() + 1023) // 1024 * 1024
        strided = lambda v: seqsum(butterfly(seqsum(pad_to(v, n).reshape(-1, 1024), dim=0).reshape(16, 64)))
    else:
        strided = seqsum
    sa, sm = strided(flat_pl * flat_m), strided(flat_m)
    g0 = torch.tensor(dloss, dtype=f32) / sm * 2.0 / torch.tensor(float(PE), dtype=f32)
    return pl, sa / sm, (g0 * mask)[..., None] * d


def loss_worst(img, p, Cc, norm_pix, order, variant=None, B=2):
    imgs, pred, masks = C.loss_inputs(B, img, p, Cc)
    worst = {}
    for mname, mask in masks.items():
        ref = R.mae_loss(imgs, pred, mask, p, norm_pix, dloss=0.37)
        pl, loss, dpred = emu_loss(imgs, pred, mask, p, norm_pix, order, 0.37, variant)
        fin = R.loss_finish(pl, mask)   # the scalar against the patch losses it was given
        r = {"patch_loss": R.ratio(pl, ref["patch_loss"], ref["e_patch"]), "loss": R.ratio(loss, fin["loss"], fin["e_loss"])}
        for prec in C.PRECS:
            r["dpred " + prec] = R.ratio(dpred.to(R.DTYPES[prec]), ref["dpred"], R.store_bound(ref["e_dpred"], ref["dpred"], prec))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("norm_pix", [0, 1])
def test_loss_bound_holds(order, norm_pix):
    worst = {}
    for img, p, Cc in C.LOSS:
        for k, v in loss_worst(img, p, Cc, norm_pix, order).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"loss emulation ({order}, norm_pix {norm_pix}): largest err/bound {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("variant", ["biased", "nchpwq"])
def test_loss_wrong_variants_exceed(variant):
    w = loss_worst(32, 16, 3, 1, "kernel", variant)
    print(f"loss {variant}: {w}")
    assert w["patch_loss"] > 1.0 and w["dpred fp32"] > 1.0


def test_loss_reference_matches_oracle():
    """The float64 'nhwpqc' reference against the project's CPU oracle of the reference model's forward_loss."""
    from oracle import vit_mae_ref as O
    imgs, pred, masks = C.loss_inputs(2, 32, 16, 3)
    cfg = O.ViTConfig(img_size=32, patch_size=16)
    for norm_pix in (False, True):
        want = O.mae_loss(imgs.double(), pred.double(), masks["random"].double(), cfg, norm_pix)
        got = R.mae_loss(imgs, pred, masks["random"], 16, int(norm_pix))["loss"]
        assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


# ---- heads --------------------------------------------------------------------------------------
def emu_head(case, order, variant=None):
    """f32 emulation of pm_vit_head_fwd and, on the float64 mean / rstd / feat / xhat_mean rounded to f32, pm_vit_head_bwd.
    -> the worst err / bound per output."""
    B, N, D, pool, nk, has_bias, head, regime = case
    x, gamma, beta, W, bias, dlogits, dfeat = C.head_inputs(B, N, D, nk, regime)
    bias = bias if has_bias else None
    ref = R.head_fwd(x, pool, gamma, beta, W if head else None, bias)
    kern = order == "kernel"
    if pool == 0:
        mean, rstd = emu_stats(x[:, 0], R.LN_EPS, order)
        xm = (x[:, 0] - mean[:, None]) * rstd[:, None]
    else:
        mean, rstd = emu_stats(x, R.LN_EPS, order)
        xh = (x - mean[..., None]) * rstd[..., None]
        if kern:
            red = [seqsum(xh[:, 1 + w::4], dim=1) for w in range(4)]
            tot = (red[0] + red[1]) + (red[2] + red[3])
        else:
            tot = seqsum(xh[:, 1:], dim=1)
        xm = tot * torch.tensor(1.0 / ((N if variant == "divN" else N - 1)), dtype=f32)
    feat = xm * gamma + beta
    r = {"mean": R.ratio(mean, ref["mean"] if pool == 0 else ref["mean"], ref["e_mean"]), "rstd": R.ratio(rstd, ref["rstd"], ref["e_rstd"]),
         "feat": R.ratio(feat, ref["feat"], ref["e_feat"])}
    if head:
        prod = feat[:, None, :] * W[None]
        dot = (wave_vec_sum(prod, False) if pool == 0 else block_thread_sum(prod)) if kern else seqsum(prod)
        r["logits"] = R.ratio(dot + (bias if bias is not None else 0.0), ref["logits"], ref["e_logits"])
    # backward on reference-made statistics
    mean_in, rstd_in, feat_in = ref["mean"].float(), ref["rstd"].float(), ref["feat"].float()
    xhm_in = ref["xhat_mean"].float() if pool == 1 else None
    dl, df = (dlogits, None) if head else (None, dfeat)
    prior = {n: C.randn(*s, seed=50 + i) for i, (n, s) in enumerate((("dW", (nk, D)), ("dbias", (nk,)), ("dgamma", (D,)), ("dbeta", (D,))))}
    bref = R.head_bwd(dl, df, x, pool, gamma, W if head else None, feat_in if head else None, xhm_in, mean_in, rstd_in, prior)
    g = df if df is not None else seqsum(dl[:, :, None] * W[None], dim=1)
    if pool == 0:
        xh_in = (x[:, 0] - mean_in[:, None]) * rstd_in[:, None]
        gg = g * gamma
        red = block_thread_sum if kern else seqsum
        c1, c2 = red(gg) / torch.tensor(float(D), dtype=f32), red(gg * xh_in) / torch.tensor(float(D), dtype=f32)
        o = rstd_in[:, None] * (gg - c1[:, None] - xh_in * c2[:, None])
        dx = torch.zeros(B, N, D)
        dx[:, 0] = o
        xa = xh_in
    else:
        xh_in = (x - mean_in[..., None]) * rstd_in[..., None]
        gg = g * torch.tensor(1.0 / (N - 1), dtype=f32) * gamma
        c1 = (block_thread_sum(gg) if kern else seqsum(gg)) / torch.tensor(float(D), dtype=f32)
        t2 = gg[:, None] * xh_in
        c2 = (wave_vec_sum(t2, False) if kern else seqsum(t2)) / torch.tensor(float(D), dtype=f32)
        dx = rstd_in[..., None] * (gg[:, None] - c1[:, None, None] - xh_in * c2[..., None])
        dx[:, 0] = 0.0
        xa = xhm_in
    for prec in C.PRECS:
        r["dx " + prec] = R.ratio(dx.to(R.DTYPES[prec]), bref["dx"], R.store_bound(bref["e_dx"], bref["dx"], prec))
    pv = variant if variant in ("no_tail", "acc0") else None
    sums = {"dgamma": prior["dgamma"] + split_sum(g * xa, 2, order, pv), "dbeta": prior["dbeta"] + split_sum(g, 2, order, pv)}
    if head:
        sums["dW"] = prior["dW"] + split_sum(dl[:, :, None] * feat_in[:, None, :], 2, order, pv)
        sums["dbias"] = prior["dbias"] + seqsum(dl, dim=0)
    for n, got in sums.items():
        r[n] = R.ratio(got, bref[n], R.sum_bound(bref["n_" + n], bref["t_" + n]))
    return r


@pytest.mark.parametrize("order", ORDERS)
def test_head_bounds_hold(order):
    worst = {}
    for case in C.HEAD:
        for k, v in emu_head(case, order).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"head emulation ({order}): largest err/bound {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("variant,keys", [("no_tail", ("dW", "dgamma", "dbeta")), ("acc0", ("dW", "dgamma", "dbeta")), ("divN", ("feat",))])
def test_head_wrong_variants_exceed(variant, keys):
    worst = {}
    for case in C.HEAD:
        for k, v in emu_head(case, "kernel", variant).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k in keys:
        assert worst[k] > 1.0, (variant, k, worst[k])


# ---- the bit-exact class ------------------------------------------------------------------------
def _rne_bf16_bits(x):
    """Round-to-nearest-even f32 -> bf16 in integer arithmetic (finite values and infinities)."""
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def test_cast_table_and_torch_rounding():
    t = C.cast_table()
    assert t.numel() == 327680
    fin = ~torch.isnan(t)
    got = t.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got[fin], _rne_bf16_bits(t)[fin])                                    # torch's bf16 cast is RNE, ties included
    assert bool(torch.isnan(t.to(torch.bfloat16))[~fin].all())
    with np.errstate(over="ignore"):
        want16 = torch.from_numpy(t.numpy().astype(np.float16))
    assert R.equal_bits(t.to(torch.float16), want16)                                        # and its fp16 cast is numpy's
    ties = C.fp16_tie_table()
    with np.errstate(over="ignore"):
        assert R.equal_bits(ties.to(torch.float16), torch.from_numpy(ties.numpy().astype(np.float16)))
    # what the table is for: bf16 ties both ways, fp16 subnormals, fp16 overflow, infinities, NaNs
    bits = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    tie = fin & ((bits & 0xFFFF) == 0x8000)
    up = got[tie] != (bits[tie] >> 16)
    assert bool(up.any()) and bool((~up).any())
    a = t.abs()
    assert bool(((a > 0) & (a < 2.0 ** -14)).any()) and bool(((a > 65520) & fin & ~torch.isinf(t)).any()) and bool(torch.isinf(t).any()) and bool((~fin).any())
    h = ties.to(torch.float16)
    assert bool(torch.isinf(h).any()) and bool(((h.abs() > 0) & (h.abs() < 2.0 ** -14)).any())


@pytest.mark.parametrize("variant", ["truncate", "half_up"])
def test_wrong_casts_differ(variant):
    t = C.cast_table()
    t = t[~torch.isnan(t) & ~torch.isinf(t)]
    b = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    wrong = (b >> 16) if variant == "truncate" else ((b + 0x8000) >> 16)
    assert not torch.equal(wrong & 0xFFFF, _rne_bf16_bits(t))


def test_wrong_masking_tiebreak_differs():
    for regime in ("two", "zeros", "equal"):
        n = C.noise(1, 196, regime)
        ids_shuffle, ids_restore, _ = R.masking(n, 49)
        v, pos = n[0], torch.arange(196)
        rank = ((v[None, :] < v[:, None]) | ((v[None, :] == v[:, None]) & (pos[None, :] < pos[:, None]))).sum(1)
        assert torch.equal(rank.int(), ids_restore[0])     # rank counting with ties to the earlier index IS the stable argsort
        wrong = ((v[None, :] < v[:, None]) | ((v[None, :] == v[:, None]) & (pos[None, :] > pos[:, None]))).sum(1)
        assert not torch.equal(wrong.int(), ids_restore[0])


def test_wrong_im2col_differs():
    for img, p, Cc in C.IM2COL:
        imgs = C.randn(2, Cc, img, img, seed=3)
        want = R.im2col(imgs, p, None, Cc * p * p, f32)
        g = img // p
        swapped = imgs.reshape(2, Cc, g, p, g, p).permute(0, 2, 4, 1, 5, 3).reshape(-1, Cc * p * p)
        assert not torch.equal(swapped, want)
        # and the restatement against the convolution it feeds: unfold is torch's own im2col
        assert torch.equal(F.unfold(imgs, p, stride=p).transpose(1, 2).reshape(-1, Cc * p * p), want)
