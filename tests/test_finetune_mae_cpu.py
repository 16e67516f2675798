"""The fine-tune recipe's host side and the yardsticks of its kernels, without a GPU: every bound of tests/finetune_ref.py is held to an
f32 emulation of the kernel's arithmetic (which must pass) and to wrong variants (which must fail); the layer-decay groups are held to
the reference's own (tests/golden/layer_decay.json); the Mixup draws to a hand-computed sequence from a seeded RandomState."""
import json
import os
import types

import numpy as np
import pytest
import torch

import finetune_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
LAM_INEXACT = 0.9871234567891234


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- mixing
def test_mixup_bound_passes_the_emulation_and_catches_an_f32_subtraction():
    x = torch.randn(4, 3, 6, 10, generator=_gen(1))
    x[0, 0, 0, :4] = 0.0   # lam 0 + oml b: the whole value comes through 1 - lam
    for lam in (0.3, 0.0, LAM_INEXACT, 0.5000001):
        lam32, oml32 = FR.record(lam)
        want, e = FR.mixup(x, lam32, oml32)
        assert FR.ratio(FR.mixup_f32(x, lam32, oml32), want, e) <= 1.0, lam
    lam32, oml32 = FR.record(LAM_INEXACT)
    wrong = float(torch.tensor(1.0) - torch.tensor(lam32))   # 1.f - lam computed in f32
    assert wrong != oml32
    want, e = FR.mixup(x, lam32, oml32)
    assert FR.ratio(FR.mixup_f32(x, lam32, wrong), want, e) > 1.0


def test_cutmix_reference_and_a_swap_that_reads_written_values():
    x = torch.randn(4, 3, 9, 7, generator=_gen(2))
    box = (2, 6, 1, 5)
    want = FR.cutmix(x, box)
    yl, yh, xl, xh = box
    for b in range(4):
        inside = torch.zeros(9, 7, dtype=torch.bool)
        inside[yl:yh, xl:xh] = True
        assert torch.equal(want[b][:, inside], x[3 - b][:, inside]) and torch.equal(want[b][:, ~inside], x[b][:, ~inside])
    assert torch.equal(FR.cutmix(x, (3, 3, 0, 7)), x) and torch.equal(FR.cutmix(x, (0, 9, 0, 7)), x.flip(0))
    wrong = x.clone()   # sample by sample, in place: the partner gets back what was just written to it
    for b in range(4):
        wrong[b, :, yl:yh, xl:xh] = wrong[3 - b, :, yl:yh, xl:xh]
    assert not torch.equal(wrong, want)


# ---------------------------------------------------------------------------------------------------- soft-target cross-entropy
def _ce_case(B, C, seed):
    g = _gen(seed)
    logits = torch.randn(B, C, generator=g) * 2.0
    target = torch.randint(0, C, (B,), generator=g)
    if C >= 2:
        logits[:, C - 1] -= 40.0
        target[1] = C - 1
    target[B - 1] = target[0]   # the planted same-class pair
    return logits, target


def _targets_f32(target, C, lam32, oml32, on, off):
    y1 = torch.full((len(target), C), off, dtype=torch.float32).scatter_(1, target[:, None], on)
    y2 = torch.full((len(target), C), off, dtype=torch.float32).scatter_(1, target.flip(0)[:, None], on)
    return y1 * lam32 + y2 * oml32


@pytest.mark.parametrize("B,C", [(2, 1), (2, 2), (4, 5), (66, 7), (8, 1000)])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("lam", [1.0, 0.0, 0.3])
def test_soft_ce_bounds_pass_the_emulation(B, C, smoothing, lam):
    logits, target = _ce_case(B, C, B + C)
    lam32, oml32 = FR.record(lam)
    on, off = FR.on_off(smoothing, C)
    ref = FR.soft_ce(logits, target, lam32, oml32, smoothing, 0.5)
    loss, dl = FR.soft_ce_f32(logits, _targets_f32(target, C, lam32, oml32, on, off), 0.5)
    assert FR.ratio(loss, ref["loss"], ref["e_loss"]) <= 1.0 and FR.ratio(dl, ref["dlogits"], ref["e_dlogits"]) <= 1.0
    # it IS timm's SoftTargetCrossEntropy over mixup_target; at lam 1 LabelSmoothingCrossEntropy, at smoothing 0 too plain CE
    z = logits.double()
    want = torch.sum(-FR.soft_targets(target, C, lam32, oml32, smoothing) * torch.log_softmax(z, -1), -1).mean()
    assert abs(float(ref["loss"] - want)) <= 1e-12 * max(1.0, abs(float(want)))
    if lam == 1.0:
        logp = torch.log_softmax(z, -1)
        nll = -logp.gather(1, target[:, None])[:, 0]
        ls = ((1.0 - smoothing) * nll + smoothing * (-logp.mean(-1))).mean()   # timm LabelSmoothingCrossEntropy.forward
        assert abs(float(ref["loss"] - ls)) <= 1e-6 * max(1.0, abs(float(ls)))   # (on / off are f32 values: 1e-7 apart)
        if smoothing == 0.0:
            assert abs(float(ref["loss"] - torch.nn.functional.cross_entropy(z, target))) <= 1e-12 * max(1.0, abs(float(want)))


def test_soft_ce_bounds_catch_the_wrong_variants():
    B, C, smoothing = 6, 7, 0.1
    logits, target = _ce_case(B, C, 5)
    lam32, oml32 = FR.record(0.3)
    on, off = FR.on_off(smoothing, C)
    ref = FR.soft_ce(logits, target, lam32, oml32, smoothing, 1.0)
    # (a) an else-if chain over the two classes: the weights of a same-class pair do not add
    t = _targets_f32(target, C, lam32, oml32, on, off)
    chain = t.clone()
    for b in (0, B - 1):
        chain[b, target[b]] = lam32 * on + oml32 * off
    loss, dl = FR.soft_ce_f32(logits, chain, 1.0)
    assert FR.ratio(loss, ref["loss"], ref["e_loss"]) > 1.0 and FR.ratio(dl, ref["dlogits"], ref["e_dlogits"]) > 1.0
    # (b) off = smoothing / (C - 1)
    off_w = np.float32(smoothing / (C - 1))
    loss, dl = FR.soft_ce_f32(logits, _targets_f32(target, C, lam32, oml32, np.float32(1.0 - smoothing + off_w), off_w), 1.0)
    assert FR.ratio(loss, ref["loss"], ref["e_loss"]) > 1.0 and FR.ratio(dl, ref["dlogits"], ref["e_dlogits"]) > 1.0
    # (c) 1 - lam computed in f32 where lam is not an f32 value: the row without a same-class partner notices
    lam32, oml32 = FR.record(LAM_INEXACT)
    ref = FR.soft_ce(logits, target, lam32, oml32, 0.0, 1.0)
    wrong = float(torch.tensor(1.0) - torch.tensor(lam32))
    on0, off0 = FR.on_off(0.0, C)
    _, dl = FR.soft_ce_f32(logits, _targets_f32(target, C, lam32, wrong, on0, off0), 1.0)
    _, ok = FR.soft_ce_f32(logits, _targets_f32(target, C, lam32, oml32, on0, off0), 1.0)
    assert FR.ratio(ok, ref["dlogits"], ref["e_dlogits"]) <= 1.0 < FR.ratio(dl, ref["dlogits"], ref["e_dlogits"])


# ---------------------------------------------------------------------------------------------------- pool + fc_norm
def _pool_case(B, N, D, seed):
    g = _gen(seed)
    x = torch.randn(B, N, D, generator=g) * 2.0 + 0.5
    x[:, 0] = 1e4 * torch.randn(B, D, generator=g)
    return x, torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(B, D, generator=g)


@pytest.mark.parametrize("B,N,D", [(2, 197, 768), (3, 50, 64), (1, 2, 64)])
def test_pool_bounds_pass_the_emulation_and_catch_the_wrong_variants(B, N, D):
    x, gamma, beta, dfeat = _pool_case(B, N, D, N + D)
    fwd = FR.pool_fwd(x, gamma, beta)
    # forward in f32: the two-stage sum (32-row partials, ascending), / (N - 1), LayerNorm
    parts = [x[:, n0:min(n0 + 32, N)].sum(1) for n0 in range(1, N, 32)]
    pooled = torch.stack(parts).sum(0) / float(N - 1)
    mean = pooled.sum(-1, keepdim=True) / D
    rstd = torch.rsqrt(((pooled - mean) ** 2).sum(-1, keepdim=True) / D + 1e-6)
    feat = (pooled - mean) * rstd * gamma + beta
    assert FR.ratio(pooled, fwd["pooled"], fwd["e_pooled"]) <= 1.0 and FR.ratio(feat, fwd["feat"], fwd["e_feat"]) <= 1.0
    assert FR.ratio(mean[:, 0], fwd["mean"], fwd["e_mean"]) <= 1.0 and FR.ratio(rstd[:, 0], fwd["rstd"], fwd["e_rstd"]) <= 1.0
    if N > 2:   # the mean over N rows instead of N - 1 (the cls row counted in the divisor)
        assert FR.ratio(torch.stack(parts).sum(0) / float(N), fwd["pooled"], fwd["e_pooled"]) > 1.0
    # backward from the f32 statistics
    ref = FR.pool_bwd(dfeat, pooled, mean[:, 0], rstd[:, 0], gamma, N)
    row = FR.pool_bwd_f32(dfeat, pooled, mean[:, 0], rstd[:, 0], gamma, N)
    dx = row[:, None].expand(B, N, D).clone()
    dx[:, 0] = 0.0
    assert FR.ratio(dx, ref["dx"], ref["e_dx"]) <= 1.0
    with_cls = row[:, None].expand(B, N, D)   # the cls row included in dx
    assert FR.ratio(with_cls, ref["dx"], ref["e_dx"]) > 1.0
    over_n = dx * float(N - 1) / float(N)      # dpooled / N
    assert FR.ratio(over_n, ref["dx"], ref["e_dx"]) > 1.0
    # it is autograd's gradient of fc_norm(x[:, 1:].mean(1))
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xd[:, 1:].mean(1), (D,), gd, bd, 1e-6)
    y.backward(dfeat.double())
    exact = FR.pool_bwd(dfeat, fwd["pooled"], fwd["mean"], fwd["rstd"], gamma, N)
    assert torch.allclose(exact["dx"], xd.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(exact["dgamma"], gd.grad, rtol=1e-9, atol=1e-12) and torch.allclose(exact["dbeta"], bd.grad, rtol=1e-9, atol=1e-12)
    # dgamma / dbeta in f32, ascending over b, into a prior value
    prior = {"dgamma": torch.randn(D, generator=_gen(3)) * 0.3, "dbeta": torch.randn(D, generator=_gen(4)) * 0.3}
    ref = FR.pool_bwd(dfeat, pooled, mean[:, 0], rstd[:, 0], gamma, N, prior=prior)
    sg, sb = torch.zeros(D), torch.zeros(D)
    for b in range(B):
        sg = sg + dfeat[b] * ((pooled[b] - mean[b]) * rstd[b])
        sb = sb + dfeat[b]
    assert FR.ratio(prior["dgamma"] + sg, ref["dgamma"], FR.sum_bound(ref["n_dgamma"] + 1, ref["t_dgamma"])) <= 1.0
    assert FR.ratio(prior["dbeta"] + sb, ref["dbeta"], FR.sum_bound(ref["n_dbeta"] + 1, ref["t_dbeta"])) <= 1.0


def test_linear_head_bounds_pass_the_emulation():
    g = _gen(9)
    feat, W, bias = torch.randn(5, 768, generator=g) * 1.5, torch.randn(7, 768, generator=g) / 768 ** 0.5, torch.randn(7, generator=g) * 0.1
    dl = torch.randn(5, 7, generator=g) * 0.1
    want, e = FR.linear(feat, W, bias)
    assert FR.ratio(feat @ W.T + bias, want, e) <= 1.0
    want, e = FR.dfeat(dl, W)
    acc = torch.zeros(5, 768)
    for c in range(7):   # ascending over the classes
        acc = acc + dl[:, c:c + 1] * W[c]
    assert FR.ratio(acc, want, e) <= 1.0
    assert FR.ratio(acc * (1 + 1e-5), want, e) > 1.0


# ---------------------------------------------------------------------------------------------------- layer decay
def test_param_groups_lrd_equal_the_reference_fixture():
    from ssl4polyp_amd import models_vit
    from ssl4polyp_amd.lr_decay import get_layer_id_for_vit, param_groups_lrd
    with open(os.path.join(HERE, "golden", "layer_decay.json")) as fh:
        cases = json.load(fh)["cases"]
    assert {(c["depth"], c["global_pool"]) for c in cases} == {(12, False), (12, True), (32, True), (32, False)}
    assert any(c["frozen"] for c in cases)
    for c in cases:
        model = models_vit.VisionTransformer(img_size=32, patch_size=16, embed_dim=8, depth=c["depth"], num_heads=2, num_classes=3,
                                             global_pool=c["global_pool"])
        assert [n for n, _ in model.named_parameters()] == c["all_names"], "the model's parameter names and order are timm's"
        assert model.no_weight_decay() == set(c["no_weight_decay"]) == {"pos_embed", "cls_token"}
        for n, p in model.named_parameters():
            p.requires_grad_(n not in c["frozen"])
        groups = param_groups_lrd(model, c["weight_decay"], model.no_weight_decay(), c["layer_decay"], with_names=True)
        got = [{"name": g["name"], "lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"], "params": g["param_names"]} for g in groups]
        assert got == c["groups"]
        by_name = dict(model.named_parameters())
        assert all([by_name[n] is p for n, p in zip(g["param_names"], g["params"])] for g in groups)
        plain = param_groups_lrd(model, c["weight_decay"], model.no_weight_decay(), c["layer_decay"])
        assert all(sorted(g) == ["lr_scale", "params", "weight_decay"] for g in plain)   # what the reference returns
        L = c["depth"] + 1
        assert groups[-1]["lr_scale"] == 1.0 and get_layer_id_for_vit("fc_norm.weight", L) == L == get_layer_id_for_vit("head.bias", L)
        assert get_layer_id_for_vit("blocks.3.mlp.fc1.weight", L) == 4 and get_layer_id_for_vit("patch_embed.proj.bias", L) == 0


def test_adjust_learning_rate_applies_lr_scale():
    from ssl4polyp_amd.train import adjust_learning_rate
    opt = types.SimpleNamespace(param_groups=[{"lr_scale": 0.75 ** 3}, {"lr_scale": 1.0}, {}])
    args = types.SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=5, epochs=50)
    lr = adjust_learning_rate(opt, 2.5, args)
    assert lr == 1e-3 * 2.5 / 5 and [g["lr"] for g in opt.param_groups] == [lr * 0.75 ** 3, lr, lr]


# ---------------------------------------------------------------------------------------------------- Mixup draws
def test_mixup_draws_follow_the_documented_order():
    from ssl4polyp_amd.mixup import Mixup
    H, W = 224, 160
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, switch_prob=0.5, label_smoothing=0.1, num_classes=10,
                rng=np.random.RandomState(7))
    rs = np.random.RandomState(7)   # the same stream, consumed by hand in the documented order
    kinds = set()
    for _ in range(40):
        lam, cut, box = mix.draw((8, 3, H, W))
        if not rs.rand() < 0.9:
            want = (1.0, False, (0, 0, 0, 0))
        else:
            use_cutmix = bool(rs.rand() < 0.5)
            lam0 = float(rs.beta(1.0, 1.0) if use_cutmix else rs.beta(0.8, 0.8))
            if use_cutmix:
                ratio = np.sqrt(1 - lam0)
                cut_h, cut_w = int(H * ratio), int(W * ratio)
                cy = rs.randint(0, H)
                cx = rs.randint(0, W)
                yl, yh = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
                xl, xh = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
                want = (1.0 - (yh - yl) * (xh - xl) / float(H * W), True, (yl, yh, xl, xh))
            else:
                want = (lam0, False, (0, 0, 0, 0))
        assert (lam, cut, box) == want
        kinds.add((cut, lam == 1.0))
    assert kinds == {(True, False), (False, False), (False, True)}, "CutMix, Mixup and the no-mix draw all occurred"
    # the first draws of RandomState(7), written out: rand() = 0.0763 < 0.9; rand() = 0.7799 >= 0.5 -> Mixup; beta(0.8, 0.8)
    first = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, switch_prob=0.5, rng=np.random.RandomState(7)).draw((8, 3, H, W))
    chk = np.random.RandomState(7)
    assert abs(chk.rand() - 0.07630829) < 1e-8 and abs(chk.rand() - 0.77991879) < 1e-8
    assert first == (float(chk.beta(0.8, 0.8)), False, (0, 0, 0, 0))
    # one alpha only: no switch draw
    only_cut = Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, rng=np.random.RandomState(3))
    rs = np.random.RandomState(3)
    assert rs.rand() < 1.0
    lam0 = float(rs.beta(1.0, 1.0))
    _, cut, _ = only_cut.draw((2, 3, 32, 32))
    assert cut is True and rs.randint(0, 32) >= 0
    only_mix = Mixup(mixup_alpha=0.8, cutmix_alpha=0.0, rng=np.random.RandomState(3))
    rs = np.random.RandomState(3)
    rs.rand()
    assert only_mix.draw((2, 3, 32, 32)) == (float(rs.beta(0.8, 0.8)), False, (0, 0, 0, 0))


def test_prob_zero_never_mixes_and_the_box_is_clipped_at_every_edge():
    from ssl4polyp_amd.mixup import Mixup, cutmix_bbox_and_lam, rand_bbox
    never = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, rng=np.random.RandomState(1))
    assert all(never.draw((4, 3, 32, 32)) == (1.0, False, (0, 0, 0, 0)) for _ in range(20))

    class Fixed:   # randint returns the centres it is given: cy first, then cx
        def __init__(self, cy, cx):
            self.vals = [cy, cx]

        def randint(self, lo, hi):
            v = self.vals.pop(0)
            assert lo <= v < hi
            return v

    H, W, lam = 20, 30, 0.75   # ratio 0.5: cut_h 10, cut_w 15 -> half sizes 5 and 7
    assert rand_bbox((2, 3, H, W), lam, Fixed(10, 15)) == (5, 15, 8, 22)        # inside
    assert rand_bbox((2, 3, H, W), lam, Fixed(0, 15)) == (0, 5, 8, 22)          # top
    assert rand_bbox((2, 3, H, W), lam, Fixed(19, 15)) == (14, 20, 8, 22)       # bottom
    assert rand_bbox((2, 3, H, W), lam, Fixed(10, 0)) == (5, 15, 0, 7)          # left
    assert rand_bbox((2, 3, H, W), lam, Fixed(10, 29)) == (5, 15, 22, 30)       # right
    assert rand_bbox((2, 3, H, W), lam, Fixed(0, 0)) == (0, 5, 0, 7)            # a corner
    box, lam2 = cutmix_bbox_and_lam((2, 3, H, W), lam, Fixed(19, 29))
    assert box == (14, 20, 22, 30) and lam2 == 1.0 - 6 * 8 / 600.0
    box, lam2 = cutmix_bbox_and_lam((2, 3, H, W), 0.9999, Fixed(3, 4))          # a box of no area: lam back to 1
    assert box[1] - box[0] == 0 and lam2 == 1.0


def test_refusals_and_the_record():
    from ssl4polyp_amd import main_finetune_mae, mixup
    for mode in ("pair", "elem"):
        with pytest.raises(NotImplementedError, match="batch"):
            mixup.Mixup(mode=mode)
    with pytest.raises(NotImplementedError, match="cutmix_minmax"):
        mixup.Mixup(cutmix_minmax=(0.2, 0.8))
    assert "not been checked against timm" in " ".join(mixup.Mixup.__doc__.split())
    words = mixup.MixState.pack(LAM_INEXACT, True, (1, 2, 3, 4))
    assert words.dtype == np.int32 and words.shape == (8,) and words[2:].tolist() == [1, 1, 2, 3, 4, 0]
    assert tuple(float(v) for v in np.frombuffer(words.tobytes(), dtype=np.float32)[:2]) == FR.record(LAM_INEXACT)
    parse = main_finetune_mae.get_args_parser().parse_args
    main_finetune_mae.check_supported(parse([]))
    assert parse([]).drop_path == 0.0 and parse([]).global_pool is True and parse(["--cls_token"]).global_pool is False
    for flags, gap in ((["--drop_path", "0.1"], "stochastic depth"), (["--aa", "rand-m9-mstd0.5-inc1"], "RandAugment"),
                       (["--reprob", "0.25"], "random erasing"), (["--color_jitter", "0.4"], "colour jitter"), (["--dist_eval"], "one GPU"),
                       (["--mixup_mode", "elem"], "batch"), (["--cutmix_minmax", "0.2", "0.8"], "cutmix_minmax")):
        with pytest.raises(NotImplementedError, match=gap):
            main_finetune_mae.check_supported(parse(flags))
    a, b = main_finetune_mae.mix_rng(3, 1), main_finetune_mae.mix_rng(3, 1)
    assert a.rand() == b.rand() and main_finetune_mae.mix_rng(3, 2).rand() != main_finetune_mae.mix_rng(3, 1).rand()


def test_load_pretrained_for_finetune():
    """main_finetune.py:255-279: both pools' missing-key assertions, the head's std 2e-5, another grid refused."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd import _lib, models_vit
    torch.manual_seed(0)
    mae = A.MaskedAutoencoderViT(embed_dim=64, depth=2, num_heads=2, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2)
    ckpt = {k: v.clone() for k, v in mae.state_dict().items()}
    cls = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=500)
    msg = models_vit.load_pretrained_for_finetune(cls, ckpt)
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} and all("decoder" in k or k == "mask_token" for k in msg.unexpected_keys)
    assert torch.equal(cls.blocks[1].mlp.fc2.weight, mae.blocks[1].mlp.fc2.weight)
    assert 1e-5 < float(cls.head.weight.detach().std()) < 3e-5 and float(cls.head.bias.detach().abs().max()) == 0.0
    pooled = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=5, global_pool=True)
    with pytest.raises(AssertionError):   # the MAE's final norm is an unexpected key there, but a stray fc_norm is not missing
        models_vit.load_pretrained_for_finetune(pooled, {**ckpt, "fc_norm.weight": torch.ones(64)})
    msg = models_vit.load_pretrained_for_finetune(pooled, ckpt)
    assert set(msg.missing_keys) == {"head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"} and "norm.weight" in msg.unexpected_keys
    with pytest.raises(AssertionError):
        models_vit.load_pretrained_for_finetune(cls, {k: v for k, v in ckpt.items() if k != "cls_token"})
    wrong_head = {**ckpt, "head.weight": torch.zeros(3, 64), "head.bias": torch.zeros(3)}
    assert set(models_vit.load_pretrained_for_finetune(cls, wrong_head).missing_keys) == {"head.weight", "head.bias"}
    with pytest.raises(_lib.PolypMaeError):
        models_vit.load_pretrained_for_finetune(cls, {**ckpt, "pos_embed": torch.zeros(1, 50, 64)})


def test_the_new_entry_points_are_declared_and_bound():
    from ssl4polyp_amd import _lib
    with open(os.path.join(HERE, "..", "include", "polypmae.h")) as fh:
        header = fh.read()
    for name in ("pm_mix_batch", "pm_soft_ce_workspace", "pm_soft_ce", "pm_pool_norm_fwd_train", "pm_pool_norm_bwd_workspace",
                 "pm_pool_norm_bwd", "pm_linear_head_fwd", "pm_linear_head_dfeat"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    import ctypes
    assert ctypes.sizeof(_lib.MixRecord) == 32
