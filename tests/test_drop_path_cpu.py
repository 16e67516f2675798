"""Stochastic depth of the fine-tune ViT, the part that needs no GPU: the per-block rates, when the draw is active, the refusals,
the host restatement of the scale table (tests/drop_path_ref.py) with the property the GPU model test relies on, the C-ABI
declarations, and a float64 autograd check of the tests' own reference block."""
import os
import re

import numpy as np
import pytest
import torch

import drop_path_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pm_drop_path_add", "pm_drop_path_scale_cast", "pm_drop_path_scales", "pm_drop_path_workspace")


def _model(depth, **kw):
    from ssl4polyp_amd import models_vit
    return models_vit.VisionTransformer(embed_dim=64, depth=depth, num_heads=2, num_classes=5, **kw)


@pytest.mark.parametrize("depth", [1, 2, 12])
@pytest.mark.parametrize("rate", [0.1, 0.3])
def test_rates_follow_linspace(depth, rate):
    m = _model(depth, drop_path_rate=rate)
    assert m.drop_path_rates == [float(v) for v in torch.linspace(0, rate, depth)]
    assert len(m.drop_path_rates) == depth and m.drop_path_rates[0] == 0.0 and m.drop_path_rate == rate
    if depth > 1:
        assert m.drop_path_rates[-1] == float(torch.tensor(rate, dtype=torch.float32))


def test_active_in_training_at_a_positive_rate_only():
    m = _model(2, drop_path_rate=0.5)
    assert m.training and m.drop_path_active
    m.eval()
    assert not m.drop_path_active
    m.train()
    assert m.drop_path_active and m.last_drop_scales is None
    z = _model(2)
    assert z.drop_path_rate == 0.0 and z.drop_path_rates == [0.0, 0.0] and not z.drop_path_active
    assert not _model(2, drop_path_rate=0.0).drop_path_active
    # the state dict is the reference's, with or without the argument
    assert list(m.state_dict()) == list(z.state_dict())


@pytest.mark.parametrize("rate", [-0.1, 1.0])
def test_rates_outside_the_unit_interval_are_refused(rate):
    with pytest.raises(ValueError, match="drop_path_rate"):
        _model(2, drop_path_rate=rate)


def test_factories_pass_the_rate_through():
    from ssl4polyp_amd import models_vit
    m = models_vit.vit_base_patch16(num_classes=3, global_pool=True, drop_path_rate=0.1)
    assert m.drop_path_rates == [float(v) for v in torch.linspace(0, 0.1, 12)]


def test_the_draw_is_refused_under_stream_capture(monkeypatch):
    from ssl4polyp_amd import _lib
    m = _model(2, drop_path_rate=0.5)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.PolypMaeError, match="under stream capture.*baked into the graph.*drop_scales="):
        m._draw_drop_scales(4, torch.device("cuda", 0))


def test_scale_rule():
    """fl32(keep + u) >= 1 keeps; a kept branch carries fl32(1 / keep); rate 0 keeps everything at exactly 1."""
    u = np.array([0.0, 0.2499999, 0.25, 0.4999999, 0.5, 0.75, 0.99999994], dtype=np.float32)   # (the sums below 1 are exact)
    noise = np.broadcast_to(u, (3, 2, u.size))
    t = R.scales_from_noise(noise, [0.0, 0.25, 0.5])
    assert t.dtype == np.float32 and (t[0] == 1.0).all()
    assert (t[1] == np.where(u >= np.float32(0.25), np.float32(1) / np.float32(0.75), 0).astype(np.float32)).all()
    assert (t[2] == np.where(u >= np.float32(0.5), np.float32(2.0), 0).astype(np.float32)).all()
    # the f32 sum decides, not the exact one: 0.9 + 0.099999994 rounds up to 1
    keep = np.float32(1) - np.float32(0.1)
    edge = np.float32(0.099999994)
    assert np.float32(keep + edge) >= 1 and float(keep) + float(edge) < 1
    assert R.scales_from_noise(np.full((1, 2, 1), edge, np.float32), [0.1])[0, 0, 0] == np.float32(1) / keep


def test_the_model_tests_seed_keeps_and_drops_in_every_branch():
    """The GPU model test seeds the device generator with MODEL_SEED right before its forward (offset 0) and, for the accumulation
    case, runs a second forward behind it: both tables, by construction, have a kept and a dropped sample in each branch of every
    block above 0, and ones in block 0."""
    rates = R.rates(R.MODEL_RATE, R.MODEL["depth"])
    assert rates == [0.0, 0.25, 0.5]
    n = R.MODEL["depth"] * 2 * R.MODEL_B
    assert R.drawn(n) == 48 and R.drawn(5) == 8
    tables = [R.scale_table(R.MODEL_SEED, off, rates, R.MODEL_B) for off in (0, R.drawn(n))]
    assert not np.array_equal(tables[0], tables[1])
    for t in tables:
        assert t.shape == (3, 2, R.MODEL_B) and (t[0] == 1.0).all()
        for i in (1, 2):
            inv = np.float32(1) / (np.float32(1) - np.float32(rates[i]))
            for j in (0, 1):
                kept = int((t[i, j] == inv).sum())
                assert 0 < kept < R.MODEL_B and int((t[i, j] == 0).sum()) == R.MODEL_B - kept, (i, j, t[i, j])
    a = R.arbitrary_table(3, 8)
    assert a.unique().numel() == 3 * 2 * 8 - 5 and int((a == 0).sum()) == 6 and bool(torch.isfinite(a).all())


def test_symbols_are_declared_in_the_header_and_the_binding():
    from ssl4polyp_amd import _lib
    import __graft_entry__ as g
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polypmae.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared in include/polypmae.h"
        assert name in _lib.SIGNATURES, name + " is not bound in _lib.SIGNATURES"
    assert len(_lib.SIGNATURES["pm_drop_path_add"]) == 8 and len(_lib.SIGNATURES["pm_drop_path_scale_cast"]) == 11
    assert len(_lib.SIGNATURES["pm_drop_path_scales"]) == 6 and len(_lib.SIGNATURES["pm_drop_path_workspace"]) == 3
    assert "pm_droppath.hip" in g.SOURCES and g.SOURCE_FLAGS["pm_droppath.hip"] == ["-ffp-contract=off"]


def test_workspace_query_answers_without_a_gpu():
    import __graft_entry__ as g
    from ssl4polyp_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    small, big = _lib.workspace_bytes("pm_drop_path_workspace", 1, 4), _lib.workspace_bytes("pm_drop_path_workspace", 64 * 197, 768)
    assert small >= 16 and small % 16 == 0 and big % 16 == 0
    assert big >= 768 * 4 and big <= 1024 * 768 * 4   # partial rows: at least one, no more than the LayerNorm backward keeps
    with pytest.raises(_lib.PolypMaeError):
        _lib.workspace_bytes("pm_drop_path_workspace", 8, 6)   # D % 4


def test_reference_block_drops_a_sample_exactly():
    """The float64 block the GPU tests compare against, one block, B = 3: the sample with s = 0 in both branches passes through
    (d out / d x = I), contributes nothing to any weight gradient, and the kept samples' gradients are those of the scaled block."""
    from oracle import vit_mae_ref as O
    cfg = O.ViTConfig(img_size=32, patch_size=8, embed_dim=16, depth=1, num_heads=2)
    g = torch.Generator().manual_seed(3)
    sd = {n: (torch.randn(s, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
          for n, s in O.param_shapes(cfg, False, None) if n.startswith("blocks.0.")}
    B, N, D = 3, 5, 16
    x = torch.randn(B, N, D, generator=g, dtype=torch.float64, requires_grad=True)
    s_attn = torch.tensor([1.25, 0.0, 2.0], dtype=torch.float64)
    s_mlp = torch.tensor([0.5, 0.0, 1.5], dtype=torch.float64)
    out = R.block(x, sd, "blocks.0.", 2, s_attn, s_mlp)
    assert torch.equal(out[1], x[1].detach())                       # bit for bit through both branches
    dy = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    names = sorted(sd)
    full = torch.autograd.grad(out, [x] + [sd[n] for n in names], dy, retain_graph=True)
    assert torch.equal(full[0][1], dy[1])                           # d out / d x = I for the dropped sample
    assert not torch.equal(full[0][0], dy[0])
    kept = dy.clone()
    kept[1] = 0
    without = torch.autograd.grad(out, [sd[n] for n in names], kept)
    for n, a, b in zip(names, full[1:], without):
        assert torch.equal(a, b), n + ": the dropped sample reached a weight gradient"
    # and the scales really scale: s = 1 everywhere is the oracle's own block
    ones = torch.ones(B, dtype=torch.float64)
    assert torch.equal(R.block(x, sd, "blocks.0.", 2, ones, ones), O.block(x, sd, "blocks.0.", 2))
