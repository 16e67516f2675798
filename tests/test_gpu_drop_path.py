"""Stochastic depth on the device: the three kernels of csrc/pm_droppath.hip alone (bit-equal to torch where a result is one
rounding, float64 element-wise bounds for the column sum), and models_vit.VisionTransformer(drop_path_rate=...) against a float64
model that applies the scale table read back from the device (tests/drop_path_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import drop_path_ref as R
from rowops_ref import U32

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32
GUARD, FILL = 64, 12345.0
# tests/test_gpu_finetune_mae.py MODEL_TOL, the bounds of the same model without drop path: (logits max-rel, gradient rel-L2)
MODEL_TOL = {"fp32": (1e-4, 1e-3), "bf16": (7.5e-3, 1.5e-2)}
# fp16: tests/test_gpu_models.py states no fp16 pair; __graft_entry__.smoke's rule for the mode is used: 11 significant bits per
# operand instead of 8 = 1/8 of the bf16 bounds, x 1.5
MODEL_TOL["fp16"] = (7.5e-3 / 8 * 1.5, 1.5e-2 / 8 * 1.5)
SHAPES = [(1, 1, 4), (3, 5, 8), (2, 197, 768), (2, 257, 1280)]   # (B, N, D)
ACT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PM_EINVAL, PM_ESHAPE = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def abi(name, *args):
    from ssl4polyp_amd import _lib
    return getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream())


def _guarded(shape, dtype=f32, init=None):
    """A tensor that is a slice of a larger buffer: GUARD elements of FILL in front and behind (16-byte aligned); NaN-filled unless
    `init` is given (tests/test_gpu_finetune_mae.py)."""
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if init is not None:
        view.copy_(init)
    else:
        view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_hold(buf, what):
    assert bool((buf[:GUARD] == FILL).all()), what + ": written in front of the buffer"
    assert bool((buf[-GUARD:] == FILL).all()), what + ": written behind the buffer"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _scales(B):
    """Distinct per sample, a zero among them from B = 2 on."""
    return torch.tensor([1.25] if B == 1 else [0.0, 1.25, 0.5, 2.0][:B], dtype=f32, device=DEV)


def _workspace(M, D):
    from ssl4polyp_amd import _lib
    need = _lib.workspace_bytes("pm_drop_path_workspace", M, D)
    return need, torch.full((need // 4,), FILL, dtype=f32, device=DEV)


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("alias", [False, True], ids=["out", "in_place"])
def test_drop_path_add_equals_torch_bit_for_bit(shape, alias):
    B, N, D = shape
    M = B * N
    g = _gen(M + D)
    x = torch.randn(M, D, generator=g).to(DEV)
    y = torch.randn(M, D, generator=g).to(DEV)
    s = _scales(B)
    rows = s.repeat_interleave(N)
    want = x + y * rows[:, None]
    if alias:
        buf, out = _guarded((M, D), init=y)
        assert abi("pm_drop_path_add", x, out, out, s, M, N, D) == 0
    else:
        buf, out = _guarded((M, D))
        assert abi("pm_drop_path_add", x, y, out, s, M, N, D) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "pm_drop_path_add")
    assert torch.equal(out, want)
    if B > 1:   # the dropped sample keeps its residual stream bit for bit
        assert float(s[0]) == 0.0 and torch.equal(out[:N].view(torch.int32), x[:N].view(torch.int32))
        assert not torch.equal(out[N:2 * N], x[N:2 * N])


def test_drop_path_add_refusals():
    x = torch.zeros(4, 8, device=DEV)
    s = torch.ones(2, device=DEV)
    assert abi("pm_drop_path_add", x, x, x, s, 4, 2, 6) == PM_ESHAPE      # D % 4
    assert abi("pm_drop_path_add", x, x, x, s, 4, 3, 8) == PM_ESHAPE      # M is not a whole number of samples
    assert abi("pm_drop_path_add", x, None, x, s, 4, 2, 8) == PM_EINVAL
    assert abi("pm_drop_path_add", x, x, x, None, 4, 2, 8) == PM_EINVAL


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_drop_path_scale_cast(shape, prec):
    B, N, D = shape
    M = B * N
    dt = ACT[prec]
    g = _gen(3 * M + D)
    dy = torch.randn(M, D, generator=g).to(DEV)
    prior = torch.randn(D, generator=g).to(DEV)
    s = _scales(B)
    rows = s.repeat_interleave(N)
    want_act = (dy * rows[:, None]).to(dt)
    need, ws = _workspace(M, D)
    runs = []
    for _ in range(2):
        abuf, act = _guarded((M, D), dtype=dt)
        cbuf, col = _guarded((D,), init=prior)
        assert abi("pm_drop_path_scale_cast", dy, s, act, {"fp32": 0, "bf16": 1, "fp16": 2}[prec], col, M, N, D, ws, need) == 0
        torch.cuda.synchronize()
        _guards_hold(abuf, "pm_drop_path_scale_cast dy_act")
        _guards_hold(cbuf, "pm_drop_path_scale_cast colsum")
        runs.append((act.clone(), col.clone()))
    assert torch.equal(runs[0][0], want_act)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ in their bits"
    # the column sum ADDS to what was there.  Element-wise float64 bound of tests/rowops_ref.py's form, (terms + 1) u32 sum|.|: the
    # M products (exact in float64, one f32 rounding each in the kernel) and the prior value are M + 1 terms
    prod = dy.double() * rows.double()[:, None]
    want = prior.double() + prod.sum(0)
    bound = (M + 2) * U32 * (prod.abs().sum(0) + prior.double().abs())
    err = (runs[0][1].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"scale_cast {shape} {prec}: colsum err/bound {ratio:.3f}")
    assert ratio <= 1.0
    assert not torch.equal(runs[0][1], prior)


@pytest.mark.parametrize("shape", [(3, 5, 8), (2, 197, 768)])
def test_drop_path_scale_cast_without_a_column_sum_and_refusals(shape):
    B, N, D = shape
    M = B * N
    dy = torch.randn(M, D, generator=_gen(5)).to(DEV)
    s = _scales(B)
    need, ws = _workspace(M, D)
    abuf, act = _guarded((M, D), dtype=torch.bfloat16)
    cbuf, col = _guarded((D,), init=torch.ones(D))
    # colsum = NULL: no workspace is needed, none is touched, and nothing is written outside dy_act
    assert abi("pm_drop_path_scale_cast", dy, s, act, 1, None, M, N, D, None, 0) == 0
    assert abi("pm_drop_path_scale_cast", dy, s, act, 1, None, M, N, D, ws, need) == 0
    torch.cuda.synchronize()
    _guards_hold(abuf, "pm_drop_path_scale_cast dy_act")
    _guards_hold(cbuf, "an unused colsum buffer")
    assert torch.equal(act, (dy * s.repeat_interleave(N)[:, None]).to(torch.bfloat16))
    assert bool((ws == FILL).all()) and bool((col == 1).all())
    # with a column sum the workspace must be there and large enough; nothing runs otherwise
    assert abi("pm_drop_path_scale_cast", dy, s, act, 1, col, M, N, D, ws, need - 4) == PM_EINVAL
    assert abi("pm_drop_path_scale_cast", dy, s, act, 1, col, M, N, D, None, 0) == PM_EINVAL
    assert abi("pm_drop_path_scale_cast", dy, s, act, 7, col, M, N, D, ws, need) == PM_EINVAL   # no such dtype
    assert abi("pm_drop_path_scale_cast", dy, s, act, 1, col, M, N + 1, D, ws, need) == PM_ESHAPE
    torch.cuda.synchronize()
    assert bool((col == 1).all()) and bool((ws == FILL).all())


def test_drop_path_scales_equal_the_host_table():
    depth, B, rates = 3, 8, [0.0, 0.25, 0.5]
    rates_dev = torch.tensor(rates, dtype=f32, device=DEV)
    for seed, off in ((R.MODEL_SEED, 0), (123456789012345, (7 << 32) + 48)):
        key, sid = R.draw_key(seed, off)
        nbuf, noise = _guarded((depth, 2, B))
        obuf, out = _guarded((depth, 2, B))
        assert abi("pm_mae_noise", noise, depth * 2 * B, ctypes.c_ulonglong(key), ctypes.c_uint(sid)) == 0
        assert abi("pm_drop_path_scales", noise, rates_dev, out, depth, B) == 0
        torch.cuda.synchronize()
        _guards_hold(nbuf, "pm_mae_noise")
        _guards_hold(obuf, "pm_drop_path_scales")
        want = R.scale_table(seed, off, rates, B)
        assert np.array_equal(out.cpu().numpy(), want)
        assert bool((out[0] == 1.0).all()) and set(out[2].unique().tolist()) == {0.0, 2.0}
    # values at the rule's edges, where the f32 sum rounds up to 1 and the exact one stays below
    edges = np.array([0.0, 0.099999994, 0.09999999, 0.1, 0.3, 0.29999998, 0.5, 0.99999994], dtype=np.float32)
    noise = torch.from_numpy(np.broadcast_to(edges, (4, 2, 8)).copy()).to(DEV)
    rates = [0.0, 0.1, 0.3, float(torch.linspace(0, 0.3, 12)[7])]
    out = torch.empty_like(noise)
    assert abi("pm_drop_path_scales", noise, torch.tensor(rates, dtype=f32, device=DEV), out, 4, 8) == 0
    assert np.array_equal(out.cpu().numpy(), R.scales_from_noise(noise.cpu().numpy(), rates))
    assert abi("pm_drop_path_scales", noise, None, out, 4, 8) == PM_EINVAL
    assert abi("pm_drop_path_scales", noise, out, out, 0, 8) == PM_ESHAPE


# ---------------------------------------------------------------------------------------------------- the model
B, C = R.MODEL_B, R.MODEL_C
_UNSET = object()


def _model(pool, prec, rate=R.MODEL_RATE, seed=11):
    """The tiny fine-tune model (three blocks) with every parameter away from its initial value, as tests/test_gpu_finetune_mae.py
    builds it; rate=_UNSET: built without the argument."""
    from ssl4polyp_amd import models_vit
    torch.manual_seed(seed)
    kw = {} if rate is _UNSET else {"drop_path_rate": rate}
    model = models_vit.VisionTransformer(num_classes=C, global_pool=pool, precision=prec, **R.MODEL, **kw)
    g = _gen(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n == "head.weight":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif p.ndim == 1:
                p.add_(torch.randn(p.shape, generator=g) * (0.1 if n.endswith("weight") else 0.02))
    return model.to(DEV)


def _batch(seed):
    g = _gen(seed)
    imgs = torch.randn(B, 3, 224, 224, generator=g)
    target = torch.randint(0, C, (B,), generator=g)
    return imgs.to(DEV), target.to(DEV)


def _loss(logits, target):
    return torch.nn.functional.cross_entropy(logits, target)


_REF = {}


def _float64(model, imgs, target, pool, scales, tag):
    """Logits and every parameter gradient of the float64 model with `scales` applied, on the model's own weights.  Computed once
    per (pool, tag): the seeded weights are the same in every precision mode, and nothing changes a cached result."""
    key = (pool, tag)
    if key not in _REF:
        from oracle import vit_mae_ref as O
        cfg = O.ViTConfig(img_size=224, patch_size=16, **R.MODEL)
        leaves = {n: v.detach().double().cpu().requires_grad_(True) for n, v in model.state_dict().items()}
        logits = R.vit_finetune_logits(leaves, imgs.detach().double().cpu(), cfg, pool, scales.detach().double().cpu())
        _loss(logits, target.cpu()).backward()
        _REF[key] = (logits.detach(), {n: v.grad for n, v in leaves.items()})
    return _REF[key]


def _without_key_bias(n, g):
    """attn.qkv.bias: the key part has a zero gradient (softmax is invariant to it), pure round-off: tests/test_gpu_models.py:133."""
    if n.endswith("attn.qkv.bias"):
        D = g.numel() // 3
        return torch.cat([g[:D], g[2 * D:]])
    return g


def _compare(model, logits, want_logits, want, prec, what, scale=1.0, only=None):
    tl, tg = MODEL_TOL[prec]
    e = rel(logits, want_logits)
    print(f"{what}: logits max-rel {e:.2e} (bound {tl:.1e})")
    assert logits.shape == (B, C) and e < tl, (what, e)
    worst = 0.0
    for n, p in model.named_parameters():
        if only is not None and not only(n):
            assert p.grad is None, n + " is frozen and got a gradient"
            continue
        assert p.grad is not None, n + " got no gradient"
        e = rel_l2(_without_key_bias(n, p.grad / scale), _without_key_bias(n, want[n]))
        worst = max(worst, e)
        assert e < tg, (what, n, e)
    print(f"{what}: worst gradient rel-L2 {worst:.2e} (bound {tg:.1e})")


def _host_table(offset=0):
    return torch.from_numpy(R.scale_table(R.MODEL_SEED, offset, R.rates(R.MODEL_RATE, R.MODEL["depth"]), B))


@pytest.mark.parametrize("pool", [True, False], ids=["global_pool", "cls_token"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_model_with_its_own_draw_against_float64(pool, prec):
    model = _model(pool, prec)
    imgs, target = _batch(41)
    model.train()
    torch.manual_seed(R.MODEL_SEED)
    logits = model(imgs)
    _loss(logits, target).backward()
    table = model.last_drop_scales
    # the device's table is the host restatement's, whose drops and keeps tests/test_drop_path_cpu.py asserts by construction
    assert table.shape == (3, 2, B) and torch.equal(table.cpu(), _host_table())
    want_logits, want = _float64(model, imgs, target, pool, table, "drawn")
    _compare(model, logits, want_logits, want, prec, f"drawn table {prec} pool={pool}")
    assert float(model.pos_embed.grad.abs().max()) > 0 and float(model.cls_token.grad.abs().max()) > 0
    # evaluation never drops: the float64 model with every scale at 1
    model.eval()
    with torch.no_grad():
        again = model(imgs)
    ones = torch.ones(3, 2, B)
    assert rel(again, _float64(model, imgs, target, pool, ones, "ones")[0]) < MODEL_TOL[prec][0]
    assert torch.equal(model.last_drop_scales, table), "an evaluation forward must not replace the training table"


@pytest.mark.parametrize("pool", [True, False], ids=["global_pool", "cls_token"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_model_with_a_supplied_table_of_arbitrary_scales(pool, prec):
    """Scales distinct per sample, block and branch (block 0 included: a supplied table runs every block with it)."""
    model = _model(pool, prec)
    imgs, target = _batch(41)
    table = R.arbitrary_table(3, B).to(DEV)
    from ssl4polyp_amd import _lib
    off = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
    logits = model(imgs, drop_scales=table)
    assert torch.cuda.default_generators[torch.cuda.current_device()].get_offset() == off, "a supplied table draws nothing"
    _loss(logits, target).backward()
    assert model.last_drop_scales is table
    want_logits, want = _float64(model, imgs, target, pool, table, "arbitrary")
    _compare(model, logits, want_logits, want, prec, f"arbitrary table {prec} pool={pool}")
    with pytest.raises(_lib.PolypMaeError, match="drop_scales"):
        model(imgs, drop_scales=table[:, :, :4].contiguous())
    model.eval()
    with pytest.raises(_lib.PolypMaeError, match="training mode"):
        model(imgs, drop_scales=table)


def test_frozen_lower_blocks():
    """Blocks 0 and 1 (and the front) frozen: the trainable part gets the float64 gradients, the frozen part none."""
    model = _model(True, "fp32")
    trainable = lambda n: n.startswith(("blocks.2.", "fc_norm.", "head."))
    for n, p in model.named_parameters():
        p.requires_grad_(trainable(n))
    imgs, target = _batch(41)
    torch.manual_seed(R.MODEL_SEED)
    logits = model(imgs)
    _loss(logits, target).backward()
    assert torch.equal(model.last_drop_scales.cpu(), _host_table())
    want_logits, want = _float64(model, imgs, target, True, model.last_drop_scales, "drawn")
    _compare(model, logits, want_logits, want, "fp32", "frozen blocks 0-1", only=trainable)
    # and with block 1 alone frozen, under the arbitrary table: the dgrad chain runs through a frozen block's scaled branches
    model = _model(True, "fp32")
    trainable = lambda n: n.startswith(("blocks.0.", "blocks.2.", "fc_norm.", "head."))
    for n, p in model.named_parameters():
        p.requires_grad_(trainable(n))
    table = R.arbitrary_table(3, B).to(DEV)
    logits = model(imgs, drop_scales=table)
    _loss(logits, target).backward()
    want_logits, want = _float64(model, imgs, target, True, table, "arbitrary")
    _compare(model, logits, want_logits, want, "fp32", "block 1 frozen between trainable ones", only=trainable)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_micro_steps_accumulate(prec):
    """accum_iter = 2: each micro-step draws its own table; the accumulated gradients are the sum of the two single steps'."""
    model = _model(True, prec)
    batches = [_batch(41), _batch(42)]
    half = 0.5
    single, tables = [], []
    torch.manual_seed(R.MODEL_SEED)
    for x, y in batches:
        model.zero_grad(set_to_none=True)
        (_loss(model(x), y) * half).backward()
        single.append({n: p.grad.clone() for n, p in model.named_parameters()})
        tables.append(model.last_drop_scales.clone())
    assert torch.equal(tables[0].cpu(), _host_table()) and torch.equal(tables[1].cpu(), _host_table(R.drawn(3 * 2 * B)))
    model.zero_grad(set_to_none=True)
    torch.manual_seed(R.MODEL_SEED)
    (_loss(model(batches[0][0]), batches[0][1]) * half).backward()
    first = model.head.weight.grad
    (_loss(model(batches[1][0]), batches[1][1]) * half).backward()
    assert torch.equal(model.last_drop_scales, tables[1])
    assert model.head.weight.grad.data_ptr() == first.data_ptr(), "the second micro-step accumulates in place"
    for n, p in model.named_parameters():
        e = rel_l2(_without_key_bias(n, p.grad), _without_key_bias(n, single[0][n] + single[1][n]))
        assert e < MODEL_TOL[prec][1], ("accum", n, e)


@pytest.mark.parametrize("pool", [True, False], ids=["global_pool", "cls_token"])
def test_default_path_keeps_its_bits(pool):
    """eval() of a model built with a rate, and train() of a model built with rate 0.0: the bits of a model built without the
    argument (the same launches: nothing on that path may change)."""
    imgs, target = _batch(41)
    twin = _model(pool, "bf16", rate=_UNSET)
    twin.train()
    want = twin(imgs)
    _loss(want, target).backward()
    zero = _model(pool, "bf16", rate=0.0)
    zero.train()
    assert not zero.drop_path_active
    got = zero(imgs)
    _loss(got, target).backward()
    assert zero.last_drop_scales is None and torch.equal(got, want)
    for (n, p), (_, q) in zip(zero.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    dropped = _model(pool, "bf16")
    dropped.eval()
    twin.eval()
    with torch.no_grad():
        assert torch.equal(dropped(imgs), twin(imgs))
    assert dropped.last_drop_scales is None


def test_draw_follows_the_device_generator():
    model = _model(True, "fp32")
    imgs, _ = _batch(41)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    n = 3 * 2 * B
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        assert gen.get_offset() == 0
        with torch.no_grad():
            model(imgs)
            a = model.last_drop_scales.clone()
            assert gen.get_offset() == R.drawn(n)
            model(imgs)
            b = model.last_drop_scales.clone()
            assert gen.get_offset() == 2 * R.drawn(n)
        runs.append((a, b))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "re-seeding replays both tables"
    assert not torch.equal(runs[0][0], runs[0][1]), "consecutive forwards draw different tables"
    # a count that is no multiple of 4 advances the offset to the next one: B = 3 draws 18 numbers
    torch.manual_seed(77)
    with torch.no_grad():
        model(imgs[:3])
    assert model.last_drop_scales.shape == (3, 2, 3) and gen.get_offset() == 20 == R.drawn(18)
    assert np.array_equal(model.last_drop_scales.cpu().numpy(), R.scale_table(77, 0, model.drop_path_rates, 3))


def _three_steps(rate, seed):
    from ssl4polyp_amd.optim import FusedAdamW
    model = _model(True, "bf16", rate=rate)
    model.train()
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    torch.manual_seed(seed)
    losses = []
    for it in range(3):
        imgs, target = _batch(50 + it)
        opt.zero_grad(set_to_none=True)
        loss = _loss(model(imgs), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), {n: p.detach().clone() for n, p in model.named_parameters()}


def test_three_optimizer_steps():
    l1, p1 = _three_steps(R.MODEL_RATE, 9)
    l2, p2 = _three_steps(R.MODEL_RATE, 9)
    l0, p0 = _three_steps(0.0, 9)
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(l0).all())
    assert torch.equal(l1, l2) and all(torch.equal(p1[n], p2[n]) for n in p1), "two seeded runs differ"
    assert all(bool(torch.isfinite(v).all()) for v in p1.values())
    assert not torch.equal(p1["blocks.2.mlp.fc2.weight"], p0["blocks.2.mlp.fc2.weight"])
    assert not torch.equal(l1, l0)


def test_fp16_with_the_loss_scaler():
    from ssl4polyp_amd.optim import LossScaler
    model = _model(True, "fp16")
    imgs, target = _batch(41)
    sc = LossScaler(init_scale=1024.0)
    torch.manual_seed(R.MODEL_SEED)
    logits = model(imgs)
    sc.scale(_loss(logits, target)).backward()
    assert torch.equal(model.last_drop_scales.cpu(), _host_table())
    want_logits, want = _float64(model, imgs, target, True, model.last_drop_scales, "drawn")
    _compare(model, logits, want_logits, want, "fp16", "fp16 drawn table", scale=1024.0)
