"""The fine-tune kernels (csrc/pm_finetune.hip) and what is built on them, on the device: batch mixing against torch's own three-op
sequence / indexed copy bit for bit; soft-target cross-entropy, the trainable global_pool and the plain Linear head against the
float64 restatements and element-wise bounds of tests/finetune_ref.py (held to f32 emulations and to wrong variants by
tests/test_finetune_mae_cpu.py); the fine-tune model against a float64 model at the tolerances tests/test_gpu_models.py applies to
the tiny classifiers; FusedAdamW over the layer-decay groups against torch.optim.AdamW; main_finetune_mae end to end.  Outputs lie
between guard regions that are checked afterwards.  Each test prints its largest err / bound per output (`pytest -s`)."""
import ctypes
import functools
import json
import types

import numpy as np
import pytest
import torch

import finetune_ref as FR
import probe_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32
GUARD, FILL = 64, 12345.0
TRAJ_TOL = 2e-5   # tests/test_gpu_finetune_schedule.py: the suite's bound on optimiser trajectories (rel-L2)
# tests/test_gpu_models.py:42-47 TOL, as test_tiny_classifiers_vs_reference_fixture applies it: (logits max-rel, gradient rel-L2)
MODEL_TOL = {"fp32": (1e-4, 1e-3), "bf16": (7.5e-3, 1.5e-2)}


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
    """A tensor that is a slice of a larger buffer: GUARD elements of FILL in front and behind (16-byte aligned); NaN-filled (floats)
    or -1 (integers) unless `init` is given."""
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if init is not None:
        view.copy_(init)
    else:
        view.fill_(float("nan") if dtype.is_floating_point else -1)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_hold(buf, what):
    assert bool((buf[:GUARD] == FILL).all()), what + ": written in front of the buffer"
    assert bool((buf[-GUARD:] == FILL).all()), what + ": written behind the buffer"


def _report(r, what):
    for k, v in r.items():
        print(f"{what} {k}: err/bound {v:.3f}")
    for k, v in r.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of its bound"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _record(lam, use_cutmix=False, box=(0, 0, 0, 0)):
    """The device record of one draw, written the way the training loop writes it."""
    from ssl4polyp_amd.mixup import MixState
    st = MixState(torch.device(DEV, torch.cuda.current_device()))
    st.write(lam, use_cutmix, box)
    return st


# ---------------------------------------------------------------------------------------------------- batch mixing
MIX_SHAPES = [(2, 16, 16), (4, 224, 224), (6, 30, 18)]
LAM_INEXACT = 0.9871234567891234   # not an f32 value, and f32(1 - lam) != 1.f - f32(lam)


@functools.lru_cache(maxsize=None)
def _mix_input(shape):
    B, H, W = shape
    x = torch.randn(B, 3, H, W, generator=_gen(B + H + W))
    x[0, 0, 0, :4] = 0.0   # (a zero against a non-zero partner: where a wrong 1 - lam shows)
    return x.to(DEV)


@pytest.mark.parametrize("shape", MIX_SHAPES)
@pytest.mark.parametrize("lam", [0.3, 0.0, LAM_INEXACT])
def test_mixup_equals_torch_bit_for_bit(shape, lam):
    B, H, W = shape
    x0 = _mix_input(shape)
    buf, x = _guarded((B, 3, H, W), init=x0)
    st = _record(lam)
    assert abi("pm_mix_batch", x, B, 3, H, W, st.record, 1) == 0
    want = x0.clone()
    flipped = want.flip(0).mul_(1.0 - lam)   # timm Mixup._mix_batch
    want.mul_(lam).add_(flipped)
    torch.cuda.synchronize()
    _guards_hold(buf, f"mixup {shape}")
    assert torch.equal(x, want), f"mixup {shape} lam {lam}: {(x != want).sum().item()} elements differ"
    ref, e = FR.mixup(x0, *FR.record(lam))
    assert FR.ratio(x, ref, e) <= 1.0


def _boxes(H, W):
    return {"empty": (3, 3, 2, 9), "empty_x": (1, 5, 7, 7), "whole": (0, H, 0, W), "top_left": (0, H // 2, 0, W // 3),
            "bottom_right": (H // 2, H, W - 5, W), "left_edge": (2, H - 1, 0, 3), "right_edge": (1, 4, W - 3, W),
            "odd_xl": (1, H - 2, 3, 3 + 6), "odd_xl_odd_width": (0, H, 5, 5 + 7), "one_pixel": (H - 1, H, W - 1, W)}


@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_cutmix_equals_the_indexed_copy(shape):
    B, H, W = shape
    x0 = _mix_input(shape)
    for name, box in _boxes(H, W).items():
        yl, yh, xl, xh = box
        buf, x = _guarded((B, 3, H, W), init=x0)
        st = _record(0.5, True, box)   # (lam does not matter to the images: the box does)
        assert abi("pm_mix_batch", x, B, 3, H, W, st.record, 1) == 0
        want = x0.clone()
        want[:, :, yl:yh, xl:xh] = x0.flip(0)[:, :, yl:yh, xl:xh]   # timm: x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        torch.cuda.synchronize()
        _guards_hold(buf, f"cutmix {shape} {name}")
        assert torch.equal(x, want), f"cutmix {shape} {name}"
        outside = torch.ones(H, W, dtype=torch.bool, device=DEV)
        outside[yl:yh, xl:xh] = False
        assert torch.equal(x[:, :, outside].view(torch.int32), x0[:, :, outside].view(torch.int32)), f"{name}: bytes outside the box"
        if "empty" in name:
            assert torch.equal(x.view(torch.int32), x0.view(torch.int32))
    assert _boxes(H, W)["odd_xl"][2] % 2 == 1 and (_boxes(H, W)["odd_xl_odd_width"][3] - _boxes(H, W)["odd_xl_odd_width"][2]) % 4


def test_mix_refusals_and_the_identity_draw():
    from ssl4polyp_amd import _lib, mixup
    x0 = _mix_input((6, 30, 18))
    st = _record(0.3)
    buf, x = _guarded((5, 3, 30, 18), init=x0[:5])
    assert abi("pm_mix_batch", x, 5, 3, 30, 18, st.record, 1) == _lib.PM_ESHAPE   # timm asserts an even batch
    assert abi("pm_mix_batch", x, 4, 3, 30, 18, None, 1) == _lib.PM_EINVAL
    assert abi("pm_mix_batch", x, 4, 3, 30, 18, st.record, 0) == 0                # the host's identity draw: no launch
    ident = _record(1.0)
    assert abi("pm_mix_batch", x, 4, 3, 30, 18, ident.record, 1) == 0             # the device's identity draw: nothing written
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), x0[:5].view(torch.int32))
    with pytest.raises(ValueError):
        mixup.mix_batch(x0[:5].contiguous(), st)
    # the record's two weights are each rounded from the double
    words = mixup.MixState.pack(LAM_INEXACT, False, (0, 0, 0, 0))
    lam32, oml32 = np.frombuffer(words.tobytes(), dtype=np.float32)[:2]
    assert (float(lam32), float(oml32)) == FR.record(LAM_INEXACT) and np.float32(1.0) - lam32 != oml32


# ---------------------------------------------------------------------------------------------------- soft-target cross-entropy
CE_SHAPES = [(2, 1), (2, 2), (4, 5), (66, 7), (64, 1000), (2, 1000)]


@functools.lru_cache(maxsize=None)
def _ce_case(shape):
    """Logits with a last class whose bias is -40 (a target all the same), and one planted same-class pair (rows 0 and B - 1)."""
    B, C = shape
    g = _gen(B * 31 + C)
    logits = torch.randn(B, C, generator=g) * 2.0
    target = torch.randint(0, C, (B,), generator=g)
    if C >= 2:
        logits[:, C - 1] -= 40.0
        target[1] = C - 1
    target[B - 1] = target[0]
    return logits.to(DEV), target.to(DEV)


def _soft_ce(logits, target, rec, smoothing, scale, grad=True):
    from ssl4polyp_amd import _lib
    B, C = logits.shape
    size = ctypes.c_size_t(0)
    assert _lib.load().pm_soft_ce_workspace(B, ctypes.byref(size)) == 0 and size.value == 4 * B
    bufs = {"loss": _guarded((1,)), "dlogits": _guarded((B, C)), "ws": _guarded((B,))}
    o = {n: v for n, (_, v) in bufs.items()}
    st = abi("pm_soft_ce", logits, target, B, C, rec, float(smoothing), scale, o["loss"], o["dlogits"] if grad else None, o["ws"], 4 * B)
    torch.cuda.synchronize()
    for n, (buf, _) in bufs.items():
        _guards_hold(buf, f"soft_ce {n}")
    return st, o


@pytest.mark.parametrize("shape", CE_SHAPES)
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("lam", [1.0, 0.0, 0.3])
def test_soft_ce(shape, smoothing, lam):
    B, C = shape
    logits, target = _ce_case(shape)
    assert int(target[0]) == int(target[B - 1])
    st = _record(lam)
    scale = torch.tensor(0.5, device=DEV)
    status, o = _soft_ce(logits, target, st.record, smoothing, scale)
    assert status == 0
    ref = FR.soft_ce(logits, target, *FR.record(lam), smoothing, 0.5)
    what = f"soft_ce {shape} s {smoothing} lam {lam}"
    r = {"loss": FR.ratio(o["loss"][0], ref["loss"], ref["e_loss"]), "dlogits": FR.ratio(o["dlogits"], ref["dlogits"], ref["e_dlogits"])}
    # the planted pair: the two weights of its class add up (an else-if chain over the two classes would lose one of them)
    t = FR.soft_targets(target, C, *FR.record(lam), smoothing)
    on, off = FR.on_off(smoothing, C)
    lam32, oml32 = FR.record(lam)
    assert abs(float(t[0, int(target[0])]) - (lam32 + oml32) * on) < 1e-12
    # `scale` is honoured: twice the scale, twice the gradient (a power of two: exactly), the same loss
    _, o2 = _soft_ce(logits, target, st.record, smoothing, torch.tensor(1.0, device=DEV))
    assert torch.equal(o2["dlogits"], o["dlogits"] * 2) and torch.equal(o2["loss"], o["loss"])
    # without a gradient: the same loss, dlogits untouched
    _, o3 = _soft_ce(logits, target, st.record, smoothing, None, grad=False)
    assert torch.equal(o3["loss"], o["loss"]) and bool(torch.isnan(o3["dlogits"]).all())
    if lam == 1.0:   # a NULL record is lam = 1
        _, o4 = _soft_ce(logits, target, None, smoothing, scale)
        assert torch.equal(o4["loss"], o["loss"]) and torch.equal(o4["dlogits"], o["dlogits"])
        if smoothing == 0.0:   # plain cross-entropy: within the bound of pm_probe_ce's restatement too
            c = P.ce(logits, target, 0.5)
            r["loss vs probe_ref.ce"] = P.ratio(o["loss"][0], c["loss"], c["e_loss"])
            r["dlogits vs probe_ref.ce"] = P.ratio(o["dlogits"], c["dlogits"], c["e_dlogits"])
    _report(r, what)


def test_soft_ce_out_of_range_target_and_refusals():
    from ssl4polyp_amd import _lib
    logits, target = _ce_case((4, 5))
    st = _record(0.3)
    scale = torch.tensor(1.0, device=DEV)
    for bad in (5, -1):
        t = target.clone()
        t[2] = bad
        status, o = _soft_ce(logits, t, st.record, 0.1, scale)
        assert status == 0 and bool(torch.isnan(o["loss"]).all())
        # row 2 holds the bad target, row 1 = B - 1 - 2 mixes with it: both get a zero row; the others their usual gradient
        assert bool((o["dlogits"][2] == 0).all()) and bool((o["dlogits"][1] == 0).all())
        ref = FR.soft_ce(logits, target, *FR.record(0.3), 0.1, 1.0)
        assert FR.ratio(o["dlogits"][[0, 3]], ref["dlogits"][[0, 3]], ref["e_dlogits"][[0, 3]]) <= 1.0
    lb, loss = _guarded((1,))
    db, dl = _guarded((4, 5))
    wb, ws = _guarded((4,))
    assert abi("pm_soft_ce", logits, target, 4, 5, st.record, 0.1, scale, loss, dl, ws, 12) == _lib.PM_EINVAL      # short workspace
    assert abi("pm_soft_ce", logits, target, 4, 5, st.record, 0.1, None, loss, dl, ws, 16) == _lib.PM_EINVAL       # gradient, no scale
    assert abi("pm_soft_ce", logits, target, 4, 0, st.record, 0.1, scale, loss, dl, ws, 16) == _lib.PM_ESHAPE
    assert abi("pm_soft_ce", logits, target, 70000, 5, st.record, 0.1, scale, loss, dl, ws, 280000) == _lib.PM_ESHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all())


def test_soft_target_ce_op_carries_the_upstream_factor():
    """The autograd op: loss.backward() leaves dlogits x scale; through a loss scale of 1024 exactly 1024 times that."""
    from ssl4polyp_amd.mixup import soft_target_ce
    logits, target = _ce_case((4, 5))
    st = _record(0.3)
    scale = torch.tensor(0.5, device=DEV)
    a = logits.clone().requires_grad_(True)
    loss = soft_target_ce(a, target, st, 0.1, scale)
    loss.backward()
    ref = FR.soft_ce(logits, target, *FR.record(0.3), 0.1, 0.5)
    assert FR.ratio(loss.detach(), ref["loss"], ref["e_loss"]) <= 1.0 and FR.ratio(a.grad, ref["dlogits"], ref["e_dlogits"]) <= 1.0
    b = logits.clone().requires_grad_(True)
    (soft_target_ce(b, target, st, 0.1, scale) * 1024.0).backward()
    assert torch.equal(b.grad, a.grad * 1024.0)


# ---------------------------------------------------------------------------------------------------- global_pool, training
POOL = [(2, 197, 768), (3, 50, 768), (2, 257, 1280), (1, 2, 64)]


@functools.lru_cache(maxsize=None)
def _pool_case(case):
    B, N, D = case
    g = _gen(N + D)
    x = torch.randn(B, N, D, generator=g) * 2.0 + 0.5
    x[:, 0] = 1e4 * torch.randn(B, D, generator=g)   # the cls row: excluded from the mean
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dfeat = torch.randn(B, D, generator=g)
    return tuple(t.to(DEV) for t in (x, gamma, beta, dfeat))


def _pool_forward(case):
    from ssl4polyp_amd import _lib
    B, N, D = case
    x, gamma, beta, _ = _pool_case(case)
    size = ctypes.c_size_t(0)
    assert _lib.load().pm_pool_norm_workspace(B, N, D, ctypes.byref(size)) == 0
    bufs = {"ws": _guarded((size.value // 4,)), "feat": _guarded((B, D)), "pooled": _guarded((B, D)), "mean": _guarded((B,)),
            "rstd": _guarded((B,))}
    o = {n: v for n, (_, v) in bufs.items()}
    st = abi("pm_pool_norm_fwd_train", x, B, N, D, gamma, beta, 1e-6, o["feat"], o["pooled"], o["mean"], o["rstd"], o["ws"], size.value)
    torch.cuda.synchronize()
    for n, (buf, _) in bufs.items():
        _guards_hold(buf, f"pool forward {case} {n}")
    return st, o, size.value


@pytest.mark.parametrize("case", POOL)
def test_pool_train_forward(case):
    B, N, D = case
    x, gamma, beta, _ = _pool_case(case)
    st, o, nbytes = _pool_forward(case)
    assert st == 0
    fb, feat = _guarded((B, D))
    ws = torch.empty(nbytes // 4, device=DEV)
    assert abi("pm_pool_norm_fwd", x, B, N, D, gamma, beta, 1e-6, feat, ws, nbytes) == 0
    torch.cuda.synchronize()
    assert torch.equal(o["feat"].view(torch.int32), feat.view(torch.int32)), "feat must have the bits of pm_pool_norm_fwd"
    ref = FR.pool_fwd(x, gamma, beta)
    _report({"feat": FR.ratio(o["feat"], ref["feat"], ref["e_feat"]), "pooled": FR.ratio(o["pooled"], ref["pooled"], ref["e_pooled"]),
             "mean": FR.ratio(o["mean"], ref["mean"], ref["e_mean"]), "rstd": FR.ratio(o["rstd"], ref["rstd"], ref["e_rstd"])},
            f"pool forward {case}")


@pytest.mark.parametrize("case", POOL)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_pool_backward(case, prec):
    from ssl4polyp_amd import _lib
    B, N, D = case
    x, gamma, beta, dfeat = _pool_case(case)
    st, f, _ = _pool_forward(case)
    assert st == 0
    act = FR.R.DTYPES[prec]
    size = ctypes.c_size_t(0)
    assert _lib.load().pm_pool_norm_bwd_workspace(B, N, D, ctypes.byref(size)) == 0 and size.value == 4 * B * D
    prior_g, prior_b = (torch.randn(D, generator=_gen(8)) * 0.3).to(DEV), (torch.randn(D, generator=_gen(9)) * 0.3).to(DEV)
    what = f"pool backward {case} {prec}"

    def run(dgamma0, dbeta0, want_params=True):
        bufs = {"dx": _guarded((B, N, D)), "dx_act": _guarded((B, N, D), act), "dgamma": _guarded((D,), init=dgamma0),
                "dbeta": _guarded((D,), init=dbeta0), "ws": _guarded((B * D,))}
        o = {n: v for n, (_, v) in bufs.items()}
        status = abi("pm_pool_norm_bwd", dfeat, f["pooled"], f["mean"], f["rstd"], gamma, B, N, D, o["dx"], o["dx_act"],
                     _lib.dtype_code(act), o["dgamma"] if want_params else None, o["dbeta"] if want_params else None, o["ws"], size.value)
        torch.cuda.synchronize()
        for n, (buf, _) in bufs.items():
            _guards_hold(buf, f"{what} {n}")
        return status, o

    zeros = torch.zeros(D, device=DEV)
    status, o = run(zeros, zeros)
    assert status == 0
    ref = FR.pool_bwd(dfeat, f["pooled"], f["mean"], f["rstd"], gamma, N)
    dx = o["dx"]
    assert bool((dx[:, 0] == 0).all()), "the cls row does not reach the pooled feature"
    assert bool((dx[:, 1:].view(torch.int32) == dx[:, 1:2].view(torch.int32)).all()), "every patch row of a sample holds the same bits"
    assert torch.equal(o["dx_act"], dx.to(act)), "dx_act is the round-to-nearest-even copy of dx"
    r = {"dx": FR.ratio(dx, ref["dx"], ref["e_dx"]),
         "dgamma": FR.ratio(o["dgamma"], ref["dgamma"], FR.sum_bound(ref["n_dgamma"], ref["t_dgamma"])),
         "dbeta": FR.ratio(o["dbeta"], ref["dbeta"], FR.sum_bound(ref["n_dbeta"], ref["t_dbeta"]))}
    # into pre-filled buffers: one addition into what they held
    status, o2 = run(prior_g, prior_b)
    assert status == 0 and torch.equal(o2["dx"], dx)
    ref2 = FR.pool_bwd(dfeat, f["pooled"], f["mean"], f["rstd"], gamma, N, prior={"dgamma": prior_g, "dbeta": prior_b})
    r["dgamma into prior"] = FR.ratio(o2["dgamma"], ref2["dgamma"], FR.sum_bound(ref2["n_dgamma"] + 1, ref2["t_dgamma"]))
    r["dbeta into prior"] = FR.ratio(o2["dbeta"], ref2["dbeta"], FR.sum_bound(ref2["n_dbeta"] + 1, ref2["t_dbeta"]))
    # frozen fc_norm: NULL leaves nothing written
    status, o3 = run(prior_g, prior_b, want_params=False)
    assert status == 0 and torch.equal(o3["dgamma"], prior_g) and torch.equal(o3["dbeta"], prior_b) and torch.equal(o3["dx"], dx)
    _report(r, what)


def test_pool_refusals():
    from ssl4polyp_amd import _lib
    case = (2, 197, 768)
    B, N, D = case
    x, gamma, beta, dfeat = _pool_case(case)
    st, f, nbytes = _pool_forward(case)
    fb, feat = _guarded((B, D))
    pb, pooled = _guarded((B, D))
    m, r = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    ws = torch.empty(nbytes // 4, device=DEV)
    assert abi("pm_pool_norm_fwd_train", x, B, 1, D, gamma, beta, 1e-6, feat, pooled, m, r, ws, nbytes) == _lib.PM_ESHAPE
    assert abi("pm_pool_norm_fwd_train", x, B, N, D, gamma, beta, 1e-6, feat, pooled, m, r, ws, nbytes - 4) == _lib.PM_EINVAL
    assert abi("pm_pool_norm_fwd_train", x, B, N, 2052, gamma, beta, 1e-6, feat, pooled, m, r, ws, nbytes) == _lib.PM_ESHAPE
    db, dx = _guarded((B, N, D))
    ws2 = torch.empty(B * D, device=DEV)
    args = (dfeat, f["pooled"], f["mean"], f["rstd"], gamma)
    assert abi("pm_pool_norm_bwd", *args, B, 1, D, dx, None, 0, None, None, ws2, 4 * B * D) == _lib.PM_ESHAPE
    assert abi("pm_pool_norm_bwd", *args, B, N, D, dx, None, 0, None, None, ws2, 4 * B * D - 4) == _lib.PM_EINVAL
    assert abi("pm_pool_norm_bwd", *args, B, N, D, None, dx, 0, None, None, ws2, 4 * B * D) == _lib.PM_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(feat).all()) and bool(torch.isnan(pooled).all()) and bool(torch.isnan(dx).all())
    _guards_hold(db, "refused pool backward")


# ---------------------------------------------------------------------------------------------------- the plain Linear head
HEAD = [(2, 64, 1), (2, 64, 2), (3, 64, 5), (3, 768, 7), (64, 64, 2), (64, 768, 1000), (65, 64, 7), (65, 768, 2), (64, 1280, 5),
        (65, 1280, 1000), (3, 1280, 2), (2, 768, 1000)]   # tests/test_gpu_linprobe.py HEAD


@pytest.mark.parametrize("case", HEAD)
def test_linear_head(case):
    B, D, C = case
    g = _gen(B * 7 + D + C)
    feat = (torch.randn(B, D, generator=g) * 1.5 + 0.3).to(DEV)
    W = (torch.randn(C, D, generator=g) * (1.0 / D ** 0.5)).to(DEV)
    bias = (torch.randn(C, generator=g) * 0.1).to(DEV)
    dlogits = (torch.randn(B, C, generator=g) * 0.1).to(DEV)
    what = f"linear head {case}"
    lb, logits = _guarded((B, C))
    fb, dfeat = _guarded((B, D))
    assert abi("pm_linear_head_fwd", feat, B, D, C, W, bias, logits) == 0
    assert abi("pm_linear_head_dfeat", dlogits, W, B, D, C, dfeat) == 0
    prior_w, prior_b = (torch.randn(C, D, generator=_gen(5)) * 0.01).to(DEV), (torch.randn(C, generator=_gen(6)) * 0.01).to(DEV)
    gwb, gw = _guarded((C, D), init=prior_w)
    gbb, gb = _guarded((C,), init=prior_b)
    assert abi("pm_probe_head_bwd", dlogits, feat, B, D, C, gw, gb) == 0   # dW / dbias of this head: the probe's kernel, unchanged
    torch.cuda.synchronize()
    for buf, n in ((lb, "logits"), (fb, "dfeat"), (gwb, "dW"), (gbb, "dbias")):
        _guards_hold(buf, f"{what} {n}")
    want, e = FR.linear(feat, W, bias)
    want_d, e_d = FR.dfeat(dlogits, W)
    b = P.head_bwd(dlogits, feat, prior_w, prior_b)
    _report({"logits": FR.ratio(logits, want, e), "dfeat": FR.ratio(dfeat, want_d, e_d),
             "dW": P.ratio(gw, b["dW"], P.sum_bound(b["n"], b["t_dW"])), "dbias": P.ratio(gb, b["dbias"], P.sum_bound(b["n"], b["t_dbias"]))},
            what)


@pytest.mark.parametrize("case", [(2, 64, 1), (3, 768, 7), (2, 64, 81)])
def test_linear_head_has_the_bits_of_the_probe_head(case):
    """pm_probe_head_fwd and pm_linear_head_fwd launch one linear_kernel (csrc/pm_pool_head.h): on the xhat the probe's BatchNorm
    left, the plain head gives the probe's logits bit for bit.  One class and one k-step; three k-steps and a partial 16-class group;
    a second 64-class strip whose second wave is partial."""
    B, D, C = case
    g = _gen(B * 11 + D + C)
    feat = (torch.randn(B, D, generator=g) * 1.5 + 0.3).to(DEV)
    W = (torch.randn(C, D, generator=g) * (1.0 / D ** 0.5)).to(DEV)
    bias = (torch.randn(C, generator=g) * 0.1).to(DEV)
    rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    bufs = {"xhat": _guarded((B, D)), "probe logits": _guarded((B, C)), "linear logits": _guarded((B, C))}
    o = {n: v for n, (_, v) in bufs.items()}
    assert abi("pm_probe_head_fwd", feat, B, D, C, W, bias, rm, rv, nbt, 1, 0.1, 1e-6, o["xhat"], o["probe logits"]) == 0
    assert abi("pm_linear_head_fwd", o["xhat"], B, D, C, W, bias, o["linear logits"]) == 0
    torch.cuda.synchronize()
    for n, (buf, _) in bufs.items():
        _guards_hold(buf, f"shared linear kernel {case} {n}")
    assert not bool(torch.isnan(o["probe logits"]).any())
    assert torch.equal(o["probe logits"].view(torch.int32), o["linear logits"].view(torch.int32))


def test_linear_head_refusals():
    from ssl4polyp_amd import _lib
    feat, W, bias = torch.randn(2, 64, device=DEV), torch.randn(3, 64, device=DEV), torch.randn(3, device=DEV)
    lb, logits = _guarded((2, 3))
    assert abi("pm_linear_head_fwd", feat, 2, 62, 3, W, bias, logits) == _lib.PM_ESHAPE
    assert abi("pm_linear_head_fwd", feat, 2, 64, 65536, W, bias, logits) == _lib.PM_ESHAPE
    assert abi("pm_linear_head_fwd", feat, 2, 64, 3, None, bias, logits) == _lib.PM_EINVAL
    assert abi("pm_linear_head_dfeat", logits, W, 2, 64, 0, feat) == _lib.PM_ESHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(logits).all())


# ---------------------------------------------------------------------------------------------------- the model
TINY = dict(embed_dim=64, depth=2, num_heads=2)
LAM_MODEL, SMOOTHING = 0.3, 0.1


def _tiny_model(pool, prec, C=5, seed=11):
    """The tiny fine-tune model with every parameter away from its initial value (head, fc_norm and the biases start at 0 / 1)."""
    from ssl4polyp_amd import models_vit
    torch.manual_seed(seed)
    model = models_vit.VisionTransformer(num_classes=C, global_pool=pool, precision=prec, **TINY)
    g = _gen(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n == "head.weight":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif p.ndim == 1:
                p.add_(torch.randn(p.shape, generator=g) * (0.1 if n.endswith("weight") else 0.02))
    return model.to(DEV)


def _batch(B, C, seed, mix=True):
    """Images (mixed on the device with lam = 0.3 when `mix`), labels with a same-class pair, the draw's state."""
    g = _gen(seed)
    imgs = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    target = torch.randint(0, C, (B,), generator=g)
    target[B - 1] = target[0]
    st = _record(LAM_MODEL if mix else 1.0)
    if mix:
        from ssl4polyp_amd.mixup import mix_batch
        mix_batch(imgs, st)
    return imgs, target.to(DEV), st


def _float64_grads(model, imgs, target, pool, lam, cfg, blocks_on=None):
    """Logits and every parameter gradient of finetune_ref's float64 model on the model's own weights."""
    leaves = {}
    for n, v in model.state_dict().items():
        dev = "cpu" if (blocks_on is None or n.startswith("patch_embed.")) else blocks_on
        leaves[n] = v.detach().double().to(dev).requires_grad_(True)
    logits = FR.vit_finetune_logits(leaves, imgs.detach().double().cpu(), cfg, pool)
    FR.soft_ce_autograd(logits, target.to(logits.device), *FR.record(lam), SMOOTHING).backward()
    return logits.detach(), {n: v.grad for n, v in leaves.items()}


def _without_key_bias(n, g):
    """attn.qkv.bias: the key part has a zero gradient (softmax is invariant to it), pure round-off: tests/test_gpu_models.py:133."""
    if n.endswith("attn.qkv.bias"):
        D = g.numel() // 3
        return torch.cat([g[:D], g[2 * D:]])
    return g


@pytest.mark.parametrize("pool", [True, False], ids=["global_pool", "cls_token"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiny_finetune_model_against_float64(pool, prec):
    from oracle import vit_mae_ref as O
    from ssl4polyp_amd.mixup import soft_target_ce
    tl, tg = MODEL_TOL[prec]
    cfg = O.ViTConfig(img_size=224, patch_size=16, **TINY)
    model = _tiny_model(pool, prec)
    imgs, target, st = _batch(4, 5, 21)
    model.train()
    logits = model(imgs)
    loss = soft_target_ce(logits, target, st, SMOOTHING)
    loss.backward()
    want_logits, want = _float64_grads(model, imgs, target, pool, LAM_MODEL, cfg)
    print(f"tiny {prec} pool={pool}: logits max-rel {rel(logits, want_logits):.2e}")
    assert logits.shape == (4, 5) and rel(logits, want_logits) < tl
    worst = 0.0
    for n, p in model.named_parameters():
        assert p.grad is not None, n + " got no gradient"
        e = rel_l2(_without_key_bias(n, p.grad), _without_key_bias(n, want[n]))
        worst = max(worst, e)
        assert e < tg, (n, e)
    print(f"tiny {prec} pool={pool}: worst gradient rel-L2 {worst:.2e}")
    assert float(model.pos_embed.grad.abs().max()) > 0 and float(model.cls_token.grad.abs().max()) > 0
    # two micro-steps with accum_iter = 2 = the sum of the two micro-batches' gradients at scale 1 / 2
    half = torch.tensor(0.5, device=DEV)
    imgs2, target2, st2 = _batch(4, 5, 22)
    single = []
    for x, y, s in ((imgs, target, st), (imgs2, target2, st2)):
        model.zero_grad(set_to_none=True)
        soft_target_ce(model(x), y, s, SMOOTHING, half).backward()
        single.append({n: p.grad.clone() for n, p in model.named_parameters()})
    model.zero_grad(set_to_none=True)
    soft_target_ce(model(imgs), target, st, SMOOTHING, half).backward()
    first = model.head.weight.grad
    soft_target_ce(model(imgs2), target2, st2, SMOOTHING, half).backward()
    assert model.head.weight.grad.data_ptr() == first.data_ptr(), "the second micro-step accumulates in place"
    for n, p in model.named_parameters():
        e = rel_l2(_without_key_bias(n, p.grad), _without_key_bias(n, single[0][n] + single[1][n]))
        assert e < tg, ("accum", n, e)
    # evaluation: no graph, the same logits
    model.eval()
    with torch.no_grad():
        again = model(imgs)
    assert not again.requires_grad and rel(again, want_logits) < tl


def test_frozen_encoder_trains_the_head_and_the_final_norm_only():
    """Everything under fc_norm frozen: the stack runs forward-only, head and fc_norm get the float64 gradients, nothing else one."""
    from oracle import vit_mae_ref as O
    from ssl4polyp_amd.mixup import soft_target_ce
    cfg = O.ViTConfig(img_size=224, patch_size=16, **TINY)
    for pool in (True, False):
        model = _tiny_model(pool, "fp32")
        for n, p in model.named_parameters():
            p.requires_grad_(n.startswith(("head.", "fc_norm.", "norm.")))
        imgs, target, st = _batch(4, 5, 23)
        soft_target_ce(model(imgs), target, st, SMOOTHING).backward()
        _, want = _float64_grads(model, imgs, target, pool, LAM_MODEL, cfg)
        for n, p in model.named_parameters():
            if p.requires_grad:
                assert rel_l2(p.grad, want[n]) < MODEL_TOL["fp32"][1], n
            else:
                assert p.grad is None, n


def test_vitb_global_pool_against_float64():
    """ViT-B/16, B = 8, global_pool, fp32 mode: the float64 model's blocks run on the device (the patch convolution on the host)."""
    from oracle import vit_mae_ref as O
    from ssl4polyp_amd import models_vit
    from ssl4polyp_amd.mixup import soft_target_ce
    tl, tg = MODEL_TOL["fp32"]
    torch.manual_seed(5)
    model = models_vit.vit_base_patch16(num_classes=10, global_pool=True, precision="fp32")
    with torch.no_grad():
        model.head.weight.normal_(0.0, 0.05, generator=_gen(6))
        model.fc_norm.weight.normal_(1.0, 0.1, generator=_gen(7))
        model.fc_norm.bias.normal_(0.0, 0.05, generator=_gen(8))
    model.to(DEV).train()
    imgs, target, st = _batch(8, 10, 24)
    logits = model(imgs)
    soft_target_ce(logits, target, st, SMOOTHING).backward()
    want_logits, want = _float64_grads(model, imgs, target, True, LAM_MODEL, O.VIT_BASE, blocks_on=DEV)
    assert rel(logits, want_logits) < tl
    params = dict(model.named_parameters())
    for n in ("fc_norm.weight", "head.weight", "blocks.0.mlp.fc1.weight"):
        e = rel_l2(params[n].grad, want[n])
        print(f"vit-b {n}: gradient rel-L2 {e:.2e}")
        assert e < tg, (n, e)


def test_probe_path_is_untouched():
    """A ProbeHead model's forward gives the bits of head(forward_features(x)), as before; a head that is neither is refused."""
    from ssl4polyp_amd import _lib, models_vit
    for pool in (True, False):
        model = models_vit.add_probe_head(_tiny_model(pool, "bf16")).to(DEV).eval()
        imgs = torch.randn(4, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        with torch.no_grad():
            assert torch.equal(model(imgs), model.head(model.forward_features(imgs)))
    model.head = torch.nn.Identity()
    with pytest.raises(_lib.PolypMaeError):
        model(imgs)


def test_cls_token_path_keeps_its_width_limit():
    """ViT-H width with the cls token: pm_vit_head_fwd's D <= 1024 refusal surfaces as it is; global_pool runs at that width."""
    from ssl4polyp_amd import _lib, models_vit
    imgs = torch.randn(2, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    wide = dict(embed_dim=1280, depth=1, num_heads=16, num_classes=3, precision="bf16")
    with pytest.raises(_lib.PolypMaeError, match="pm_vit_head_fwd"):
        models_vit.VisionTransformer(global_pool=False, **wide).to(DEV)(imgs)
    model = models_vit.VisionTransformer(global_pool=True, **wide).to(DEV)
    out = model(imgs)
    out.sum().backward()
    assert out.shape == (2, 3) and model.pos_embed.grad is not None and bool(torch.isfinite(model.fc_norm.weight.grad).all())


# ---------------------------------------------------------------------------------------------------- optimiser
def test_fused_adamw_over_layer_decay_groups_follows_torch():
    """Five steps of mix -> forward -> soft CE -> backward with the lr adjusted across a warm-up boundary: FusedAdamW over
    param_groups_lrd against torch.optim.AdamW over the same groups, fed the device's gradients."""
    from ssl4polyp_amd.lr_decay import param_groups_lrd
    from ssl4polyp_amd.mixup import Mixup, soft_target_ce
    from ssl4polyp_amd.optim import FusedAdamW
    from ssl4polyp_amd.train import adjust_learning_rate
    model = _tiny_model(True, "fp32")
    model._rt.ensure(torch.device(DEV, torch.cuda.current_device()))
    groups = param_groups_lrd(model, 0.05, model.no_weight_decay(), 0.75, with_names=True)
    assert len(groups) == 8   # 4 layer ids x (decay, no_decay)
    opt = FusedAdamW(model, groups, lr=1e-3)
    named = dict(model.named_parameters())
    twin = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named.items()}
    ref = torch.optim.AdamW([{"params": [twin[n] for n in g["param_names"]], "lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"]}
                             for g in groups], lr=1e-3)
    args = types.SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=1, epochs=3)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=5, rng=np.random.RandomState(2))
    start = {n: p.detach().clone() for n, p in named.items()}
    worst = 0.0
    for it in range(5):
        epoch = it / 2.0   # two iterations per epoch: 0, 0.5 | 1.0 (the warm-up's end), 1.5 | 2.0
        for o in (opt, ref):
            lr = adjust_learning_rate(o, epoch, args)
        assert [g["lr"] for g in opt.param_groups] == [lr * g["lr_scale"] for g in groups] == [g["lr"] for g in ref.param_groups]
        assert opt.param_groups[0]["lr"] == lr * 0.75 ** 3 and opt.param_groups[-1]["lr"] == lr
        imgs, target, _ = _batch(4, 5, 30 + it, mix=False)
        imgs, target = mix(imgs, target)
        opt.zero_grad(set_to_none=True)
        soft_target_ce(model(imgs), target, mix.state, 0.1).backward()
        for n, p in named.items():
            twin[n].grad = p.grad.detach().clone()
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        for n, p in named.items():
            e = rel_l2(p, twin[n])
            worst = max(worst, e)
            assert e <= TRAJ_TOL, (it, n, e)
        if it == 0:   # the warm-up starts at lr 0: nothing moves
            assert all(torch.equal(p, start[n]) for n, p in named.items())
    print(f"layer-decay AdamW: worst parameter rel-L2 over 5 steps {worst:.2e}")
    assert not torch.equal(named["blocks.0.mlp.fc1.weight"], start["blocks.0.mlp.fc1.weight"])


# ---------------------------------------------------------------------------------------------------- end to end
class _Batches:
    """A loader of fixed device batches (the same every epoch)."""

    def __init__(self, n, B, C, seed):
        g = _gen(seed)
        self.items = [(torch.randn(B, 3, 224, 224, generator=g).to(DEV), torch.randint(0, C, (B,), generator=g).to(DEV)) for _ in range(n)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def test_main_finetune_mae_end_to_end(tmp_path, monkeypatch):
    """Tiny model, 2 epochs of 4 micro-batches, mixup 0.8 + cutmix 1.0 + smoothing 0.1, accum_iter 2, clip_grad 1.0: finite losses, the
    reference's log and checkpoint keys; a run resumed after epoch 0 ends with the uninterrupted run's bits; --eval reproduces the
    logged accuracy; fp16 once; --drop_path 0.1 is refused."""
    from ssl4polyp_amd import main_finetune_mae, models_vit
    monkeypatch.setattr(models_vit, "vit_test_patch16", functools.partial(models_vit.VisionTransformer, **TINY), raising=False)
    train, val = _Batches(4, 4, 5, 40), _Batches(2, 4, 5, 41)
    keep = [x.clone() for x, _ in train.items]

    def args(out, **kw):
        a = main_finetune_mae.get_args_parser().parse_args(
            ["--model", "vit_test_patch16", "--batch_size", "4", "--epochs", "2", "--accum_iter", "2", "--warmup_epochs", "1",
             "--nb_classes", "5", "--output_dir", str(out), "--num_workers", "0", "--blr", "0.05", "--precision", "fp32", "--seed", "3",
             "--mixup", "0.8", "--cutmix", "1.0", "--smoothing", "0.1", "--clip_grad", "1.0", "--layer_decay", "0.75"])
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    torch.manual_seed(1)
    pre = models_vit.VisionTransformer(num_classes=5, **TINY)
    ckpt = tmp_path / "pretrain.pth"
    torch.save({"model": {k: v for k, v in pre.state_dict().items() if not k.startswith(("head.", "norm."))}}, ckpt)
    model, opt, hist = main_finetune_mae.run(args(tmp_path / "a", finetune=str(ckpt)), train, val)
    assert model.global_pool and [h["epoch"] for h in hist] == [0, 1] and all(np.isfinite(h["train"]["loss"]) for h in hist)
    assert hist[0]["train"]["samples"] == 16 and hist[0]["test"]["samples"] == 8
    assert all(torch.equal(a, b[0]) for a, b in zip(keep, train.items)), "the loader's own tensors are never mixed in place"
    assert len(opt.param_groups) == 8 and opt.param_groups[0]["lr_scale"] == 0.75 ** 3
    start = models_vit.VisionTransformer(num_classes=5, global_pool=True, **TINY)
    assert not torch.equal(model.blocks[0].mlp.fc1.weight.cpu(), pre.blocks[0].mlp.fc1.weight), "the encoder trained"
    lines = [json.loads(ln) for ln in open(tmp_path / "a" / "log.txt")]
    assert len(lines) == 2 and {"train_lr", "train_loss", "test_loss", "test_acc1", "test_acc5", "epoch", "n_parameters"} <= set(lines[1])
    assert lines[1]["test_acc1"] == hist[1]["test"]["acc1"] and lines[1]["n_parameters"] == sum(p.numel() for p in start.parameters())
    first, last = tmp_path / "a" / "ckpts" / "checkpoint-0.pth", tmp_path / "a" / "ckpts" / "checkpoint-1.pth"
    saved = torch.load(str(last), map_location="cpu", weights_only=False)
    assert {"model", "optimizer", "epoch", "scaler", "args"} == set(saved) and saved["epoch"] == 1
    assert set(saved["model"]) == set(start.state_dict()) and "fc_norm.weight" in saved["model"]
    assert {"lr", "lr_scale", "weight_decay", "betas", "eps", "params"} <= set(saved["optimizer"]["param_groups"][0])
    # resume from the first epoch's checkpoint: the second epoch is the uninterrupted run's, bit for bit
    model_b, _, hist_b = main_finetune_mae.run(args(tmp_path / "b", resume=str(first), finetune=str(ckpt)), train, val)
    assert [h["epoch"] for h in hist_b] == [1] and hist_b[0]["test"] == hist[1]["test"]
    assert hist_b[0]["train"]["loss"] == hist[1]["train"]["loss"]
    for (k, a), b in zip(model.state_dict().items(), model_b.state_dict().values()):
        assert torch.equal(a, b), k
    # --eval on the last checkpoint reports the last epoch's accuracy
    _, _, ev = main_finetune_mae.run(args(tmp_path / "c", resume=str(last), eval=True), None, val)
    assert ev[0]["test"]["acc1"] == hist[1]["test"]["acc1"] and ev[0]["test"]["loss"] == hist[1]["test"]["loss"]
    # fp16 (dynamic loss scaling), the cls token, label smoothing without mixing: one epoch, finite
    _, _, hist_h = main_finetune_mae.run(args(tmp_path / "d", precision="fp16", epochs=1, global_pool=False, mixup=0.0, cutmix=0.0),
                                          train, val)
    assert np.isfinite(hist_h[0]["train"]["loss"]) and np.isfinite(hist_h[0]["test"]["loss"])
    _, _, hist_m = main_finetune_mae.run(args(tmp_path / "e", precision="fp16", epochs=1), train, val)
    assert np.isfinite(hist_m[0]["train"]["loss"])
    with pytest.raises(NotImplementedError, match="drop_path"):
        main_finetune_mae.run(args(tmp_path / "f", drop_path=0.1), train, val)
