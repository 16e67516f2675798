"""Gradient clipping by global norm and per-group gradient norms on the device: pm_grad_norms (deterministic f64 statistics over
flat gradient segments), pm_grad_clip (the coefficient of torch.nn.utils.clip_grad_norm_, folded into slot [10] of the AdamW
records) and FusedAdamW.step(max_norm=...) / grad_norms / last_clip / the training loops on top of them.  `pytest -m gpu`.

Bounds.  Sums of squares: the f32 squares are exact in f64, and with at least 256 accumulators over at most 2^20 elements the
longest chain is 4096 additions: 4096 x 2^-53 = 4.5e-13 < 1e-12 relative.  Coefficient: one f32 rounding of a f64 value, 1 ulp.
Parameters / moments against torch: the 2e-5 of tests/test_gpu_models.py test_fused_adamw_matches_torch_adamw_and_graph_replay
(the only new error is the f32 rounding of the coefficient).  Everything that must not move: bit for bit.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from ssl4polyp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
FLT_MIN = float(np.finfo(np.float32).tiny)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _close(a, b, rel=1e-15):
    """a == b up to a few float64 roundings (sqrt, products)."""
    return abs(float(a) - float(b)) <= rel * abs(float(b))


class Guarded:
    """A tensor of n elements inside an allocation with GUARD sentinel elements in front of it and behind it."""

    def __init__(self, n, dtype, fill):
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.n, self.fill = n, fill
        self.view = self.full[GUARD:GUARD + n]

    def intact(self):
        g = torch.cat([self.full[:GUARD], self.full[GUARD + self.n:]])
        return bool((g == self.fill).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the statistics kernel
# ---------------------------------------------------------------------------------------------------------------------------
SEG_GROUPS = (0, 1, 3, 0, 3, 1, 0, 1)           # interleaved; group 2 has no segment at all
# the sizes of tests/test_gpu_adamw_footprint.py: one vector, a ragged chunk, 64 chunks + one vector, more chunks than workgroups
SEG_SIZES = (4, 1028, 262148, 1048580, 1028, 4, 262148, 1028)


def _stat_inputs(planted):
    rng = np.random.default_rng(17)
    segs = []
    for grp, n in zip(SEG_GROUPS, SEG_SIZES):
        x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        if n > 4:
            x[5::97] = np.float32(1e-40)          # denormals
            x[1] = np.float32(-3e-45)
        if grp == 3:                               # +-1e18: the squares overflow f32 and need f64's range
            x[0], x[-1] = np.float32(1e18), np.float32(-1e18)
        segs.append(x)
    if planted:  # 3 NaN in group 0, +inf and -inf in group 1
        segs[3][7], segs[3][1048579], segs[6][4096] = np.nan, np.nan, np.nan
        segs[1][1027], segs[7][0] = np.inf, -np.inf
    return segs


@pytest.mark.parametrize("planted", [False, True])
def test_statistics_kernel_per_group_f64_sums_counts_and_bits(planted):
    lib = _lib.load()
    G = 4
    host = _stat_inputs(planted)
    bufs = []
    for x in host:
        b = Guarded(len(x), torch.float32, 7.0)   # (a guard that was read would show in the sums)
        b.view.copy_(torch.from_numpy(x))
        bufs.append(b)
    arr = (_lib.GradSegment * len(bufs))(*[_lib.GradSegment(b.view.data_ptr(), b.n, g) for b, g in zip(bufs, SEG_GROUPS)])
    size = ctypes.c_size_t(0)
    _lib.check(lib.pm_grad_norms_workspace(len(bufs), G, ctypes.byref(size)), "pm_grad_norms_workspace")
    assert size.value % 8 == 0
    ws = Guarded(size.value // 8, torch.float64, -5.0)
    sumsq = Guarded(G, torch.float64, -5.0)
    stats = Guarded(3, torch.float32, -5.0)
    runs = []
    for poison in (-5.0, 123.0):                   # the workspace is fully rewritten: what it held before does not matter
        ws.view.fill_(poison)
        _lib.check(lib.pm_grad_norms(arr, len(bufs), G, ws.view.data_ptr(), size.value, sumsq.view.data_ptr(), stats.view.data_ptr(),
                                     _stream()), "pm_grad_norms")
        runs.append((sumsq.view.clone(), stats.view.clone()))
    torch.cuda.synchronize()
    assert ws.intact() and sumsq.intact() and stats.intact() and all(b.intact() for b in bufs)
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))     # bit-identical, NaN included
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    got, triple = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    want = np.zeros(G)
    n_nan = n_inf = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for x, g in zip(host, SEG_GROUPS):
            x64 = x.astype(np.float64)
            fin = np.isfinite(x64)
            want[g] += math.fsum(np.square(x64[fin]))
            if not fin.all():
                want[g] += float(np.square(x64[~fin]).sum())   # nan if any NaN, else inf
            n_nan, n_inf = n_nan + int(np.isnan(x).sum()), n_inf + int(np.isinf(x).sum())
    for g in range(G):
        print(f"[measured] group {g}: got {got[g]!r}, float64 reference {want[g]!r}")
        if np.isfinite(want[g]):
            assert abs(got[g] - want[g]) <= 1e-12 * want[g], g
        else:
            assert np.array_equal(got[g], want[g], equal_nan=True), g
    assert got[2] == 0.0 and want[3] > 1.9e36
    assert (n_nan, n_inf) == ((3, 2) if planted else (0, 0)) and triple[1] == n_nan and triple[2] == n_inf
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.float64(0.0)
        for g in range(G):
            total = total + got[g]
        assert np.array_equal(triple[0], np.float32(total), equal_nan=True)            # the f64 sums, added in group order, rounded


def test_statistics_kernel_several_chunks_per_workgroup_and_two_launches():
    """The two remaining paths: more chunks than workgroups (5 x 2^20 + 4 elements = 1281 chunks of 4096: two per workgroup, the
    last of them shared with the next segment, so the group changes inside a workgroup) and more segments than one launch
    carries (70 > 64).  A lane adds 32 squares, the trees 8 levels, the second stage 6 rows + 8 levels: far inside 1e-12."""
    lib = _lib.load()
    rng = np.random.default_rng(23)
    sizes = [5 * (1 << 20) + 4] + [1028] * 69
    groups = [0] + [1 + (i % 2) for i in range(69)]
    host = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for n in sizes]
    flat = torch.from_numpy(np.concatenate(host)).to(DEV)   # (contiguous ranges, as the optimizer's flat gradient)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    arr = (_lib.GradSegment * 70)(*[_lib.GradSegment(flat.data_ptr() + 4 * int(o), n, g) for o, n, g in zip(offs, sizes, groups)])
    size = ctypes.c_size_t(0)
    _lib.check(lib.pm_grad_norms_workspace(70, 3, ctypes.byref(size)), "pm_grad_norms_workspace")
    ws, sumsq, stats = Guarded(size.value // 8, torch.float64, -5.0), Guarded(3, torch.float64, -5.0), Guarded(3, torch.float32, -5.0)
    _lib.check(lib.pm_grad_norms(arr, 70, 3, ws.view.data_ptr(), size.value, sumsq.view.data_ptr(), stats.view.data_ptr(), _stream()),
               "pm_grad_norms")
    torch.cuda.synchronize()
    assert ws.intact() and sumsq.intact() and stats.intact()
    got = sumsq.view.cpu().numpy()
    want = [math.fsum(np.square(np.concatenate([x for x, g in zip(host, groups) if g == k]).astype(np.float64))) for k in range(3)]
    print(f"[measured] got {got.tolist()}, float64 reference {want}")
    assert all(abs(got[k] - want[k]) <= 1e-12 * want[k] for k in range(3))
    assert stats.view.cpu().tolist() == [float(np.float32((got[0] + got[1]) + got[2])), 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the coefficient
# ---------------------------------------------------------------------------------------------------------------------------
def _clip(sumsq, grad_scale=1.0, slot10=0.0, max_norm=1.0, clip=1, scaled=0):
    lib = _lib.load()
    G = len(sumsq)
    s = torch.tensor(sumsq, dtype=torch.float64, device=DEV)
    hyper = torch.zeros(G, 16, device=DEV)
    hyper[:, :6] = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 0.05, grad_scale], device=DEV)
    hyper[:, 10] = slot10
    hyper[:, 11:] = 77.0
    before = hyper.clone()
    record = Guarded(G + 3, torch.float64, -5.0)
    _lib.check(lib.pm_grad_clip(s.data_ptr(), hyper.data_ptr(), G, max_norm, clip, scaled, record.view.data_ptr(), _stream()),
               "pm_grad_clip")
    torch.cuda.synchronize()
    assert record.intact()
    other = [c for c in range(16) if c != 10]
    assert torch.equal(hyper[:, other], before[:, other])      # only slot [10] is ever written
    return hyper[:, 10].cpu().numpy(), record.view.cpu().numpy(), before[:, 10].cpu().numpy()


def test_clip_coefficient_and_slot_10():
    sumsq = [1.0, 4.0, 0.0]
    total = math.sqrt(5.0)
    # below max_norm: coef is exactly 1, a loss-scale factor in [10] keeps its value exactly, and an empty slot reads 1.0 (= none)
    h10, rec, _ = _clip(sumsq, max_norm=10.0)
    assert rec[4] == 1.0 and _close(rec[3], total) and _close(rec[0], 1.0) and _close(rec[1], 2.0) and rec[2] == 0.0
    assert rec[5] == 10.0 and list(h10) == [1.0] * 3
    inv = float(np.float32(1.0 / 1024.0))
    h10, rec, was = _clip(sumsq, slot10=inv, max_norm=10.0, scaled=1)
    assert rec[4] == 1.0 and np.array_equal(h10, was) and _close(rec[3], total * inv)
    # above max_norm: within one f32 ulp of the float64 expression
    want = 1.0 / (total + 1e-6)
    h10, rec, _ = _clip(sumsq, max_norm=1.0)
    print(f"[measured] coef {rec[4]!r} (float64 {want!r}); slot [10] {h10[0]!r}")
    assert _close(rec[4], want) and all(abs(float(h) - want) <= _ulp32(want) for h in h10)
    # with 1 / loss scale already in [10] (written by the scale update of this step): the norm is the unscaled one, [10] the product
    big = [v * 1024.0 ** 2 for v in sumsq]
    h10, rec, _ = _clip(big, slot10=inv, max_norm=1.0, scaled=1)
    assert _close(rec[3], total) and _close(rec[4], want)
    assert all(abs(float(h) - want * inv) <= _ulp32(want * inv) for h in h10)
    # without `scaled`, what an earlier clip left in [10] counts as 1
    h10, rec, _ = _clip(sumsq, slot10=0.37, max_norm=1.0, scaled=0)
    assert _close(rec[4], want) and all(abs(float(h) - want) <= _ulp32(want) for h in h10)
    # grad_scale = 1/2 (two ranks, summed gradients): the norm of the averaged gradient
    h10, rec, _ = _clip(sumsq, grad_scale=0.5, max_norm=1.0)
    want_half = 1.0 / (0.5 * total + 1e-6)
    assert _close(rec[0], 0.5) and _close(rec[1], 1.0) and rec[2] == 0.0 and _close(rec[3], 0.5 * total) and _close(rec[4], want_half)
    assert all(abs(float(h) - want_half) <= _ulp32(want_half) for h in h10)
    # norms only: the records are left alone
    h10, rec, was = _clip(sumsq, slot10=0.37, clip=0)
    assert np.array_equal(h10, was) and rec[4] == 1.0 and _close(rec[3], total) and rec[5] == math.inf
    # never the 0 that means "no scaling"
    h10, rec, _ = _clip([1e300, 0.0, 0.0], max_norm=1.0)
    assert rec[4] == FLT_MIN and list(h10) == [np.float32(FLT_MIN)] * 3


# ---------------------------------------------------------------------------------------------------------------------------
# 3 - 5. the optimizer
# ---------------------------------------------------------------------------------------------------------------------------
def _tiny_cls(prec="fp32", seed=5, depth=2):
    import ssl4polyp_amd as A
    torch.manual_seed(seed)
    return A.ViT_from_MAE(None, True, 2, False, None, embed_dim=64, depth=depth, num_heads=2, out_token="cls", precision=prec).to(DEV)


def _two_groups(m):
    head = list(m.lin_head.parameters())
    hid = {id(p) for p in head}
    return [{"params": head, "lr": 2e-3, "name": "head"}, {"params": [p for p in m.parameters() if id(p) not in hid and p.requires_grad]}]


def _f64_norms(groups, div=1.0):
    gn = [math.sqrt(sum(float((p.grad.double() / div).square().sum()) for p in g["params"] if p.grad is not None)) for g in groups]
    return gn, math.sqrt(sum(v * v for v in gn))


def _moments(opt, names):
    sd = opt.state_dict()
    return {n: (sd["state"][k]["exp_avg"], sd["state"][k]["exp_avg_sq"]) for k, n in enumerate(names) if k in sd["state"]}


def test_clipped_fused_adamw_matches_clip_grad_norm_and_torch_adamw_fp32():
    from ssl4polyp_amd.optim import FusedAdamW
    imgs = torch.randn(2, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    labels = torch.tensor([1.0, 0.0], device=DEV)
    MAX_NORM = 0.01
    norms_t = []

    def make(kind, max_norm):
        m = _tiny_cls()
        groups = _two_groups(m)
        names = {id(p): n for n, p in m.named_parameters()}
        order = [names[id(p)] for g in groups for p in g["params"]]
        if kind == "torch":
            opt = torch.optim.AdamW(groups, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
        else:
            opt = FusedAdamW(m, groups, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)

        def step():
            opt.zero_grad(set_to_none=True)
            z = m(imgs)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(z[:, 1] - z[:, 0], labels)
            loss.backward()
            if kind == "torch":
                norms_t.append(float(torch.nn.utils.clip_grad_norm_([p for g in groups for p in g["params"]], max_norm)))
                opt.step()
            else:
                opt.step(max_norm=max_norm)
            return loss
        return m, opt, step, order

    m_t, o_t, s_t, order = make("torch", MAX_NORM)
    m_f, o_f, s_f, _ = make("fused", MAX_NORM)
    m_u, o_u, s_u, _ = make("fused", None)        # the same run without clipping
    assert o_f.last_clip is None
    for it in range(5):
        if it == 3:
            for o in (o_t, o_f, o_u):
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
        lt, lf, _ = s_t(), s_f(), s_u()
    torch.cuda.synchronize()
    print(f"[measured] torch total norms {norms_t}, max_norm {MAX_NORM}")
    assert len(norms_t) == 5 and all(n > MAX_NORM for n in norms_t)      # clipping was active on every step
    assert abs(lt.item() - lf.item()) < 1e-5
    for (n, pt), (_, pf) in zip(m_t.named_parameters(), m_f.named_parameters()):
        if pt.requires_grad and not n.endswith("attn.qkv.bias"):  # (see test_fused_adamw_matches_torch_adamw_and_graph_replay)
            assert rel_l2(pf, pt) < 2e-5, n
    mo_t, mo_f, mo_u = _moments(o_t, order), _moments(o_f, order), _moments(o_u, order)
    assert set(mo_t) == set(mo_f) == set(mo_u) and len(mo_t) > 10
    worst = 0.0
    for n in mo_t:
        if n.endswith("attn.qkv.bias"):
            continue
        for k in (0, 1):  # Adam's parameters hardly depend on the gradient's scale; its moments do
            e = rel_l2(mo_f[n][k], mo_t[n][k])
            worst = max(worst, e)
            assert e < 2e-5, (n, k, e)
            assert rel_l2(mo_u[n][k], mo_t[n][k]) > 1e-2, (n, k)
    print(f"[measured] worst moment rel-L2 against torch {worst:.3e}")
    # the record of the last step against float64 of the gradients it consumed (the flat gradients are not rewritten)
    rec = o_f.last_clip.cpu().numpy()
    gn, total = _f64_norms(o_f.param_groups)
    want = R.clip_coef(total, MAX_NORM)
    print(f"[measured] last_clip {rec.tolist()}; float64 groups {gn}, total {total}, coef {want}")
    assert rec.shape == (5,) and rec[4] == MAX_NORM
    assert all(abs(rec[g] - gn[g]) <= 1e-12 * gn[g] for g in range(2)) and abs(rec[2] - total) <= 1e-12 * total
    assert abs(rec[3] - want) <= 1e-12 * want
    assert all(abs(float(h) - want) <= _ulp32(want) for h in o_f._hyper[:, 10].cpu())
    # grad_norms: the same figures without a step, and no clip coefficient in them
    g2 = o_f.grad_norms().cpu().numpy()
    assert g2.shape == (3,) and all(abs(g2[i] - v) <= 1e-12 * v for i, v in enumerate(gn + [total]))
    # dropping max_norm clears what the clip left in slot [10]
    o_f.step()
    assert float(o_f._hyper[:, 10].abs().max()) == 0.0
    with pytest.raises(_lib.PolypMaeError):
        o_f.step(max_norm=0.0)


def test_fp16_loss_scaler_with_max_norm_against_torch_gradscaler(monkeypatch):
    """Oracle: the same model driven by torch's GradScaler (unscale_, clip_grad_norm_, step, update) and torch AdamW, as
    tests/test_gpu_fp16.py test_torch_gradscaler_drives_the_fp16_path_too drives it, held to that test's conditions (the scale
    stays, the loss falls and is finite) and, sharper, to that file's 2e-5 for a FusedAdamW step against torch AdamW on the
    unscaled gradients.  Two fp16 copies that evolve apart by f32 roundings of the update drift by 1e-4 in the gradient norm
    within three steps (fp16 weight roundings flip): the oracle's weights are therefore set to this model's before every step,
    so that both see the same gradients bit for bit and every step's update is compared, with moments that have 4 steps of history."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd.optim import FusedAdamW, LossScaler
    imgs = torch.randn(4, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    labels = torch.tensor([0, 1, 1, 0], device=DEV)
    MAX_NORM = 0.01
    m, ref = _tiny_cls("fp16", seed=11), _tiny_cls("fp16", seed=11)
    opt = FusedAdamW(m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    params_t = [p for p in ref.parameters() if p.requires_grad]
    topt = torch.optim.AdamW(params_t, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    sc = LossScaler(init_scale=4096.0)
    tsc = torch.amp.GradScaler("cuda", init_scale=4096.0)
    lib = _lib.load()   # (the one handle every host wrapper calls through)
    calls = {"pm_grad_norms": 0, "pm_grad_stats": 0}
    for name in calls:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    losses = []
    for it in range(4):
        opt.zero_grad(set_to_none=True)
        loss = A.supervised_loss(m(imgs), labels, pos_weight=1.0)
        losses.append(loss.detach())
        sc.scale(loss).backward()
        sc.unscale_(opt)
        sc.step(opt, max_norm=MAX_NORM)
        sc.update()
        topt.zero_grad(set_to_none=True)
        tsc.scale(A.supervised_loss(ref(imgs), labels, pos_weight=1.0)).backward()
        for p, q in zip(m.parameters(), ref.parameters()):
            assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad)
        tsc.unscale_(topt)
        total_t = float(torch.nn.utils.clip_grad_norm_(params_t, MAX_NORM))
        tsc.step(topt)
        tsc.update()
        assert total_t > MAX_NORM
        # the reported norms are those of the UNSCALED gradients: torch's own (f32) and float64 of this model's gradients / scale
        rec = opt.last_clip.cpu().numpy()
        _, total = _f64_norms(opt.param_groups, div=4096.0)
        print(f"[measured] step {it}: last_clip {rec.tolist()}, torch total {total_t!r}, float64 total {total!r}")
        assert abs(rec[1] - total) <= 1e-12 * total and abs(rec[0] - total) <= 1e-12 * total
        assert abs(rec[1] - total_t) < 1e-5 * total_t                 # (torch's figure is an f32 norm)
        assert abs(rec[2] - R.clip_coef(total, MAX_NORM)) <= 1e-12 * rec[2]
        with torch.no_grad():
            for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
                if p.requires_grad and not n.endswith("attn.qkv.bias"):
                    assert rel_l2(p, q) < 2e-5, (it, n)
                q.copy_(p)
    assert calls == {"pm_grad_norms": 4, "pm_grad_stats": 0}        # one statistics pass per step, not two
    gn = opt.grad_norms(sc).cpu().numpy()                             # (one more pass, on request)
    assert abs(gn[1] - total) <= 1e-12 * total and calls["pm_grad_norms"] == 5
    assert sc.get_scale() == tsc.get_scale() == 4096.0 and sc.counters()["skipped"] == 0
    losses = [float(l) for l in losses]
    assert losses[-1] < losses[0] and all(l == l for l in losses)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    mo, mo_t = _moments(opt, [n for n, _ in m.named_parameters()]), _moments(topt, names)   # (opt holds every parameter)
    assert set(mo) >= set(mo_t) and len(mo_t) > 10
    mo = {n: mo[n] for n in mo_t}
    for n in mo:
        if not n.endswith("attn.qkv.bias"):
            assert rel_l2(mo[n][0], mo_t[n][0]) < 2e-5 and rel_l2(mo[n][1], mo_t[n][1]) < 2e-5, n
    # a step with an Inf in the flat gradient: nothing is touched, bit for bit, and the scale backs off
    opt.zero_grad(set_to_none=True)
    sc.scale(A.supervised_loss(m(imgs), labels, pos_weight=1.0)).backward()
    m.lin_head.weight.grad.view(-1)[1] = float("inf")
    f = m._rt.flat
    before = {k: t.clone() for k, t in list(f.P.items()) + [("M" + r, t) for r, t in opt._M.items()] + [("V" + r, t) for r, t in opt._V.items()]}
    shadow = f.S.clone() if f.S is not None else None
    sc.step(opt, max_norm=MAX_NORM)
    sc.update()
    torch.cuda.synchronize()
    after = dict(list(f.P.items()) + [("M" + r, t) for r, t in opt._M.items()] + [("V" + r, t) for r, t in opt._V.items()])
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert shadow is None or torch.equal(shadow, f.S)
    assert sc.get_scale() == 2048.0 and sc.counters()["found_inf_last"] and sc.counters()["skipped"] == 1
    assert not math.isfinite(float(opt.last_clip[1]))


def _tiny_mae():
    import ssl4polyp_amd as A
    torch.manual_seed(3)
    return A.MaskedAutoencoderViT(embed_dim=64, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=2, decoder_num_heads=2).to(DEV)


def _run(kind, max_norm, mode="eager", steps=4):
    """`steps` optimizer steps of a tiny model from one seed; returns every buffer the update writes, and the last clip record."""
    from ssl4polyp_amd.graph import GraphedStep
    from ssl4polyp_amd.optim import FusedAdamW, add_weight_decay
    g = torch.Generator(device=DEV).manual_seed(11)
    imgs = torch.randn(4, 3, 224, 224, device=DEV, generator=g)
    labels = torch.tensor([1.0, 0.0, 0.0, 1.0], device=DEV)
    noise = torch.rand(4, 196, device=DEV, generator=g)
    overlap = mode == "overlap"
    if kind == "cls":
        m = _tiny_cls("bf16", seed=3, depth=3)
        opt = FusedAdamW(m, _two_groups(m), lr=1e-3, weight_decay=0.05, overlap_forward=overlap)
    else:
        m = _tiny_mae()
        opt = FusedAdamW(m, add_weight_decay(m, 0.05), lr=2e-3, betas=(0.9, 0.95), overlap_forward=overlap)
    kw = {} if max_norm is None else {"max_norm": max_norm}

    def step():
        opt.zero_grad(set_to_none=True)
        if kind == "cls":
            z = m(imgs)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(z[:, 1] - z[:, 0], labels)
        else:
            loss = m(imgs, 0.75, noise=noise)[0]
        loss.backward()
        opt.step(**kw)
        return loss

    if mode == "graph":
        gs = GraphedStep(step, opt, warmup=1)      # one eager step, then the captured step replayed
        for _ in range(steps - 1):
            gs.replay()
    else:
        for _ in range(steps):
            step()
    opt.sync()
    torch.cuda.synchronize()
    f = m._rt.flat
    out = {"P" + r: t.clone() for r, t in f.P.items()}
    out.update({"M" + r: t.clone() for r, t in opt._M.items()})
    out.update({"V" + r: t.clone() for r, t in opt._V.items()})
    if f.S is not None:
        out["S"] = f.S.clone()
    if max_norm is not None:
        out["clip"] = opt.last_clip.clone()
    return out


@pytest.mark.parametrize("kind", ["cls", "mae"])
def test_a_clip_that_never_bites_changes_no_bit(kind):
    """max_norm = 1e30: coef is exactly 1, so parameters, moments and shadow equal those of a step without max_norm."""
    a, b = _run(kind, None, steps=3), _run(kind, 1e30, steps=3)
    assert float(b["clip"][-2]) == 1.0 and float(b["clip"][-1]) == 1e30 and 0 < float(b["clip"][-3]) < 1e3
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert "S" in a and len(a) == 7


def test_clipped_eager_graph_replay_and_overlap_agree_bit_for_bit():
    eager, graph, over = (_run("cls", 0.01, mode) for mode in ("eager", "graph", "overlap"))
    assert float(eager["clip"][-2]) < 1.0          # the clip was active
    for k in eager:
        assert torch.equal(eager[k], graph[k]), ("graph", k)
        assert torch.equal(eager[k], over[k]), ("overlap", k)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the loops
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_loops_log_group_norms_and_clip_coefficient():
    from types import SimpleNamespace
    import ssl4polyp_amd as A
    from ssl4polyp_amd import train as T
    from ssl4polyp_amd.optim import FusedAdamW, add_weight_decay
    dev = torch.device("cuda", 0)
    pw = torch.tensor(1.0, device=dev)
    base_keys = {"step", "loss", "lr", "grad_norm", "grad_nan", "grad_inf"}

    def cls_run(**kw):
        m = _tiny_cls("bf16")
        opt = FusedAdamW(m, _two_groups(m), lr=1e-3, weight_decay=0.05)
        loader = T.SyntheticLoader(4, 4, dev, seed=4)
        st = T.train_epoch_cls(m, loader, opt, dev, pos_weight=pw, log_every=2, printer=None, **kw)
        return st, opt

    st, _ = cls_run()
    assert [set(r) for r in st.history] == [base_keys, base_keys] and st.grad_norm_groups == {} and st.clip_coef != st.clip_coef
    plain_norm = st.history[0]["grad_norm"]
    st, opt = cls_run(clip_grad=0.01, group_grad_norms=True)
    for rec in st.history:
        assert set(rec) == base_keys | {"grad_norm_groups", "clip_coef"}
        gg = rec["grad_norm_groups"]
        assert list(gg) == ["head", "group1"] and all(v > 0 for v in gg.values())
        assert rec["grad_norm"] == pytest.approx(math.sqrt(sum(v * v for v in gg.values())), rel=1e-12)
        assert rec["clip_coef"] == pytest.approx(R.clip_coef(rec["grad_norm"], 0.01), rel=1e-12) and rec["clip_coef"] < 1.0
    assert st.clip_coef == st.history[-1]["clip_coef"] and st.grad_norm_groups == st.history[-1]["grad_norm_groups"]
    st, _ = cls_run(group_grad_norms=True)         # norms without clipping
    for rec in st.history:
        assert set(rec) == base_keys | {"grad_norm_groups", "clip_coef"} and rec["clip_coef"] == 1.0
        assert rec["grad_norm"] == pytest.approx(math.sqrt(sum(v * v for v in rec["grad_norm_groups"].values())), rel=1e-12)
    # the same step of the same run as the plain loop logged from pm_grad_stats' f32 atomic sum (logging accuracy: ~1e-6)
    assert st.history[0]["grad_norm"] == pytest.approx(plain_norm, rel=1e-4)
    # MAE loop: args.clip_grad
    torch.manual_seed(21)
    m = A.MaskedAutoencoderViT(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                               decoder_num_heads=1).to(dev)
    opt = FusedAdamW(m, add_weight_decay(m, 0.05), lr=2e-3, betas=(0.9, 0.95))
    args = SimpleNamespace(lr=2e-3, min_lr=0.0, warmup_epochs=1, epochs=4, accum_iter=1, mask_ratio=0.75, clip_grad=0.05)
    st = T.train_one_epoch_mae(m, T.SyntheticLoader(8, 4, dev, img_size=32, seed=3), opt, dev, 0, args, log_every=2, printer=None)
    assert [set(r) for r in st.history] == [base_keys | {"grad_norm_groups", "clip_coef"}] * 2
    assert list(st.history[-1]["grad_norm_groups"]) == ["group0", "group1"] and 0 < st.history[-1]["clip_coef"] <= 1.0
    args.clip_grad = None
    st = T.train_one_epoch_mae(m, T.SyntheticLoader(8, 4, dev, img_size=32, seed=3), opt, dev, 1, args, log_every=2, printer=None)
    assert [set(r) for r in st.history] == [base_keys] * 2
