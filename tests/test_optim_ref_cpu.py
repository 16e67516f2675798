"""The bounds of tests/optim_ref.py are honest (CPU): f32 emulations of the optimizer kernels stay within 0.9 of every bound at every
case of tests/optim_cases.py, each listed wrong variant exceeds one (or differs in bits) on a named case, the Python loss-scale update
equals torch._amp_update_scale_ in every cell of the table, and the tick reference saturates where the f32 counter does."""
import numpy as np
import pytest
import torch

import optim_cases as C
import optim_ref as R
from test_gemm_ref_cpu import dgelu_f32
from test_rowops_ref_cpu import butterfly

f32 = torch.float32
SHADOWS = (torch.bfloat16, torch.float16, torch.float32)


def _case(regime, hname, step, n=C.N_CPU):
    h = C.HYPERS[hname]
    p, g, m, v = C.adamw_inputs(n, regime, C.hyper_gscale(hname), seed=step % 7)
    return p, g, m, v, R.record(*h, step=step)


def _worst(regime, hname, step, variant=None):
    p, g, m, v, rec = _case(regime, hname, step)
    emu = R.adamw_f32(p, g, m, v, rec, torch.bfloat16, variant)
    ref = R.adamw_step(p, g, m, v, rec)
    r = R.adamw_ratios(emu["p"], emu["m"], emu["v"], ref)
    r["shadow"] = 0.0 if R.equal_bits(emu["shadow"], emu["p"].to(torch.bfloat16)) else float("inf")
    return r


# ---- AdamW ---------------------------------------------------------------------------------------
def test_adamw_emulation_stays_under_the_bounds():
    peak, where = {"p": 0.0, "m": 0.0, "v": 0.0}, {}
    for regime, hname, step in C.adamw_cases():
        r = _worst(regime, hname, step)
        assert r["shadow"] == 0.0
        for k in peak:
            if r[k] > peak[k]:
                peak[k], where[k] = r[k], (regime, hname, step)
    print("adamw emulation peaks:", {k: (round(peak[k], 3), where[k]) for k in peak})
    assert all(x <= 0.9 for x in peak.values()), (peak, where)
    assert all(x > 0.2 for x in peak.values()), peak   # (a bound ten times too wide would say nothing)


@pytest.mark.parametrize("dtype", SHADOWS, ids=["bf16", "fp16", "f32"])
def test_adamw_shadow_of_the_emulation(dtype):
    p, g, m, v, rec = _case("suite", "b95_wd", 2, n=4100)
    emu = R.adamw_f32(p, g, m, v, rec, dtype)
    assert emu["shadow"].dtype == dtype and R.equal_bits(emu["shadow"], emu["p"].to(dtype))
    assert not R.equal_bits(R.adamw_f32(p, g, m, v, rec, dtype, "shadow_pre_update")["shadow"], emu["p"].to(dtype))


# variant -> the case that must reject it, and the output it shows in
REJECTED_AT = {
    "eps_in_sqrt": (("tiny", "b95_wd", 1000), "p"),
    "eps_times_rsqrt_bc2": (("tiny", "b999_wd0", 1), "p"),
    "bc_step_plus_1": (("suite", "b95_wd", 1), "p"),
    "bc_step_minus_1": (("suite", "b95_wd", 2), "p"),
    "wd_after_update": (("suite", "b999_wd", 1), "p"),
    "l2_decay": (("suite", "b95_wd", 1000), "m"),
    "v_unscaled": (("suite", "half", 2), "v"),
    "inv_scale_ignored": (("suite", "half_inv1024", 2), "m"),
    "m_beta2": (("suite", "b95_wd", 2), "m"),
    "shadow_pre_update": (("suite", "b95_wd", 1), "shadow"),
}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_adamw_wrong_variants_are_rejected(variant):
    case, out = REJECTED_AT[variant]
    r = _worst(*case, variant=variant)
    print(variant, case, {k: (x if x == float("inf") else round(x, 2)) for k, x in r.items()})
    assert r[out] > 1.0, (variant, case, r)
    assert max(_worst(*case).values()) <= 0.9   # (the right expression passes the same case)


def test_adamw_reference_is_torch_adamw():
    """Three steps of torch.optim.AdamW in float64 against adamw_step fed its own outputs: the restatement is the update rule."""
    p, g, m, v = C.adamw_inputs(257, "cold", 1.0)
    pt = p.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    pr, mr, vr = p.double(), m.double(), v.double()
    for step in (1, 2, 3):
        gs = C.adamw_inputs(257, "suite", 1.0, seed=step)[1]
        pt.grad = gs.double()
        opt.step()
        rec = R.record(1e-2, 0.9, 0.999, 1e-8, 0.05, step=step).double()   # (the f32 record widened; torch gets the same betas)
        o = R.adamw_step(pr, gs, mr, vr, rec)
        pr, mr, vr = o["p"], o["m"], o["v"]
    # the record holds f32(0.9), f32(0.999), f32(1e-2) ...: equal to torch's float64 hyper-parameters to 1e-7
    assert R.rel(pr, pt.detach()) < 1e-6


# ---- ticks ---------------------------------------------------------------------------------------
def test_tick_reference():
    rec = R.record(1e-3, 0.9, 0.95, 1e-8, 0.05, step=9)
    step, bc1, rs = R.tick(rec)
    assert step == 10.0 and bc1 == np.float32(1 - np.float32(0.9).astype(np.float64) ** 10)
    assert abs(rs - (1 - 0.95 ** 10) ** -0.5) < 1e-6
    rec[6] = float(C.TICK_SATURATED)
    assert R.tick(rec) == (R.SATURATED, 1.0, 1.0)            # 2^24 + 1 is not an f32: the counter stays, the corrections are 1
    rec[6] = 16777215.0
    assert R.tick(rec) == (R.SATURATED, 1.0, 1.0)
    rec[9] = 1.0
    assert R.tick(rec) is None
    for b1, b2 in C.TICK_BETAS:                                # saturation gives 1.0 for both beta pairs
        assert R.bias_corrections(b1, b2, C.TICK_SATURATED) == (1.0, 1.0)
    a, b = torch.tensor([1.0, 1.5]), torch.tensor([1.0 + 2.0 ** -23, 1.5])
    assert R.ulps_apart(a, b).tolist() == [1, 0]
    recs = C.tick_records(200)
    assert sorted(set(recs[:, 6].tolist())) == sorted(float(s) for s in C.TICK_STEPS + (C.TICK_SATURATED,))
    for n_list in C.TICK_N:
        lst = C.tick_list(200, n_list).tolist()
        assert len(lst) == n_list and all(a < b for a, b in zip(lst, lst[1:])) and 0 <= lst[0] and lst[-1] < 200


# ---- loss scale ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", C.loss_scale_cells(), ids=lambda c: c[0])
def test_loss_scale_update_is_torch_amp_update_scale(cell):
    _, state, stats, growth, backoff, interval = cell
    new, found, inv = R.loss_scale_update(state, stats, growth, backoff, interval)
    scale, tracker = torch.tensor([state[0]], dtype=f32), torch.tensor([int(state[1])], dtype=torch.int32)
    found_inf = torch.tensor([1.0 if stats[1] + stats[2] > 0 else 0.0], dtype=f32)
    torch._amp_update_scale_(scale, tracker, found_inf, growth, backoff, interval)
    assert new[0] == scale.item() and new[1] == float(tracker.item())
    assert np.isfinite(new[0])
    assert found == found_inf.item() == new[2]
    assert new[3] == state[3] + found and new[4] == state[4] + 1.0
    assert inv == new[5] == float(np.float32(1.0) / np.float32(state[0]))


def test_loss_scale_table_reaches_every_branch():
    seen = set()
    for _, state, stats, growth, backoff, interval in C.loss_scale_cells():
        new, found, _ = R.loss_scale_update(state, stats, growth, backoff, interval)
        grown = float(np.float32(state[0])) * growth
        seen.add("backoff" if found else "kept_on_overflow" if (new[1] == 0.0 and state[1] + 1 == interval and grown > 3.4e38)
                 else "grown" if state[1] + 1 == interval else "counted")
    assert seen == {"backoff", "kept_on_overflow", "grown", "counted"}


# ---- grad stats ----------------------------------------------------------------------------------
def emu_grad_stats(g, prior, order_seed, variant=None):
    """grad_stats_kernel's sum of squares in f32: per thread over its grid-stride vectors (element by element) and its tail element,
    the wave butterfly, (w0 + w1) + (w2 + w3), then the G partials added to `out` in a random order."""
    n = g.numel()
    nvec = n >> 2
    G, _ = R.grad_stats_grid(n)
    trips = max(-(-nvec // (G * 256)), 1)
    body = torch.zeros(trips * G * 256 * 4, dtype=f32)
    body[:4 * nvec] = g[:4 * nvec]
    body = body.reshape(trips, G, 256, 4)
    th = torch.zeros(G, 256, dtype=f32)
    for t in range(trips):
        for e in range(4):
            th = th + body[t, :, :, e] * body[t, :, :, e]
    if variant != "no_tail":
        for j in range(n & 3):
            th[0, j] = th[0, j] + g[4 * nvec + j] * g[4 * nvec + j]
    w = butterfly(th.reshape(G, 4, 64))
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    out = torch.tensor(prior, dtype=f32)
    for i in torch.randperm(G, generator=C.gen(order_seed)).tolist():
        out = out + part[i]
    return out


@pytest.mark.parametrize("n", C.STATS_SIZES)
def test_grad_stats_bound(n):
    g = C.stats_input(n)
    G, k = R.grad_stats_grid(n)
    assert 1 <= G <= 1024 and (G - 1) * 256 < max(n >> 2, 1) and 256 * G * (k // 4) >= (n >> 2)
    peak = 0.0
    for prior in (0.0, C.STATS_PRIOR[0]):
        ref = R.grad_stats(g, (prior, 0.0, 0.0))
        for seed in range(3 if G > 1 else 1):
            got = emu_grad_stats(g, prior, seed)
            peak = max(peak, abs(got.double().item() - ref["ss"]) / ref["e_ss"])
    print(f"grad_stats n={n} G={G} k={k}: emulation peak {peak:.3f}")
    assert peak <= 0.9
    if n & 3:   # the tail dropped: the whole sum at n < 4, one term of five at n = 5
        ref = R.grad_stats(g)
        bad = abs(emu_grad_stats(g, 0.0, 0, "no_tail").double().item() - ref["ss"]) / ref["e_ss"]
        if n <= 5:
            assert bad > 1.0, (n, bad)


def test_grad_stats_grid_past_the_cap():
    assert R.grad_stats_grid(C.STATS_SIZES[-1]) == (1024, 9)    # two trips of four and a tail element
    assert R.grad_stats_grid(3) == (1, 1) and R.grad_stats_grid(4) == (1, 4) and R.grad_stats_grid(100003) == (98, 5)
    r = R.grad_stats(torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), 2.0]), C.STATS_PRIOR)
    assert (r["ss"], r["nan"], r["inf"], r["finite"]) == (5.75, 3.0, 3.0, False)


# ---- dgelu ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("bf16", "fp16", "fp32"))
def test_dgelu_bound(prec):
    dy, pre = C.dgelu_inputs(4 * ((C.dgelu_table(prec).numel() + 3) // 4), prec)
    assert pre.float().abs().max() == 12.0 and pre.numel() > 30000
    assert bool((dy.float() == 0).any()) and bool(torch.signbit(dy.float()[dy.float() == 0]).any())
    want, bound = R.dgelu(dy, pre, prec)
    d = torch.from_numpy(dgelu_f32(pre.float().numpy()))
    got32 = dy.float() * d
    got = got32.to(dy.dtype)
    raw = R.ratio(got32, want, dy.double().abs() * R.G_DPHI + 2 * R.U32 * want.abs())
    stored = R.ratio(got, want, bound)
    print(f"dgelu {prec}: emulation peak {raw:.3f} in front of the store, {stored:.3f} stored")
    assert raw <= 0.9 and stored <= 1.0
    # wrong: the tanh approximation of GELU's derivative; the pdf term dropped
    x = pre.double()
    inner = 0.7978845608028654 * (x + 0.044715 * x ** 3)
    tanh_d = 0.5 * (1 + torch.tanh(inner)) + 0.5 * x * (1 - torch.tanh(inner) ** 2) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
    assert R.ratio((dy.double() * tanh_d).float().to(dy.dtype), want, bound) > 1.0
    cdf_only = 0.5 * (1 + torch.erf(x / 2 ** 0.5))
    assert R.ratio((dy.double() * cdf_only).float().to(dy.dtype), want, bound) > 1.0
