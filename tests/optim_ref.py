"""Float64 restatements of the kernels that write the weights (pm_misc.hip: adamw_kernel, adamw_dev_kernel, the two tick kernels,
loss_scale_update_kernel, grad_stats_kernel, dgelu_kernel; pm_head.hip: scale_kernel) and the element-wise bounds of their outputs
(not a test module).  Every reference takes the operands as the kernel sees them -- the f32 buffers and the 16-float hyper record as
stored -- and runs in plain torch on whichever device they live on.  tests/test_optim_ref_cpu.py holds each bound to an f32 emulation
of the kernel's expression (and to wrong variants of it); tests/test_gpu_optim_edges.py holds the kernels to them.  u = 2^-24.

ADAMW (adamw_step).  The kernels' expression, per element, every operation one f32 rounding:
    gr = g gscale;  p *= 1 - lr wd;  m' = beta1 m + (1 - beta1) gr;  v' = beta2 v + (1 - beta2) gr gr
    denom = sqrt(v') rsqrt_bc2 + eps;  p' = p - (lr / bc1) (m' / denom)
gscale = hyper[5] (hyper[10] or 1) is formed in f32 as the kernel forms it, bc1 and rsqrt_bc2 are taken as stored.  1 - beta is
exact for beta >= 0.5 (Sterbenz).  Bounds, to first order in u, no safety factor:
    e_m    = 4 u (|beta1 m| + |(1 - beta1) gr|)      gr, the two products, the sum -- at most three of them on either term
    e_v    = 5 u v'                                  gr twice, two products, the sum; every term is positive
    r_den  = 5.5 u                                   half of v's 5 u, sqrtf, * rsqrt_bc2, + eps; all terms positive
    e_q    = |q| (r_den + u) + e_m / denom           q = m' / denom: the divide
    e_step = (lr / bc1) e_q + 2 u |step|             lr / bc1 and the product
    e_p    = 3 u |p (1 - lr wd)| + e_step + u |p'|   lr wd, 1 - that, the product; the final subtraction
Contraction into fused multiply-adds only removes roundings.  What the build's divide and square root are granted: one u each, i.e.
correctly rounded, which is what hipcc gives at its defaults (-fhip-fp32-correctly-rounded-divide-sqrt; f32 subnormals are not
flushed on gfx9).  The CPU test asserts that the f32 emulation stays under 0.9 of every bound; that tenth is the room a divide or
square root of up to 1 ulp (2 u) would need at the peak, as the GELU bounds of gemm_ref.py leave v_rcp_f32 / v_exp_f32 theirs.
The regimes keep every intermediate normal (|g gscale| >= 1e-15), so no absolute subnormal term appears.
The shadow is p' as stored, converted once: bit-equal to p_out.to(dtype), NaN by NaN-ness (equal_bits).

TICK (tick): h[6] + 1 exactly; h[7] = f32(1 - beta1^step), h[8] = f32(1 / sqrt(1 - beta2^step)) from float64, within one f32 ulp (the
device's f64 pow need not match libm's last bit).  The f32 counter saturates at 2^24 = 16 777 216 (16 777 216 + 1 rounds back), where
both corrections are 1.0 for every beta the project uses.

LOSS SCALE (loss_scale_update): torch._amp_update_scale_ restated in f32 scalar arithmetic, plus the kernel's own slots (found_inf,
skipped steps, steps, 1 / scale).  Exact.  A growth that overflows f32 keeps the scale and restarts the tracker, as torch does.

GRAD STATS (grad_stats): counts exact; sum of squares within (k + 9 + G) u T of the float64 sum T (what `out` held before included):
k terms per thread (4 per vector of its grid-stride loop, + 1 for a tail element), 9 for the square, the six butterfly levels and the
two levels of the workgroup tree, G atomic additions in any order.

DGELU (dgelu): want = dy gelu'(pre) in float64; |dy| G_DPHI + 2 u |want| (the f32 conversion is exact, gelu' carries G_DPHI, the
product rounds once and gelu's own final fma once), then store_bound.

SCALE: one IEEE multiplication per element, torch.equal to x * s.

Peaks (largest err / bound; "emu" = the f32 emulation on the CPU over every case of optim_cases.py, "device" = an MI355X, the whole
of tests/test_gpu_optim_edges.py):
    output                                   emu      device
    adamw p  (adamw_kernel: pm_adamw)        0.582    0.355     emu peak at ('tiny', 'b999_wd', step 1000)
    adamw m                                  0.473    0.465
    adamw v                                  0.505    0.511
    adamw p / m / v (adamw_dev_kernel: pm_adamw_dev and pm_adamw_segments, max_blocks 3)      0.355 / 0.465 / 0.511 -- the same
             figures: on the cases run from identical operands the two kernels gave the same bits in p, m, v and the shadow
    tick corrections (ulps)                  --       0        every h[7], h[8] equal to the float64 value rounded to f32
    loss scale                               exact    exact
    grad_stats sum of squares                0.136    0.136    at n = 4
    dgelu f32                                0.415    0.438
    dgelu bf16, in front of the store        0.384             stored: emu 0.962, device 0.994
    dgelu fp16, in front of the store        0.412             stored: emu 0.984, device 0.998
The two 16-bit dgelu figures lie between 0.9 and 1 by construction, not by accident: the store's half ulp, u_T |want|, is nearly all
of that bound and any correctly rounded store attains it on some value of a table this dense (the emulation does as well); in front
of the store the kernel's arithmetic uses under half of its share.
The ten wrong variants of VARIANTS exceed 1 by factors from 621 (weight decay after the update) to 1e12 on the cases named in
tests/test_optim_ref_cpu.py; the old shadow differs in bits.
"""
import math

import numpy as np
import torch

from attention_ref import DTYPES, U, ratio, rel  # noqa: F401  (re-exported: the tests take them from here)
from gemm_ref import G_DPHI, dgelu64
from rowops_ref import U32, equal_bits, store_bound  # noqa: F401

f32 = torch.float32
STRIDE = 16            # floats per hyper record (kHyperStride)
SATURATED = 16777216.0  # 2^24: the f32 step counter stays here


def _f32(x):
    return float(np.float32(x))


def bias_corrections(beta1, beta2, step):
    """(bc1, rsqrt_bc2) as the host of pm_adamw and the tick kernels store them: float64 from the f32 betas, rounded to f32."""
    b1, b2 = _f32(beta1), _f32(beta2)
    return _f32(1.0 - math.pow(b1, step)), _f32(1.0 / math.sqrt(1.0 - math.pow(b2, step)))


def record(lr, beta1, beta2, eps, wd, grad_scale=1.0, inv_scale=0.0, step=0, skip=0.0):
    """One 16-float hyper record (f32, CPU) standing at `step` (bias corrections filled in for step >= 1)."""
    h = torch.zeros(STRIDE, dtype=f32)
    h[:7] = torch.tensor([lr, beta1, beta2, eps, wd, grad_scale, float(step)], dtype=torch.float64).to(f32)
    if step >= 1:
        h[7], h[8] = bias_corrections(beta1, beta2, step)
    h[9], h[10] = skip, inv_scale
    return h


def gscale(hyper):
    """hyper[5] * (hyper[10] != 0 ? hyper[10] : 1) in f32, as adamw_dev_kernel forms it."""
    h = hyper.detach().cpu().to(f32)
    return float(h[5] * (h[10] if float(h[10]) != 0.0 else torch.tensor(1.0, dtype=f32)))


def adamw_step(p, g, m, v, hyper):
    """One update in float64 from the f32 operands and the record as stored.  -> dict of float64 p, m, v and e_p, e_m, e_v."""
    h = hyper.detach().cpu().double().tolist()
    lr, b1, b2, eps, wd, bc1, rs = h[0], h[1], h[2], h[3], h[4], h[7], h[8]
    gs, u = gscale(hyper), U32
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g * gs
    a, b = b1 * m, (1.0 - b1) * gr
    m1, e_m = a + b, 4 * u * (a.abs() + b.abs())
    v1 = b2 * v + (1.0 - b2) * gr * gr
    e_v = 5 * u * v1
    denom = v1.sqrt() * rs + eps
    q = m1 / denom
    e_q = q.abs() * (5.5 * u + u) + e_m / denom
    s = lr / bc1
    step = s * q
    e_step = s * e_q + 2 * u * step.abs()
    pd = p * (1.0 - lr * wd)
    p1 = pd - step
    e_p = 3 * u * pd.abs() + e_step + u * p1.abs()
    return dict(p=p1, m=m1, v=v1, e_p=e_p, e_m=e_m, e_v=e_v)


def adamw_ratios(p, m, v, ref):
    return {k: ratio(t, ref[k], ref["e_" + k]) for k, t in (("p", p), ("m", m), ("v", v))}


VARIANTS = ("eps_in_sqrt", "eps_times_rsqrt_bc2", "bc_step_plus_1", "bc_step_minus_1", "wd_after_update", "l2_decay",
            "v_unscaled", "inv_scale_ignored", "m_beta2", "shadow_pre_update")


def adamw_f32(p, g, m, v, hyper, shadow_dtype=None, variant=None):
    """The kernels' expression in torch f32 on the CPU, one rounding per operation (no fused multiply-add), and the wrong variants
    the CPU test rejects.  -> dict of f32 p, m, v (and shadow).  Also the NaN / Inf pattern the device test expects where a gradient is
    not finite."""
    h = hyper.detach().cpu().to(f32)
    p, g, m, v = (t.detach().cpu().to(f32) for t in (p, g, m, v))
    one = torch.tensor(1.0, dtype=f32)
    lr, b1, b2, eps, wd, bc1, rs = h[0], h[1], h[2], h[3], h[4], h[7], h[8]
    gs = torch.tensor(gscale(h), dtype=f32)
    if variant == "inv_scale_ignored":
        gs = h[5]
    if variant in ("bc_step_plus_1", "bc_step_minus_1"):
        c = bias_corrections(float(b1), float(b2), int(h[6]) + (1 if variant == "bc_step_plus_1" else -1))
        bc1, rs = torch.tensor(c[0], dtype=f32), torch.tensor(c[1], dtype=f32)
    gr = g * gs
    if variant == "l2_decay":
        gr = gr + wd * p
        pd = p
    elif variant == "wd_after_update":
        pd = p
    else:
        pd = p * (one - lr * wd)
    m1 = (b2 if variant == "m_beta2" else b1) * m + (one - b1) * gr
    gv = g if variant == "v_unscaled" else gr
    v1 = b2 * v + (one - b2) * gv * gv
    if variant == "eps_in_sqrt":
        denom = torch.sqrt(v1 + eps) * rs
    elif variant == "eps_times_rsqrt_bc2":
        denom = (torch.sqrt(v1) + eps) * rs
    else:
        denom = torch.sqrt(v1) * rs + eps
    p1 = pd - (lr / bc1) * (m1 / denom)
    if variant == "wd_after_update":
        p1 = p1 * (one - lr * wd)
    out = dict(p=p1, m=m1, v=v1)
    if shadow_dtype is not None:
        out["shadow"] = (p if variant == "shadow_pre_update" else p1).to(shadow_dtype)
    return out


# ------------------------------------------------------------------------------------------------ tick
def tick(rec):
    """What a tick leaves in slots 6, 7, 8 of a record (a list / tensor of its 16 f32): (step, bc1, rsqrt_bc2), or None when the
    record's skip flag is set (nothing is written)."""
    r = [float(x) for x in rec]
    if r[9] != 0.0:
        return None
    step = _f32(r[6] + 1.0)   # f32 addition: 16 777 216 + 1 rounds back to 16 777 216
    return (step,) + bias_corrections(r[1], r[2], step)


def ulps_apart(got, want):
    """|difference| in units of the last place between f32 tensors of one sign (bit patterns are ordered like the values)."""
    return (got.contiguous().view(torch.int32).long() - want.contiguous().view(torch.int32).long()).abs()


# ------------------------------------------------------------------------------------------------ loss scale
def loss_scale_update(state, stats, growth, backoff, interval):
    """pm_loss_scale_update in f32 scalar arithmetic.  state: six floats (scale, growth tracker, found_inf, skipped steps, steps,
    1 / scale used); stats: (sum of squares, #NaN, #Inf).  -> (new state [6 floats], found, 1 / scale): the last two are what slots 9
    and 10 of every group's record receive."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        s = [f(x) for x in state]
        scale, tracker = s[0], s[1]
        found = f(1.0) if f(stats[1]) + f(stats[2]) > 0 else f(0.0)
        inv = f(1.0) / scale
        s[2], s[4], s[5] = found, s[4] + f(1.0), inv
        if found != 0:
            s[0], s[1], s[3] = scale * f(backoff), f(0.0), s[3] + f(1.0)
        else:
            t = tracker + f(1.0)
            if t == f(interval):
                grown = scale * f(growth)
                s[0], s[1] = (grown if np.isfinite(grown) else scale), f(0.0)
            else:
                s[1] = t
    return [float(x) for x in s], float(found), float(inv)


# ------------------------------------------------------------------------------------------------ grad stats
def grad_stats_grid(n):
    """(G, k): the workgroups of pm_grad_stats at n elements (one per 256 vectors, at most 1024, at least 1) and the most terms one
    thread adds (4 per trip of its grid-stride loop, + 1 for a tail element)."""
    nvec = n >> 2
    G = min(max(-(-nvec // 256), 1), 1024)
    return G, 4 * -(-nvec // (G * 256)) + (1 if n & 3 else 0)


def grad_stats(g, prior=None):
    """-> dict of float64 ss (prior included), exact counts nan / inf (prior included), and e_ss."""
    g64 = g.double()
    p = [0.0, 0.0, 0.0] if prior is None else [float(x) for x in prior]
    fin = torch.where(torch.isfinite(g64), g64, torch.zeros_like(g64))
    T = abs(p[0]) + float((fin * fin).sum())
    G, k = grad_stats_grid(g.numel())
    return dict(ss=p[0] + float((fin * fin).sum()), nan=p[1] + int(torch.isnan(g).sum()), inf=p[2] + int(torch.isinf(g).sum()),
                e_ss=(k + 9 + G) * U32 * T, finite=bool(torch.isfinite(g).all()))


# ------------------------------------------------------------------------------------------------ dgelu
def dgelu(dy, pre, prec):
    """pm_dgelu from its operands (of the activation type).  -> (want, bound) in float64."""
    want = dy.double() * dgelu64(pre.double())
    return want, store_bound(dy.double().abs() * G_DPHI + 2 * U32 * want.abs(), want, prec)
