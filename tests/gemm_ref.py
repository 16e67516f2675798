"""Float64 reference and element-wise error bound of pm_gemm / pm_wgrad_group (not a test module).

Everything is computed from the operands as the kernel sees them (already rounded to the operand type), with plain torch on the
device the operands live on:

    acc  = A64 . B64^T                      T = |A|64 . |B|64^T (+ |bias|) (+ |resid| or |C_in|)
    want = the epilogue of acc in float64   (GELU: want_aux = acc + bias, want_C = gelu64(aux AS THE KERNEL STORED IT);
                                             dGELU: want = acc * gelu'64(pre))

Bound per element -- derived, no term is fitted to the kernel under test:

    b_acc = 2 (K + 2) 2^-24 T     16-bit products are exact in f32; each of the <= K + 2 additions (K products, bias, residual / C_in),
                                  in ANY order, costs at most one ulp of a partial sum that T bounds -- which also covers an
                                  accumulator that truncates (one ulp instead of half); in f32 mode each product rounds once (or
                                  not at all: fma), inside the same count.
    f32 C:      b = b_acc
    16-bit C:   b = u |want| + b_acc (+ 2^-25 for fp16: half of the smallest subnormal),   u = 2^-8 bf16, 2^-11 fp16: round to
                nearest.  A store that truncates errs by up to 2 u |want| and fails.
    GELU C:     b = u |want| + g |x| (+ 2^-25),  x = the stored pre-activation, g = G_PHI = the absolute error of Phi as gelu_parts
                computes it (Abramowitz-Stegun 7.1.26: 7.5e-8, plus its f32 chain); u = 2^-24 for an f32 C (the product x Phi)
    dGELU C:    b = u |want| + |gelu'(pre)| b_acc + |acc| g',   g' = G_DPHI likewise
G_PHI / G_DPHI are confirmed against float64 erf over every bf16 and fp16 value of [-12, 12] by tests/test_gemm_ref_cpu.py.

check() returns the worst err / b, its index and a text that names the element and the dominating term.  The old norm-wise measure
max|got - want| / max|want| (tests/test_gpu_ops.py) stays beside it: rel().

Operands that make the element-wise bound bite ("scaled" regime): N(0, 1) * 0.5 data, row m of A times 2^-(m mod 11), row n of B
times 2^-(n mod 7) -- exact in bf16 and f32, so T[m, n] spans 2^16 and a norm-wise measure sees only the rows and columns at scale
1.  fp16: its normal range ends at 2^-14, so the data is first floored at |x| >= 2^-6 and A's exponents run over m mod 9 (checked:
no element is subnormal, every scaling is exact; T spans 2^14).  Bias, residual, C_in and the dGELU pre-activation stay at unit scale.
The "uniform" regime is the old one: every row at scale 1."""
import math

import torch

TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}   # round to nearest: half an ulp of the format, relative
SUBNORMAL = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}          # half of fp16's smallest subnormal
# absolute error of Phi / of gelu' = Phi + x phi(x) as gelu_parts computes them in f32.  G_PHI: 7.5e-8 of the approximation + the
# f32 chain (rcp, exp2 of an argument rounded at |x^2 / 2 ln 2| <= 100, five fmas, 1 - half_erfc), taken as 4e-7.  G_DPHI: G_PHI +
# the pdf term, |x phi(x)| <= 0.242 at a relative error of ~ 8e-7 (the exponent's rounding times ln 2, three products) = 6e-7.
# Measured by tests/test_gemm_ref_cpu.py over every bf16 and fp16 value of [-12, 12] (float32 restatement against float64 erf):
# peak 2.65e-7 for Phi, 2.54e-7 for gelu' -- under the 0.9 the test asserts, which leaves the device's v_rcp_f32 / v_exp_f32 (about
# 1 ulp each) their room
G_PHI = 4e-7
G_DPHI = 6e-7
REGIMES = ("scaled", "uniform")
A_PERIOD, B_PERIOD = {"fp32": 11, "bf16": 11, "fp16": 9}, 7
FP16_FLOOR = 2.0 ** -6


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def rel(got, want):
    """The old norm-wise measure of tests/test_gpu_ops.py."""
    got, want = got.double(), want.double()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-12)).item()


def old_bound(in_dt, c_dt, epi, K):
    """The norm-wise bounds tests/test_gpu_ops.py asserts, per output type: 1e-2 for a bf16 C (fp16: x 1.5 / 8); for an f32 C the
    tightest of its GEMM tests, test_gemm_layouts' 2e-5 sqrt(K / 32) (16-bit operands) / 2e-6 sqrt(K / 32) (f32 operands) -- with
    test_gemm_epilogues' 3e-6 as the floor where the f32 C went through GELU / dGELU."""
    if c_dt != "fp32":
        return {"bf16": 1e-2, "fp16": 1e-2 * 1.5 / 8}[c_dt]
    b = (2e-6 if in_dt == "fp32" else 2e-5) * math.sqrt(K / 32)
    return max(b, 3e-6) if epi in ("gelu", "dgelu") else b


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _operand(rows, K, dt, seed, period, regime):
    """[rows][K] of the operand type: N(0, 1) * 0.5, row r scaled by 2^-(r mod period) in the scaled regime (exactly: asserted)."""
    x = _randn((rows, K), seed) * 0.5
    if dt == "fp16":
        x = torch.where(x.abs() < FP16_FLOOR, torch.sign(x) * FP16_FLOOR, x)
    x = x.to(TORCH[dt])
    if regime == "scaled":
        e = (torch.arange(rows) % period).to(torch.float32)
        s = torch.exp2(-e)[:, None]
        y = (x.float() * s).to(TORCH[dt])
        assert torch.equal(y.float() / s, x.float()), "the row scaling is not exact in " + dt
        x = y
    if dt == "fp16":
        nz = x.float().abs()[x != 0]
        assert nz.numel() == 0 or nz.min().item() >= 2.0 ** -14, "an fp16 operand element is subnormal"
    return x


_operands = {}


def operands(M, N, K, dt, regime, device="cpu"):
    """A [M][K], B [N][K] of the operand type, bias f32 [N], base f32 [M][N] (residual / C_in), pre [M][N] of the operand type
    (the saved pre-activation of dGELU).  Seeded by nothing but the arguments; made once per device and never written to."""
    key = (M, N, K, dt, regime, str(device))
    if key not in _operands:
        if len(_operands) > 24:
            _operands.clear()
        o = dict(A=_operand(M, K, dt, 1000, A_PERIOD[dt], regime), B=_operand(N, K, dt, 1001, B_PERIOD, regime),
                 bias=_randn((N,), 1002), base=_randn((M, N), 1003), pre=_randn((M, N), 1004).to(TORCH[dt]))
        _operands[key] = {k: v.to(device) for k, v in o.items()}
    return _operands[key]


def products(A, B):
    """(acc, T) in float64 from A [M][K], B [N][K] of any type."""
    a, b = A.double(), B.double()
    return a @ b.t(), a.abs() @ b.abs().t()


def b_acc(T, K):
    return 2.0 * (K + 2) * 2.0 ** -24 * T


def expected(epi, in_dt, c_dt, K, acc, T, bias=None, base=None, pre=None, aux_got=None):
    """-> {output name: (want, bound, {term name: tensor})} for one epilogue.  bias / base / pre: what the call was given (None: not
    given); aux_got: the pre-activation the kernel stored (GELU with aux).  All float64, on acc's device."""
    if bias is not None:
        acc_b, T = acc + bias.double(), T + bias.double().abs()
    else:
        acc_b = acc
    u_c, sub = U[c_dt], SUBNORMAL[c_dt]

    def stored(want, terms, dt):  # a value with absolute error terms, then rounded to dt (f32: not rounded again)
        if dt != "fp32":
            terms = dict(terms, rounding=U[dt] * want.abs() + SUBNORMAL[dt])
        return want, sum(terms.values()), terms

    if epi == "store":
        return {"C": stored(acc_b, {"b_acc": b_acc(T, K)}, c_dt)}
    if epi in ("resid", "accum"):
        return {"C": stored(acc_b + base.double(), {"b_acc": b_acc(T + base.double().abs(), K)}, "fp32")}
    if epi == "gelu":
        out = {}
        out["aux"] = stored(acc_b, {"b_acc": b_acc(T, K)}, in_dt)
        x = aux_got.double()   # (the reference of C needs the pre-activation the kernel stored)
        want = gelu64(x)
        terms = {"rounding": u_c * want.abs() + sub, "phi": G_PHI * x.abs()}
        out["C"] = (want, sum(terms.values()), terms)
        return out
    if epi == "dgelu":
        d = dgelu64(pre.double())
        want = acc_b * d
        terms = {"rounding": u_c * want.abs() + sub, "b_acc": d.abs() * b_acc(T, K), "dphi": acc_b.abs() * G_DPHI}
        return {"C": (want, sum(terms.values()), terms)}
    raise ValueError(epi)


def check(got, want, bound, terms, what):
    """-> (worst err / bound, (m, n), text).  A non-finite got where want is finite counts as infinitely wrong."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = err / bound.clamp_min(1e-300)
    flat = int(ratio.argmax())
    m, n = divmod(flat, ratio.shape[1])
    r = ratio[m, n].item()
    top = max(terms, key=lambda t: terms[t][m, n].item())
    text = (f"{what}: worst err/bound {r:.3f} at [{m}, {n}]: got {got[m, n].item():.9g} want {want[m, n].item():.9g} "
            f"err {err[m, n].item():.3e} bound {bound[m, n].item():.3e} ({top} dominates)")
    return r, (m, n), text
