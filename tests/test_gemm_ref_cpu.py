"""The element-wise GEMM bound of tests/gemm_ref.py is neither too tight nor too loose (CPU only).

* An emulation of the kernels' arithmetic in float32 -- products of a 16-element k-group summed in f32, groups chained in k order,
  k-slices summed slab by slab in slice order, the epilogue in f32 (GELU by a float32 restatement of gelu_parts2: same constants,
  same order), then round to nearest even -- stays inside the bound on every case of tests/gemm_cases.py in both operand regimes,
  with margin: every term that is DERIVED (b_acc, the Phi / gelu' terms) is held to 0.9, i.e. the value in front of the final
  16-bit rounding to 0.9 of the bound without its rounding term, and an f32 output to 0.9 of its whole bound.  The rounding term
  u |want| of a 16-bit output has no margin to assert: round to nearest attains it at the bottom of every binade (want = 1 + 2^-8
  in bf16 errs by 2^-8), so the stored value is held to the bound itself (< 1; the peaks are 0.99+, docs/EXPERIMENT_LOG.md).
* G_PHI and G_DPHI against float64 erf over every bf16 and fp16 value of [-12, 12].
* Six wrong variants of the emulation each exceed the bound on a case of the table; which of them the old norm-wise measure lets
  through at the scaled operands is stated and asserted in test_wrong_variants_are_rejected."""
import math

import numpy as np
import pytest
import torch

import gemm_cases as G
import gemm_ref as R

F32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def gelu_parts_f32(x):
    """gelu_parts2 of pm_common.h on a float32 array: (Phi, exp(-x^2 / 2))."""
    x = x.astype(F32)
    ax = np.abs(x)
    t = F32(1.0) / _fma(ax, np.full_like(ax, F32(0.2316418882)), F32(1.0))
    e = np.exp2((x * F32(-0.72134752044448170368)) * x).astype(F32)
    p = np.full_like(x, F32(1.061405429))
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, F32(c))
    half_erfc = ((p * F32(0.5)) * t) * e
    return np.where(x >= 0, F32(1.0) - half_erfc, half_erfc).astype(F32), e


def gelu_f32(x):
    cdf, _ = gelu_parts_f32(x)
    return x.astype(F32) * cdf


def dgelu_f32(x):
    cdf, e = gelu_parts_f32(x)
    return _fma(x.astype(F32) * F32(0.39894228040143267794), e, cdf)


def _round(v, dt, truncate=False):
    """float32 tensor -> dt (round to nearest even; truncate: towards zero, the wrong store of variant (a))."""
    if dt == "fp32":
        return v
    r = v.to(R.TORCH[dt])
    if truncate:
        over = r.float().abs() > v.abs()
        r = torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r)
    return r


def _chain(A, B, k0, k1):
    acc = torch.zeros(A.shape[0], B.shape[0])
    for g in range(k0, k1, 16):
        acc += A[:, g:min(g + 16, k1)] @ B[:, g:min(g + 16, k1)].t()
    return acc


def _sample(n):
    """All indices of a short axis; of a long one the first 96 (every operand scale, whole wave tiles), the last 96 (the ragged
    tile) and every 61st between."""
    if n <= 320:
        return torch.arange(n)
    return torch.unique(torch.cat([torch.arange(96), torch.arange(96, n - 96, 61), torch.arange(n - 96, n)]))


def emulate(c, o, rows=None, cols=None, wrong=None):
    """-> {output: (float32 value in front of the final rounding or None, stored tensor)} of case c on operands o (tests/gemm_ref.py),
    restricted to rows / cols of the output."""
    rows = torch.arange(c.M) if rows is None else rows
    cols = torch.arange(c.N) if cols is None else cols
    A, B = o["A"].float()[rows], o["B"].float()[cols]
    unit = 32 if c.family == "wgrad" else (64 if c.in_dt != "fp32" else 32)
    nk = -(-c.K // unit)
    ks = -(-nk // c.split)
    slabs = []
    for s in range(c.split):
        k0, k1 = s * ks * unit, min((s + 1) * ks * unit, c.K)
        if wrong == "c" and s == c.split - 1:
            k1 -= unit                     # (c) the last k-step of the last slice dropped
        slabs.append(_chain(A, B, k0, k1))
    sub = lambda t: t[rows][:, cols]
    if c.split > 1:                        # the reduce launch: C_in (ACCUM) or 0, then the slabs in slice order
        v = sub(o["base"]).clone() if c.epi == "accum" else torch.zeros_like(slabs[0])
        for s in slabs:
            v = v + s
        return {"C": (None, v)}
    v = slabs[0]
    if c.bias:
        bias = o["bias"][cols].clone()
        if wrong == "b":
            bias[-4:] = 0                  # (b) bias not added in the last 4 columns of the ragged tile
        v = v + bias
    if c.epi == "store":
        out = {"C": (v, _round(v, c.c_dt, truncate=wrong == "a"))}          # (a) a 16-bit store that truncates
    elif c.epi in ("resid", "accum"):
        r = sub(o["base"])
        w = r + v
        if wrong == "f":                   # (f) residual added twice in the rows beyond the last full tile
            beyond = rows >= (c.M // c.tile[0]) * c.tile[0]
            w[beyond] = (r + w)[beyond]
        out = {"C": (None, w)}
    elif c.epi == "gelu":
        aux = _round(v, c.in_dt)
        x = v if wrong == "e" else aux.float()   # (e) GELU of the unrounded pre-activation
        g = torch.from_numpy(gelu_f32(x.numpy()))
        out = {"aux": (v, aux), "C": (g, _round(g, c.c_dt))}
    else:
        g = v * torch.from_numpy(dgelu_f32(sub(o["pre"]).float().numpy()))
        out = {"C": (g, _round(g, c.c_dt))}
    if wrong == "d":                       # (d) two rows 32 apart exchanged inside a wave tile, both at scale <= 2^-8
        for name, (pre, st) in out.items():
            st = st.clone()
            st[[9, 41]] = st[[41, 9]]
            out[name] = (pre, st)
    return out


def judge(c, o, em, rows=None, cols=None):
    """-> {output: (stored err / bound, err in front of the rounding / bound without the rounding term or None, old norm-wise
    measure / its bound, text)}"""
    rows = torch.arange(c.M) if rows is None else rows
    cols = torch.arange(c.N) if cols is None else cols
    acc, T = R.products(o["A"][rows], o["B"][cols])
    sub = lambda t: t[rows][:, cols]
    exp = R.expected(c.epi, c.in_dt, c.c_dt, c.K, acc, T, bias=o["bias"][cols] if c.bias else None, base=sub(o["base"]),
                     pre=sub(o["pre"]), aux_got=em["aux"][1] if "aux" in em else None)
    res = {}
    for name, (want, bound, terms) in exp.items():
        pre, st = em[name]
        ratio, _, text = R.check(st, want, bound, terms, f"{G.case_id(c)} {name}")
        derived = None
        if "rounding" in terms:
            rest = {k: t for k, t in terms.items() if k != "rounding"}
            if name == "C" and c.epi in ("gelu", "dgelu"):   # the f32 product x Phi / acc gelu' in front of the 16-bit rounding
                rest["f32 product"] = R.U["fp32"] * want.abs()
            derived = R.check(pre, want, sum(rest.values()), rest, f"{G.case_id(c)} {name} (unrounded)")[0]
        old = R.rel(st, want) / R.old_bound(c.in_dt, c.in_dt if name == "aux" else c.c_dt, c.epi, c.K)
        res[name] = (ratio, derived, old, text)
    return res


@pytest.mark.parametrize("regime", R.REGIMES)
def test_emulation_stays_inside_the_bound(regime):
    """Every case of the table: the derived terms with a margin of 0.9, the stored 16-bit value under the bound (see the module
    docstring), the old norm-wise bound beside it.  Long axes are sampled (_sample)."""
    peak = {}
    for c in G.CASES:
        o = R.operands(c.M, c.N, c.K, c.in_dt, regime)
        rows, cols = _sample(c.M), _sample(c.N)
        for name, (ratio, derived, old, text) in judge(c, o, emulate(c, o, rows, cols), rows, cols).items():
            key = (c.family, "16-bit" if derived is not None else "f32")
            margin = derived if derived is not None else ratio
            p = peak.setdefault(key, [0.0, 0.0])
            p[0], p[1] = max(p[0], ratio), max(p[1], margin)
            assert ratio < 1.0 and margin < 0.9, text + f" derived terms {margin:.3f}"
            assert old < 1.0, text + f" norm-wise measure / its bound {old:.3f}"
    for key, (ratio, margin) in sorted(peak.items()):
        print(f"emulation {regime} {key[0]:8s} {key[1]:6s} C: peak err/bound {ratio:.3f}, derived terms {margin:.3f}")


def _all_values(dt):
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(R.TORCH[dt]).double()
    return x[torch.isfinite(x) & (x.abs() <= 12)].numpy()


def test_gelu_constants_hold():
    """The float32 restatement of gelu_parts2 against float64 erf on every bf16 and fp16 value of [-12, 12]: the peak absolute
    errors of Phi and gelu' stay under 0.9 of G_PHI / G_DPHI."""
    peak_phi = peak_d = 0.0
    for dt in ("bf16", "fp16"):
        x = _all_values(dt)
        assert x.size > 30000
        erf = np.vectorize(math.erf)
        phi = 0.5 * (1.0 + erf(x / math.sqrt(2.0)))
        d = phi + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        peak_phi = max(peak_phi, np.abs(gelu_parts_f32(x)[0].astype(np.float64) - phi).max())
        peak_d = max(peak_d, np.abs(dgelu_f32(x).astype(np.float64) - d).max())
    print(f"peak |Phi error| {peak_phi:.3e} (G_PHI {R.G_PHI:.1e}), peak |gelu' error| {peak_d:.3e} (G_DPHI {R.G_DPHI:.1e})")
    assert peak_phi < 0.9 * R.G_PHI and peak_d < 0.9 * R.G_DPHI


def _find(**want):
    for c in G.CASES:
        if all(getattr(c, k) == v for k, v in want.items()):
            return c
    raise KeyError(want)


# wrong variant -> the case it is shown on, and whether the old norm-wise measure lets it through at the scaled operands
WRONG = {
    "a": (dict(family="ring", cfg=8, layout="nt", in_dt="bf16", epi="store", N=264, K=64), True),
    "b": (dict(family="ring", cfg=9, layout="nt", in_dt="bf16", epi="store", N=260), False),
    "c": (dict(family="lds128", in_dt="bf16", epi="store", split=2), False),
    "d": (dict(family="ring", cfg=8, layout="nt", in_dt="bf16", epi="store", N=264, K=64), True),
    "e": (dict(family="ring", cfg=8, layout="nt", in_dt="bf16", epi="gelu", N=264, K=64), True),
    "f": (dict(family="ring", cfg=25, in_dt="bf16", epi="resid", N=264, K=64), False),
}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_are_rejected(wrong):
    """Each wrong variant of the emulation exceeds the element-wise bound, in both regimes.  At the scaled operands the old
    norm-wise measure lets (a) the truncating store, (d) the exchanged small rows and (e) GELU of the unrounded pre-activation
    through -- the point of the element-wise bound -- and catches (b), (c) and (f): bias and residual are at unit scale, so
    a missing bias or a doubled residual is as large as the largest elements, and a dropped k-step removes 1 / 17 of every sum."""
    want, old_passes = WRONG[wrong]
    c = _find(**want)
    for regime in R.REGIMES:
        o = R.operands(c.M, c.N, c.K, c.in_dt, regime)
        good = judge(c, o, emulate(c, o))
        bad = judge(c, o, emulate(c, o, wrong=wrong))
        assert all(r[0] < 1.0 for r in good.values())
        ratio, _, old, text = bad["C"]
        print(f"({wrong}) {regime}: err/bound {ratio:.3g}, norm-wise measure / its bound {old:.3g}")
        assert ratio > 1.0, text
        if regime == "scaled":
            assert (old < 1.0) == old_passes, text
