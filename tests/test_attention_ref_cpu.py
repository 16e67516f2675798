"""The element-wise attention bound of tests/attention_ref.py, on the CPU: a float32 emulation of the kernels' rounding points
(pm_attention.hip: P rounded in front of P V and P^T dO, dS in front of dS K and dS^T Q, one store in the activation type,
everything else f32) stays under 0.9 of it, and four wrong kernels exceed it -- one of which (P and dS truncated, not rounded)
the norm-wise bounds of tests/test_gpu_ops.py accept.  oracle/vit_bf16_grad_sim.py `_Attention` has the same rounding points but
takes neither `out` / `lse` as inputs nor a wrong variant, hence the few lines here."""
import pytest
import torch

import attention_cases as C
import attention_ref as R

SHAPES = [(2, 197, 3, 64), (2, 50, 2, 64), (2, 257, 4, 32), (1, 225, 2, 64), (2, 65, 3, 80)]


def _round(x, prec):
    return x.to(R.DTYPES[prec]).float()


def _trunc(x, prec):
    assert prec == "bf16"
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(case, prec, qkv, dout, o_in=None, lse_in=None, mutant=None):
    """float32, the kernels' rounding points; returns out, lse, dqkv in the kernels' layouts (the backward on o_in / lse_in, or
    chained on its own forward when they are None).  mutant: None or
      "truncate"   P and dS truncated to the type instead of rounded to nearest
      "delta64"    delta summed over the first 64 features of a wider head
      "drop_last"  the last key left out of O and dQ, the last query out of dK and dV
      "pad_key"    one padded key (a zero K row: score 0) counted in the forward row sum."""
    B, N, H, dh = case
    scale = dh ** -0.5
    q, k, v = (t.float() for t in R.split_qkv(qkv, B, N, H, dh))
    do = R.heads(dout, B, N, H, dh).float()
    rp = (lambda x: _trunc(x, prec)) if mutant == "truncate" else (lambda x: _round(x, prec))
    nk = N - 1 if mutant == "drop_last" else N
    s = q @ k.transpose(1, 2)
    m = s.amax(-1, keepdim=True)
    p = torch.exp((s - m) * scale)
    l = p.sum(-1, keepdim=True)
    if mutant == "pad_key":
        l = l + torch.exp((0.0 - m) * scale)
    o = _round((rp(p)[:, :, :nk] @ v[:, :nk]) / l, prec)
    lse = (m * scale + torch.log(l)).squeeze(-1)
    oi = o if o_in is None else R.heads(o_in, B, N, H, dh).float()
    ls = lse if lse_in is None else lse_in.reshape(B * H, N).float()
    nd = 64 if mutant == "delta64" else dh
    delta = (do[..., :nd] * oi[..., :nd]).sum(-1, keepdim=True)
    p = torch.exp(s * scale - ls[..., None])
    ds = rp(p * (do @ v.transpose(1, 2) - delta) * scale)
    dq = ds[:, :, :nk] @ k[:, :nk]
    dk = ds.transpose(1, 2)[:, :, :nk] @ q[:, :nk]
    dv = rp(p).transpose(1, 2)[:, :, :nk] @ do[:, :nk]
    tok = lambda x: R.tokens(x, B, N, H, dh)
    dqkv = _round(torch.cat([tok(dq), tok(dk), tok(dv)], dim=-1), prec)
    return tok(o), lse.reshape(B, H, N), dqkv


def _ratios(case, prec, regime="random", mutant=None, chained=False):
    """Largest err / bound of out, dq, dk, dv (the backward on the float64 O rounded to the type and the float64 lse, or chained)."""
    B, N, H, dh = case
    qkv, dout = C.inputs(case, prec, regime)
    fwd = R.reference(qkv, B, N, H, dh)
    if chained:
        out, lse, dqkv = emulate(case, prec, qkv, dout, mutant=mutant)
        o_in = out.to(R.DTYPES[prec])     # the reference delta is taken from that out
    else:
        o_in = fwd["out"].to(R.DTYPES[prec])
        out, lse, dqkv = emulate(case, prec, qkv, dout, o_in, fwd["lse"].float(), mutant=mutant)
    ref = R.reference(qkv, B, N, H, dh, dout, o_in)
    r = {"out": R.out_ratio(out, ref, N, prec), **R.grad_ratios(dqkv, ref, N, prec)}
    norm = {"out": R.rel(out, ref["out"]), "lse": R.rel(lse, ref["lse"])}
    for j, name in enumerate(("dq", "dk", "dv")):
        part = lambda x: x.reshape(B, N, 3, H * dh)[:, :, j]
        norm[name] = R.rel(part(dqkv), part(ref["dqkv"]))
    return r, norm


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_emulation_is_the_oracles_attention(prec):
    """Chained, the emulation above is oracle/vit_bf16_grad_sim.py `_Attention` with every rounding on (loss scale 1), which leaves
    the store of the gradients to its caller: the same values to one rounding of the type."""
    from oracle.vit_bf16_grad_sim import Rounding, _Attention
    case = B, N, H, dh = (2, 50, 2, 64)
    qkv, dout = C.inputs(case, prec)
    out, _, dqkv = emulate(case, prec, qkv, dout)
    q, k, v = (t.float().reshape(B, H, N, dh).requires_grad_(True) for t in R.split_qkv(qkv, B, N, H, dh))
    o = _Attention.apply(q, k, v, Rounding(fwd_dtype=prec, bwd_dtype=prec, loss_scale=1.0))
    o.backward(R.heads(dout, B, N, H, dh).float().reshape(B, H, N, dh))
    tok = lambda x: R.tokens(x.reshape(B * H, N, dh), B, N, H, dh)
    want = torch.cat([tok(q.grad), tok(k.grad), tok(v.grad)], dim=-1)
    u = R.U[prec]
    assert bool(((out - tok(o.detach())).abs() <= u * out.abs()).all())
    assert bool(((dqkv - want).abs() <= u * want.abs() + 2.0 ** -24).all())


@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", SHAPES, ids=C.case_id)
def test_bound_accepts_the_kernels_rounding_points(case, prec, chained):
    r, _ = _ratios(case, prec, chained=chained)
    print(f"{case} {prec} chained={chained}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()))
    assert max(r.values()) < 0.9, r


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_bound_accepts_identical_keys(prec):
    """The regime tests/test_gpu_attention_edges.py holds to the element-wise bound: the emulation must stay under 0.9 of it there."""
    r, _ = _ratios(C.IDENTICAL_KEYS, prec, regime="identical_keys")
    print(f"identical keys {prec}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()))
    assert max(r.values()) < 0.9, r


def test_softmax_spike_cannot_take_the_bound():
    """Why the spike regime keeps the norm-wise bounds: a one-hot row has dS = 0 exactly in float64 (bound 0), while the float32
    evaluation of dP - delta leaves about 1e-6 -- correct arithmetic exceeds the element-wise bound there."""
    r, norm = _ratios(C.SPIKE, "bf16", regime="spike")
    assert max(r["dq"], r["dk"]) > 0.9, r
    assert norm["out"] < R.NORM16["bf16"]["out"] and max(norm[n] for n in ("dq", "dk", "dv")) < R.NORM16["bf16"]["grad"], norm


@pytest.mark.parametrize("case", [(2, 197, 3, 64), (2, 257, 4, 32), (2, 65, 3, 80)], ids=C.case_id)
def test_bound_rejects_truncated_p_and_ds(case):
    """(a) Truncation errs by up to 2^-7 per term, all of one sign, where rounding to nearest errs by at most 2^-8: some element of
    some output exceeds the bound -- and the norm-wise bounds accept it, which is the reason this file exists."""
    r, norm = _ratios(case, "bf16", mutant="truncate")
    print(f"truncate {case}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()) + " | norm-wise " +
          " ".join(f"{n} {x:.1e}" for n, x in norm.items()))
    assert max(r.values()) > 1.0, r
    assert norm["out"] < R.NORM16["bf16"]["out"] and norm["lse"] < 1e-5, norm
    assert max(norm[n] for n in ("dq", "dk", "dv")) < R.NORM16["bf16"]["grad"], norm


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_bound_rejects_delta_over_64_of_80_features(prec):
    """(b)"""
    r, _ = _ratios((2, 65, 3, 80), prec, mutant="delta64")
    assert r["dq"] > 1.0 and r["dk"] > 1.0, r
    assert max(r["out"], r["dv"]) < 0.9, r      # delta enters dS only


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [(2, 50, 2, 64), (1, 225, 2, 64)], ids=C.case_id)
def test_bound_rejects_a_dropped_last_row(case, prec):
    """(c)"""
    r, _ = _ratios(case, prec, mutant="drop_last")
    assert min(r.values()) > 1.0, r


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_an_unmasked_padded_key_is_rejected(prec):
    """(d) N = 193: one real key in the last tile, the key behind it (a zero K row: score 0) counted in the forward row sum.  Every
    row sum grows by exp(-max score): 1.6e-4 of the largest lse, sixteen times its 1e-5 bound, in either type.  On `out` the same
    factor is a relative error of at most exp(-max) / l on every element of a row: fp16's element-wise bound (2^-11) rejects it,
    bf16's (2^-8) cannot see it at these inputs -- there the lse bound is what catches an unmasked key."""
    r, norm = _ratios((2, 193, 3, 64), prec, mutant="pad_key")
    print(f"pad_key {prec}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()) + f" | lse norm-wise {norm['lse']:.1e}")
    assert norm["lse"] > 1e-5, norm
    if prec == "fp16":
        assert r["out"] > 1.0, r
