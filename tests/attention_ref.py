"""Float64 restatement of the attention core and the element-wise error bound of its 16-bit modes (not a test module): what
pm_attention_fwd / pm_attention_bwd compute, from the operands as the kernels see them (already rounded to the activation type),
in plain torch on whichever device the operands live.  tests/test_attention_ref_cpu.py holds the bound to a float32 emulation of the
kernels' rounding points (and to four wrong ones); tests/test_gpu_attention_edges.py holds the kernels to it.

Layouts are the kernels': qkv [B, N, 3 H dh] (q | k | v, each H heads of dh), out / dout [B, N, H dh], lse / delta [B, H, N],
dqkv like qkv."""
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# unit round-off of one round-to-nearest: bf16 keeps 8 significant bits, fp16 11
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
F32_BOUNDS = {"out": 2e-5, "lse": 1e-5, "grad": 5e-5}   # f32 mode: norm-wise (rel below), as tests/test_gpu_ops.py has them
NORM16 = {"bf16": {"out": 1.5e-2, "grad": 3e-2}, "fp16": {"out": 1.5e-2 * 1.5 / 8, "grad": 3e-2 * 1.5 / 8}}  # the old 16-bit bounds


def heads(x, B, N, H, dh):
    """[B, N, H dh] -> [B H, N, dh]."""
    return x.reshape(B, N, H, dh).permute(0, 2, 1, 3).reshape(B * H, N, dh)


def tokens(x, B, N, H, dh):
    """[B H, N, dh] -> [B, N, H dh]."""
    return x.reshape(B, H, N, dh).permute(0, 2, 1, 3).reshape(B, N, H * dh)


def split_qkv(qkv, B, N, H, dh):
    """qkv [B, N, 3 H dh] -> q, k, v, each [B H, N, dh]."""
    return tuple(heads(t, B, N, H, dh) for t in qkv.reshape(B, N, 3, H * dh).unbind(2))


def rel(got, want):
    """Norm-wise: the largest absolute error over the largest reference element."""
    got, want = got.double(), want.double()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def reference(qkv, B, N, H, dh, dout=None, o_in=None, chunk=64):
    """Float64 forward (and, with dout and o_in, backward) in chunks of at most `chunk` heads.  Returns a dict of float64 tensors:
      out, lse                P = softmax(Q K^T dh^-1/2), lse = its log-sum-exp, out = P V
      t_out                   P |V|: the sum of absolute terms behind every element of out
      m_out                   max |V| of the element's head (the fp16 subnormal term of bound16)
    and for the backward, with delta = rowsum(dout * o_in), dP = dO V^T, dS = P (dP - delta) dh^-1/2:
      delta, dqkv             dQ = dS K | dK = dS^T Q | dV = P^T dO
      t_dqkv                  |dS| |K| | |dS|^T |Q| | P^T |dO|
      m_dqkv                  max |K| | max |Q| | max |dO| of the element's head."""
    scale = dh ** -0.5
    q, k, v = split_qkv(qkv, B, N, H, dh)
    bwd = dout is not None
    if bwd:
        do_h, oi_h = heads(dout, B, N, H, dh), heads(o_in, B, N, H, dh)
    acc = {n: [] for n in ("out", "t_out", "lse", "m_out", "delta", "dq", "dk", "dv", "t_dq", "t_dk", "t_dv", "m_dq", "m_dk", "m_dv")}
    hmax = lambda x: x.abs().amax(dim=(1, 2), keepdim=True).expand(-1, 1, dh)   # per head, [c, 1, dh]
    for c0 in range(0, B * H, chunk):
        sl = slice(c0, min(c0 + chunk, B * H))
        qc, kc, vc = q[sl].double(), k[sl].double(), v[sl].double()
        s = (qc @ kc.transpose(1, 2)) * scale
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse[..., None])
        acc["out"].append(p @ vc)
        acc["t_out"].append(p @ vc.abs())
        acc["lse"].append(lse)
        acc["m_out"].append(hmax(vc))
        if not bwd:
            continue
        do, oi = do_h[sl].double(), oi_h[sl].double()
        delta = (do * oi).sum(-1)
        ds = p * (do @ vc.transpose(1, 2) - delta[..., None]) * scale
        pt, dst = p.transpose(1, 2), ds.transpose(1, 2)
        acc["delta"].append(delta)
        acc["dq"].append(ds @ kc)
        acc["dk"].append(dst @ qc)
        acc["dv"].append(pt @ do)
        acc["t_dq"].append(ds.abs() @ kc.abs())
        acc["t_dk"].append(dst.abs() @ qc.abs())
        acc["t_dv"].append(pt @ do.abs())
        acc["m_dq"].append(hmax(kc))
        acc["m_dk"].append(hmax(qc))
        acc["m_dv"].append(hmax(do))
    cat = lambda n: torch.cat(acc[n], 0)
    tok = lambda n, rows=N: tokens(cat(n), B, rows, H, dh)
    ref = {"out": tok("out"), "t_out": tok("t_out"), "m_out": tok("m_out", 1), "lse": cat("lse").reshape(B, H, N)}
    if bwd:
        ref["delta"] = cat("delta").reshape(B, H, N)
        ref["dqkv"] = torch.cat([tok("dq"), tok("dk"), tok("dv")], dim=-1)
        ref["t_dqkv"] = torch.cat([tok("t_dq"), tok("t_dk"), tok("t_dv")], dim=-1)
        ref["m_dqkv"] = torch.cat([tok("m_dq", 1), tok("m_dk", 1), tok("m_dv", 1)], dim=-1)
    return ref


def bound16(want, t, m, N, prec):
    """|got - want| <= (u + 4 N 2^-24) (|want| + T) + s, element-wise, for the 16-bit modes.  From the kernels' documented rounding
    points (pm_attention.hip, header): P is rounded to the activation type in front of P V and P^T dO, dS in front of dS K and
    dS^T Q -- a relative error of at most u on every term, so u of the sum of absolute terms T; the output is stored once in the
    activation type -- u of |want| (to first order); everything else (scores, exp, row sums, delta, the accumulators) is f32 -- a
    few 2^-24 per term over the N terms of a row, 4 N 2^-24 of |want| + T.  fp16 adds the subnormal quantum
    2^-24 per rounded term and for the store: s = 2^-24 (1 + N max |other operand|); bf16 has f32's exponent range, s = 0.
    Holds for the online-softmax forward, the persistent forward and both backward families alike.  No safety factor."""
    s = 0.0 if prec == "bf16" else 2.0 ** -24 * (1.0 + N * m)
    return (U[prec] + 4.0 * N * 2.0 ** -24) * (want.abs() + t) + s


def ratio(got, want, bound):
    """Largest |got - want| / bound over the elements (0 where both are 0; inf where got is not finite)."""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return r.max().item()


def out_ratio(got, ref, N, prec):
    return ratio(got, ref["out"], bound16(ref["out"], ref["t_out"], ref["m_out"], N, prec))


def grad_ratios(got, ref, N, prec):
    """{"dq": .., "dk": .., "dv": ..}: the largest err / bound of each third of dqkv."""
    r = {}
    for j, name in enumerate(("dq", "dk", "dv")):
        part = lambda x: x.reshape(*x.shape[:-1], 3, -1)[..., j, :]
        want = part(ref["dqkv"])
        r[name] = ratio(part(got), want, bound16(want, part(ref["t_dqkv"]), part(ref["m_dqkv"]), N, prec))
    return r
