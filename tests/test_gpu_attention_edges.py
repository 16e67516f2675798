"""pm_attention_fwd / pm_attention_bwd at the edges of every instantiation (tests/attention_cases.py), against the float64 reference
and the element-wise bound of tests/attention_ref.py: the 16-bit modes are held to (u + 4 N 2^-24) (|want| + T) + s per element
(derived from the kernels' rounding points, no safety factor; tests/test_attention_ref_cpu.py), f32 mode to the norm-wise bounds of
tests/test_gpu_ops.py.  The backward is tested on reference-made `out` / `lse` as well as chained to the kernel's own; every output
lies between guards; heads are compared with the same head run alone, runs with a second run.  Each test prints its largest
err / bound per output (`pytest -s`); docs/EXPERIMENT_LOG.md has the table."""
import ctypes

import pytest
import torch

import attention_cases as C
import attention_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, FILL = 256, 7.0
FAMILY = {0: "head", 1: "persistent", 2: "split", 3: "fused"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _k(prec):
    from ssl4polyp_amd.engine import Kernels
    return Kernels(prec)


def _family(k, backward, case):
    from ssl4polyp_amd import _lib
    info = _lib.AttentionPlanInfo()
    B, N, H, dh = case
    assert k.lib.pm_attention_plan(backward, B, N, H, dh, k.act, ctypes.byref(info)) == 0
    return FAMILY[info.family]


def _guarded(shape, dtype):
    """A NaN-filled tensor that is a slice of a larger buffer: GUARD elements of FILL in front and behind, 16-byte aligned."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_hold(buf, what):
    assert bool((buf[:GUARD] == FILL).all()), what + ": written in front of the buffer"
    assert bool((buf[-GUARD:] == FILL).all()), what + ": written behind the buffer"


def _forward(k, case, qkv, what):
    B, N, H, dh = case
    ob, out = _guarded((B, N, H * dh), k.act_dtype)
    lb, lse = _guarded((B, H, N), torch.float32)
    k.attention_fwd(qkv, out, lse, B, N, H, dh)
    torch.cuda.synchronize()
    _guards_hold(ob, what + " out")
    _guards_hold(lb, what + " lse")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()), what + ": out / lse not written everywhere"
    return out, lse


def _backward(k, case, qkv, out, dout, lse, what):
    """-> dqkv, delta (delta is scratch of the two-kernel family only: the fused kernel leaves it alone)."""
    B, N, H, dh = case
    gb, dqkv = _guarded((B, N, 3 * H * dh), k.act_dtype)
    db, delta = _guarded((B, H, N), torch.float32)
    k.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, dh)
    torch.cuda.synchronize()
    _guards_hold(gb, what + " dqkv")
    _guards_hold(db, what + " delta")
    assert bool(torch.isfinite(dqkv).all()), what + ": dqkv not written everywhere"
    return dqkv, delta


_inputs = {}


def _case(case, prec, regime="random"):
    """Operands on the device and the float64 references of one (shape, precision), computed once and never written to:
    the forward, and the backward on o_in = the float64 O rounded to the type."""
    key = (case, prec, regime)
    if key not in _inputs:
        B, N, H, dh = case
        qkv, dout = (t.to(DEV) for t in C.inputs(case, prec, regime))
        fwd = R.reference(qkv, B, N, H, dh)
        o_in = fwd["out"].to(R.DTYPES[prec])
        _inputs[key] = dict(qkv=qkv, dout=dout, o_in=o_in, lse_in=fwd["lse"].float(), ref=R.reference(qkv, B, N, H, dh, dout, o_in))
    return _inputs[key]


def _check_out(out, lse, ref, N, prec, what):
    r_lse = R.rel(lse, ref["lse"]) / R.F32_BOUNDS["lse"]
    r_out = R.out_ratio(out, ref, N, prec) if prec != "fp32" else R.rel(out, ref["out"]) / R.F32_BOUNDS["out"]
    print(f"{what} out: err/bound {r_out:.3f}")
    print(f"{what} lse: err/bound {r_lse:.3f}")
    assert r_out <= 1.0, f"{what}: out at {r_out:.3f} of its bound"
    assert r_lse < 1.0, f"{what}: lse at {r_lse:.3f} of its bound"


def _check_grads(dqkv, ref, N, prec, what, cancelling=()):
    """cancelling: outputs whose terms cancel exactly in this regime, so that f32 mode's norm-wise bound is taken against the
    largest sum of absolute terms T instead of the largest (vanishing) element."""
    if prec != "fp32":
        r = R.grad_ratios(dqkv, ref, N, prec)
    else:
        part = lambda x, j: x.reshape(*x.shape[:-1], 3, -1)[..., j, :]
        r = {}
        for j, n in enumerate(("dq", "dk", "dv")):
            want = part(ref["t_dqkv"] if n in cancelling else ref["dqkv"], j)
            r[n] = ((part(dqkv, j).double() - part(ref["dqkv"], j)).abs().max() / want.abs().max()).item() / R.F32_BOUNDS["grad"]
    for n, x in r.items():
        print(f"{what} {n}: err/bound {x:.3f}")
    for n, x in r.items():
        assert x <= 1.0, f"{what}: {n} at {x:.3f} of its bound"


def _run_case(case, prec, regime="random", cancelling=()):
    B, N, H, dh = case
    k, c = _k(prec), _case(case, prec, regime)
    tag = f"attn-edge {regime} {C.case_id(case)} {prec}"
    out, lse = _forward(k, case, c["qkv"], tag)
    _check_out(out, lse, c["ref"], N, prec, f"{tag} fwd-{_family(k, 0, case)}")
    fam = _family(k, 1, case)
    # the backward alone: `out` and `lse` made by the reference, so a forward / backward pair that is wrong consistently separates
    dqkv, _ = _backward(k, case, c["qkv"], c["o_in"], c["dout"], c["lse_in"], tag)
    _check_grads(dqkv, c["ref"], N, prec, f"{tag} bwd-{fam}", cancelling)
    # ... and chained on the kernel's own forward; delta = rowsum(dO * out) of THAT out
    dqkv, _ = _backward(k, case, c["qkv"], out, c["dout"], lse, tag + " chained")
    ref = R.reference(c["qkv"], B, N, H, dh, c["dout"], out)
    _check_grads(dqkv, ref, N, prec, f"{tag} bwd-{fam}-chained", cancelling)


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("case", [c for c in C.CASES if c[1] > 1], ids=C.case_id)
def test_attention_edges(case, prec):
    _run_case(case, prec)


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("case", [c for c in C.CASES if c[1] == 1], ids=C.case_id)
def test_attention_single_token(case, prec):
    """N = 1: P = 1, so out = V, lse = q . k dh^-1/2, dV = dO and dQ = dK = 0 exactly -- a relative norm of the latter is undefined,
    and the element-wise bound of a zero is zero, which the f32 evaluation of dP - delta (two different summation orders of the same
    dh products) misses by a few 2^-24 dO V: |dQ|, |dK| < 1e-5 max|dO| max|V| max|K or Q| instead."""
    B, N, H, dh = case
    D = H * dh
    k, c = _k(prec), _case(case, prec)
    tag = f"attn-edge N=1 {C.case_id(case)} {prec}"
    q, kk, v = (t.float() for t in c["qkv"].reshape(B, 1, 3, D).unbind(2))
    out, lse = _forward(k, case, c["qkv"], tag)
    assert torch.equal(out.float(), v), tag + ": out is not V bit for bit"
    qk = (q.double() * kk.double()).reshape(B, H, dh).sum(-1) * dh ** -0.5
    assert R.rel(lse.reshape(B, H), qk) < 1e-6, tag + ": lse"
    u = R.U.get(prec, R.F32_BOUNDS["grad"])   # (f32 mode: P = exp(s - lse) is 1 to a few 2^-24 |lse|; its gradient bound)
    do = c["dout"].float()
    for name, o_in, lse_in in (("alone", c["o_in"], c["lse_in"]), ("chained", out, lse)):
        dqkv, _ = _backward(k, case, c["qkv"], o_in, c["dout"], lse_in, f"{tag} {name}")
        dq, dk, dv = dqkv.float().reshape(B, 1, 3, D).unbind(2)
        assert bool(((dv - do).abs() <= u * do.abs()).all()), f"{tag} {name}: dV is not dO"
        small = 1e-5 * do.abs().max() * v.abs().max()
        print(f"{tag} {name}: max|dQ| {dq.abs().max().item():.2e} of {(small * kk.abs().max()).item():.2e}, "
              f"max|dK| {dk.abs().max().item():.2e} of {(small * q.abs().max()).item():.2e}")
        assert dq.abs().max() < small * kk.abs().max(), f"{tag} {name}: dQ"
        assert dk.abs().max() < small * q.abs().max(), f"{tag} {name}: dK"


# (shape, precision, heads b H + h): one multi-head problem per family, then single heads of it run alone as B = 1, H = 1
LOCALITY = [
    # forward head kernel and fused backward at dh 32 under the pair map of problem_of_block (B H = 16, H even): first, last, and a
    # pair (2p, 2p + 1) that the map sends to workgroups b and b + 8
    ((2, 65, 8, 32), "bf16", (0, 6, 7, 15)),
    # persistent forward, three rounds at grid 171: the first and the last head, and the three heads of workgroup 5 (buffer 0, 1, 0
    # again); the fused backward at dh 64 on the same heads
    ((57, 197, 9, 64), "bf16", (0, 5, 5 + 171, 5 + 342, 512)),
    ((37, 197, 7, 64), "fp16", (0, 129, 130, 258)),       # two rounds at grid 130: workgroup 0's two heads, the neighbour, the last
    ((2, 97, 3, 80), "fp32", (0, 2, 5)),                  # two-kernel backward and forward, chunked, a whole chunk of padding
    ((2, 257, 2, 80), "fp16", (0, 3)),                    # two-kernel backward, 16-bit
    ((3, 197, 2, 64), "fp32", (0, 3, 5)),                 # two-kernel backward, f32, dh 64
]


@pytest.mark.parametrize("case,prec,picks", LOCALITY, ids=[f"{C.case_id(c)}-{p}" for c, p, _ in LOCALITY])
def test_attention_head_locality(case, prec, picks):
    """A head's out, lse and slice of dqkv do not depend on its neighbours: bit-identical to the same head run alone.  (Every
    kernel's arithmetic per head is a function of N alone -- same instantiation, same tile order -- so no family is exempt.)"""
    B, N, H, dh = case
    k, c = _k(prec), _case(case, prec)
    tag = f"attn-edge locality {C.case_id(case)} {prec}"
    out, lse = _forward(k, case, c["qkv"], tag)
    dqkv, _ = _backward(k, case, c["qkv"], out, c["dout"], lse, tag)
    one = (1, N, 1, dh)
    for p in picks:
        b, h = divmod(p, H)
        qkv1 = c["qkv"].view(B, N, 3, H, dh)[b:b + 1, :, :, h].reshape(1, N, 3 * dh).contiguous()
        dout1 = c["dout"].view(B, N, H, dh)[b:b + 1, :, h].contiguous()
        out1, lse1 = _forward(k, one, qkv1, f"{tag} head {p}")
        assert torch.equal(out1, out.view(B, N, H, dh)[b:b + 1, :, h]), f"{tag}: out of head {p} depends on its neighbours"
        assert torch.equal(lse1, lse[b:b + 1, h:h + 1]), f"{tag}: lse of head {p} depends on its neighbours"
        dqkv1, _ = _backward(k, one, qkv1, out1, dout1, lse1, f"{tag} head {p}")
        assert torch.equal(dqkv1.view(1, N, 3, dh), dqkv.view(B, N, 3, H, dh)[b:b + 1, :, :, h]), \
            f"{tag}: dqkv of head {p} depends on its neighbours"


@pytest.mark.parametrize("case,prec", [((37, 197, 7, 64), "bf16"), ((2, 257, 4, 32), "fp16"), ((2, 257, 2, 80), "fp32")],
                         ids=lambda v: C.case_id(v) if isinstance(v, tuple) else v)
def test_attention_is_deterministic(case, prec):
    """Two runs of forward and backward: every output bit-equal (pm_attention.hip: no cross-wave reduction, no atomics)."""
    k, c = _k(prec), _case(case, prec)
    tag = f"attn-edge determinism {C.case_id(case)} {prec}"
    runs = []
    for _ in range(2):
        out, lse = _forward(k, case, c["qkv"], tag)
        dqkv, delta = _backward(k, case, c["qkv"], out, c["dout"], lse, tag)
        runs.append((out, lse, dqkv, delta.view(torch.int32)))   # (delta: NaN where the fused kernel leaves it alone)
    for name, a, b in zip(("out", "lse", "dqkv", "delta"), *runs):
        assert torch.equal(a, b), f"{tag}: {name} differs between two runs"


@pytest.mark.parametrize("prec", C.PRECS)
def test_attention_softmax_spike_regime(prec):
    """Q and K x 6: one dominant key per query, forward and backward, every precision: finite, within the norm-wise bounds of
    test_attention_fwd_bwd (out in f32 mode: the 1e-4 of test_attention_softmax_spike).  This regime cannot take the element-wise
    bound: a one-hot row has dS = 0 exactly in float64, while the f32 evaluation of dP - delta leaves about 1e-6
    (tests/test_attention_ref_cpu.py::test_softmax_spike_cannot_take_the_bound)."""
    case = C.SPIKE
    B, N, H, dh = case
    k, c = _k(prec), _case(case, prec, "spike")
    tag = f"attn-edge spike {C.case_id(case)} {prec}"
    out, lse = _forward(k, case, c["qkv"], tag)
    b_out = R.NORM16[prec]["out"] if prec != "fp32" else 1e-4
    b_grad = R.NORM16[prec]["grad"] if prec != "fp32" else R.F32_BOUNDS["grad"]
    errs = {"out": R.rel(out, c["ref"]["out"]) / b_out, "lse": R.rel(lse, c["ref"]["lse"]) / R.F32_BOUNDS["lse"]}
    part = lambda x, j: x.reshape(B, N, 3, H * dh)[:, :, j]
    dqkv, _ = _backward(k, case, c["qkv"], c["o_in"], c["dout"], c["lse_in"], tag)
    for j, n in enumerate(("dq", "dk", "dv")):
        errs[n] = R.rel(part(dqkv, j), part(c["ref"]["dqkv"], j)) / b_grad
    dqkv, _ = _backward(k, case, c["qkv"], out, c["dout"], lse, tag + " chained")
    ref = R.reference(c["qkv"], B, N, H, dh, c["dout"], out)
    for j, n in enumerate(("dq", "dk", "dv")):
        errs[n + "-chained"] = R.rel(part(dqkv, j), part(ref["dqkv"], j)) / b_grad
    for n, x in errs.items():
        print(f"{tag} {n}: norm-wise err/bound {x:.3f}")
    for n, x in errs.items():
        assert x < 1.0, f"{tag}: {n} at {x:.3f} of its bound"


@pytest.mark.parametrize("prec", C.PRECS)
def test_attention_identical_keys_regime(prec):
    """Every key of a head the same row: a uniform softmax, every score tied for the maximum.  Takes the element-wise bound (the
    emulation sits at <= 0.28 of it: tests/test_attention_ref_cpu.py::test_bound_accepts_identical_keys).  dQ = (sum_key dS) K = 0
    up to the rounding of o_in: f32 mode's norm-wise bound on dQ is taken against the largest |dS| |K|."""
    _run_case(C.IDENTICAL_KEYS, prec, "identical_keys", cancelling=("dq",))
