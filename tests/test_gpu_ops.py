"""Per-kernel parity on the MI355X: every C-ABI entry point against a plain PyTorch fp32 reference of the
same op on identical seeded inputs (bf16 mode: inputs pre-rounded to bf16, so the only differences are
accumulation order and the documented roundings).  Run with `pytest -m gpu` on the GPU box."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECS = ["bf16", "fp16", "fp32"]


def ptol(prec, bf16, fp32):
    """Bound per precision mode: fp16 carries 11 significant bits where bf16 carries 8 -> 1/8 of the bf16 bound (x 1.5 margin)."""
    return {"bf16": bf16, "fp16": bf16 * 1.5 / 8, "fp32": fp32}[prec]


def _k(precision):
    from ssl4polyp_amd.engine import Kernels
    return Kernels(precision)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(37, 768), (50, 512), (13, 64), (7, 32), (2000, 768), (41, 1024), (130, 1280)])
@pytest.mark.parametrize("prec", PRECS)
def test_layernorm_fwd_bwd(M, D, prec):
    k = _k(prec)
    x = rnd(M, D, seed=1, scale=2.0) + 0.5
    gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    y = torch.empty(M, D, dtype=k.act_dtype, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    k.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, D)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (D,), gr, br, 1e-6)
    tol = ptol(prec, 8e-3, 2e-6)
    assert rel(y.float(), yr) < tol
    assert rel(mean, x.mean(1)) < 1e-5
    dy = rnd(M, D, seed=4).to(k.act_dtype)
    dres = rnd(M, D, seed=5)
    yr.backward(dy.float())
    dx, dx_act = torch.empty(M, D, device=DEV), torch.empty(M, D, dtype=k.act_dtype, device=DEV)
    dg, db, dc = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    k.layernorm_bwd(dy, x, gamma, mean, rstd, dres, dx, dx_act, dg, db, dc, M, D)
    want = xr.grad + dres
    assert rel(dx, want) < 1e-5
    assert rel(dx_act.float(), want) < tol
    assert rel(dg, gr.grad) < 2e-5
    assert rel(db, br.grad) < 2e-5
    assert rel(dc, want.sum(0)) < 2e-5
    # in-place residual (dres aliases dx), no optional outputs
    dx2 = dres.clone()
    k.layernorm_bwd(dy, x, gamma, mean, rstd, dx2, dx2, None, None, None, None, M, D)
    assert rel(dx2, want) < 1e-5


# ------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(200, 264, 136), (1000, 768, 768), (256, 128, 64), (34, 96, 32), (394, 3072, 768), (394, 768, 3072),
               (129, 8, 520)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
@pytest.mark.parametrize("prec", PRECS)
def test_gemm_layouts(M, N, K, layout, prec):
    k = _k(prec)
    dt = k.act_dtype
    epc = 4 if prec == "fp32" else 8
    if layout in ("tn",) and (M % epc):
        pytest.skip("k-major A needs M % chunk == 0")
    if layout in ("nn", "tn") and (N % epc):
        pytest.skip("k-major B needs N % chunk == 0")
    A = rnd(M, K, seed=10).to(dt)
    B = rnd(N, K, seed=11).to(dt)
    want = A.float() @ B.float().t()
    bias = rnd(N, seed=12)
    C = torch.full((M, N), float("nan"), device=DEV)
    a_mat, lda, akm = (A, K, 0) if layout != "tn" else (A.t().contiguous(), M, 1)
    b_mat, ldb, bkm = (B, K, 0) if layout == "nt" else (B.t().contiguous(), N, 1)
    from ssl4polyp_amd._lib import EPI_STORE
    k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, bias, C, N, EPI_STORE, M, N, K)
    tol = 2e-6 if prec == "fp32" else 2e-5
    assert rel(C, want + bias) < tol * math.sqrt(K / 32)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_epilogues(prec):
    from ssl4polyp_amd._lib import EPI_ACCUM, EPI_DGELU, EPI_GELU, EPI_RESIDUAL, EPI_STORE
    k = _k(prec)
    dt = k.act_dtype
    M, N, K = 197 * 2, 256, 192
    A, B = rnd(M, K, seed=20).to(dt), rnd(N, K, seed=21, scale=0.2).to(dt)
    bias = rnd(N, seed=22)
    acc = A.float() @ B.float().t()
    tolc = ptol(prec, 1e-2, 3e-6)
    # act-typed plain store
    C = torch.empty(M, N, dtype=dt, device=DEV)
    k.gemm(A, K, 0, B, K, 0, bias, C, N, EPI_STORE, M, N, K)
    assert rel(C.float(), acc + bias) < tolc
    # GELU: aux = pre-activation, C = gelu(pre as stored)
    aux = torch.empty(M, N, dtype=dt, device=DEV)
    k.gemm(A, K, 0, B, K, 0, bias, C, N, EPI_GELU, M, N, K, aux=aux)
    assert rel(aux.float(), acc + bias) < tolc
    assert rel(C.float(), F.gelu(aux.float())) < tolc
    # residual, out of place and in place
    resid = rnd(M, N, seed=23)
    out = torch.empty(M, N, device=DEV)
    k.gemm(A, K, 0, B, K, 0, bias, out, N, EPI_RESIDUAL, M, N, K, resid=resid)
    assert rel(out, resid + acc + bias) < 1e-5
    r2 = resid.clone()
    k.gemm(A, K, 0, B, K, 0, bias, r2, N, EPI_RESIDUAL, M, N, K, resid=r2)
    assert rel(r2, resid + acc + bias) < 1e-5
    # dGELU
    pre = rnd(M, N, seed=24).to(dt)
    k.gemm(A, K, 0, B, K, 0, None, C, N, EPI_DGELU, M, N, K, aux=pre)
    p32 = pre.float().requires_grad_(True)
    F.gelu(p32).backward(acc)
    assert rel(C.float(), p32.grad) < tolc
    # accumulate
    base = rnd(M, N, seed=25)
    b2 = base.clone()
    k.gemm(A, K, 0, B, K, 0, None, b2, N, EPI_ACCUM, M, N, K)
    assert rel(b2, base + acc) < 1e-5


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,N,K", [(394, 3072, 768), (100, 512, 256), (2000, 3072, 768)])
def test_gelu_epilogue_without_the_pre_activation_store(M, N, K, prec):
    """PM_EPI_GELU with aux = NULL (forward-only use: evaluation, frozen blocks): the activation equals the one of the storing call
    bit for bit, through the 128 x 128 kernel and the ring kernels alike, and nothing is written anywhere else."""
    from ssl4polyp_amd._lib import EPI_GELU
    k = _k(prec)
    dt = k.act_dtype
    x, W, b = rnd(M, K, seed=21).to(dt), rnd(N, K, seed=22, scale=0.05).to(dt), rnd(N, seed=23)
    out1, aux = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=dt, device=DEV)
    k.linear_fwd(x, W, b, out1, M, N, K, EPI_GELU, aux=aux)
    out2 = torch.full((M + 1, N), 7.0, dtype=dt, device=DEV)   # (a guard row behind the output)
    k.linear_fwd(x, W, b, out2, M, N, K, EPI_GELU, aux=None)
    assert torch.equal(out2[:M], out1) and bool((out2[M] == 7.0).all())
    assert rel(out1.float(), F.gelu(aux.float())) < ptol(prec, 6e-3, 2e-6)


@pytest.mark.parametrize("prec", PRECS)
def test_linear_helpers_match_autograd(prec):
    """linear_fwd / linear_dgrad / linear_wgrad == nn.Linear forward + backward."""
    k = _k(prec)
    dt = k.act_dtype
    M, K, N = 394, 192, 320
    x, W = rnd(M, K, seed=30).to(dt), rnd(N, K, seed=31, scale=0.1).to(dt)
    dy = rnd(M, N, seed=32).to(dt)
    xr, Wr = x.float().requires_grad_(True), W.float().requires_grad_(True)
    (xr @ Wr.t()).backward(dy.float())
    dx = torch.empty(M, K, device=DEV)
    k.linear_dgrad(dy, W, dx, M, N, K)
    assert rel(dx, xr.grad) < 1e-4
    dW = torch.empty(N, K, device=DEV)
    k.linear_wgrad(dy, x, dW, M, N, K, False)
    assert rel(dW, Wr.grad) < 1e-4
    k.linear_wgrad(dy, x, dW, M, N, K, True)
    assert rel(dW, 2 * Wr.grad) < 1e-4


@pytest.mark.parametrize("M,N,K,layout,epi", [
    (4000, 2304, 768, "nt", "store"), (4000, 768, 3072, "nt", "resid"), (4000, 1536, 512, "nt", "gelu"),
    (4000, 768, 2304, "nn", "store"), (4000, 3072, 768, "nn", "dgelu"), (2304, 768, 4000 + 32, "tn", "store"),
    (768, 3072, 8192, "tn", "accum"), (520, 136, 4096, "tn", "store")])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_gemm_large_tile_paths(M, N, K, layout, epi, prec):
    """Forward / dgrad / split-K wgrad shapes at a ragged M = 4000, as the dispatcher sends them (pm_gemm_plan, checked on the CPU in
    tests/test_host_cpu.py): (4000, 2304, 768) nt store and (4000, 3072, 768) nn dgelu run on ring cfg 8;
    (4000, 768, 3072) nt resid, (4000, 768, 2304) nn store (48 tiles of 256 x 256) and (4000, 1536, 512) nt gelu (96 tiles) go to
    the 128 x 128 LDS-DMA kernel by the few-tiles rule (fewer than 128 tiles, M <= 4096); the three k-major-A shapes run the split-K ring weight-gradient kernels, (520, 136) on 256 x 128
    tiles and the other two on 256 x 256.  Every ring configuration is forced in test_gemm_ring_variants."""
    from ssl4polyp_amd._lib import EPI_ACCUM, EPI_DGELU, EPI_GELU, EPI_RESIDUAL, EPI_STORE
    k = _k(prec)
    bf = k.act_dtype
    t16 = ptol(prec, 1e-2, 0)
    A, B = rnd(M, K, seed=70, scale=0.5).to(bf), rnd(N, K, seed=71, scale=0.5).to(bf)
    acc = A.float() @ B.float().t()
    a_mat, lda, akm = (A, K, 0) if layout != "tn" else (A.t().contiguous(), M, 1)
    b_mat, ldb, bkm = (B, K, 0) if layout == "nt" else (B.t().contiguous(), N, 1)
    bias = rnd(N, seed=72) if epi in ("store", "resid", "gelu") and layout != "tn" else None
    want = acc + (bias if bias is not None else 0)
    tol = 3e-5 * math.sqrt(K / 32)
    if epi == "store":
        C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if layout == "tn" else bf)
        k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, bias, C, N, EPI_STORE, M, N, K)
        assert rel(C.float(), want) < (tol if layout == "tn" else t16)
    elif epi == "accum":
        base = rnd(M, N, seed=73)
        C = base.clone()
        k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, None, C, N, EPI_ACCUM, M, N, K)
        assert rel(C, base + acc) < tol
    elif epi == "resid":
        resid = rnd(M, N, seed=74)
        C = torch.empty(M, N, device=DEV)
        k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, bias, C, N, EPI_RESIDUAL, M, N, K, resid=resid)
        assert rel(C, resid + want) < tol
    elif epi == "gelu":
        C, aux = torch.empty(M, N, dtype=bf, device=DEV), torch.empty(M, N, dtype=bf, device=DEV)
        k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, bias, C, N, EPI_GELU, M, N, K, aux=aux)
        assert rel(aux.float(), want) < t16 and rel(C.float(), F.gelu(aux.float())) < t16
    else:
        pre = rnd(M, N, seed=75).to(bf)
        C = torch.empty(M, N, dtype=bf, device=DEV)
        k.gemm(a_mat, lda, akm, b_mat, ldb, bkm, None, C, N, EPI_DGELU, M, N, K, aux=pre)
        p32 = pre.float().requires_grad_(True)
        F.gelu(p32).backward(acc)
        assert rel(C.float(), p32.grad) < t16


# every shipped ring configuration on the (W layout, epilogue) pairs the heuristics send to it
RING_PAIRS = {
    8: [("nt", "store"), ("nt", "gelu"), ("nn", "dgelu")],
    9: [("nt", "store"), ("nt", "accum")],
    10: [("nt", "store"), ("nt", "accum")],
    24: [("nt", "resid"), ("nt", "store"), ("nt", "accum"), ("nn", "store")],
    25: [("nt", "resid")],
    26: [("nt", "resid")],
}
RING_PAIRS[1] = sorted({p for v in RING_PAIRS.values() for p in v})  # the 128 x 128 kernels on the same cases
# M = 1031: a ragged last tile of 7 rows at 256 and of 71 rows at 192 (12 DMA pieces over 8 waves); N = 264: two tile columns, the
# last 8 wide; K = 32 ... 160: 1, 2, 3, 5 k-steps = every prologue / tail branch of both k-loops; the wide shape: 8 tile columns
# = a full band of 6 and a narrow one of 2, 9 k-steps; N = 260: the 4-wide stores of a 16-bit C (N & 7; k-normal W only: a k-major W
# needs N % 8 == 0).  (K % 64 != 0 plans to the generic 128 x 128 kernel whatever the variant: tests/gemm_cases.py has the ring's K.)
RING_SHAPES = [(1031, 264, 32), (1031, 264, 64), (1031, 264, 96), (1031, 264, 160), (1031, 1800, 288), (1031, 260, 64)]
_ring_inputs = {}


def _ring_case(prec, M, N, K):
    """Operands and float32 references of one shape, computed once and shared by every variant (never written to)."""
    key = (prec, M, N, K)
    if key not in _ring_inputs:
        dt = _k(prec).act_dtype
        A, B = rnd(M, K, seed=90, scale=0.5).to(dt), rnd(N, K, seed=91, scale=0.5).to(dt)
        bias, base, pre = rnd(N, seed=92), rnd(M, N, seed=93), rnd(M, N, seed=94).to(dt)
        acc = A.float() @ B.float().t()
        p32 = pre.float().requires_grad_(True)
        F.gelu(p32).backward(acc)
        _ring_inputs[key] = dict(A=A, B=B, Bt=B.t().contiguous(), bias=bias, base=base, pre=pre, acc=acc, dgelu=p32.grad)
    return _ring_inputs[key]


@pytest.mark.parametrize("variant", [8, 9, 10, 24, 25, 26, 1])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_gemm_ring_variants(prec, variant):
    """Each shipped ring kernel, forced through gemm_variant, against float32 A @ B.T of the rounded operands; C carries a guard
    row behind row M that must keep its fill value."""
    from ssl4polyp_amd._lib import EPI_ACCUM, EPI_DGELU, EPI_GELU, EPI_RESIDUAL, EPI_STORE
    k = _k(prec)
    k.gemm_variant = variant
    dt, t16, fill = k.act_dtype, ptol(prec, 1e-2, 0), 7.0
    for M, N, K in RING_SHAPES:
        c = _ring_case(prec, M, N, K)
        tol = 3e-5 * math.sqrt(K / 32)
        for layout, epi in RING_PAIRS[variant]:
            if layout == "nn" and N % 8:
                continue
            b_mat, ldb, bkm = (c["B"], K, 0) if layout == "nt" else (c["Bt"], N, 1)
            bias = c["bias"] if layout == "nt" and epi != "accum" else None
            want = c["acc"] + (bias if bias is not None else 0)
            C = torch.full((M + 1, N), fill, device=DEV, dtype=dt if epi in ("store", "gelu", "dgelu") else torch.float32)
            what = f"variant {variant} {prec} {(M, N, K)} {layout} {epi}"
            if epi == "store":
                k.gemm(c["A"], K, 0, b_mat, ldb, bkm, bias, C, N, EPI_STORE, M, N, K)
                err, bound = rel(C[:M].float(), want), t16
            elif epi == "accum":
                C[:M] = c["base"]
                k.gemm(c["A"], K, 0, b_mat, ldb, bkm, None, C, N, EPI_ACCUM, M, N, K)
                err, bound = rel(C[:M], c["base"] + want), tol
            elif epi == "resid":
                k.gemm(c["A"], K, 0, b_mat, ldb, bkm, bias, C, N, EPI_RESIDUAL, M, N, K, resid=c["base"])
                err, bound = rel(C[:M], c["base"] + want), tol
            elif epi == "gelu":
                aux = torch.full((M + 1, N), fill, device=DEV, dtype=dt)
                k.gemm(c["A"], K, 0, b_mat, ldb, bkm, bias, C, N, EPI_GELU, M, N, K, aux=aux)
                err, bound = max(rel(aux[:M].float(), want), rel(C[:M].float(), F.gelu(aux[:M].float()))), t16
                assert bool((aux[M] == fill).all()), what + ": aux guard row written"
            else:
                k.gemm(c["A"], K, 0, b_mat, ldb, bkm, None, C, N, EPI_DGELU, M, N, K, aux=c["pre"])
                err, bound = rel(C[:M].float(), c["dgelu"]), t16
            print(f"{what}: err {err:.3e} bound {bound:.3e}")
            assert err < bound, what
            assert bool((C[M] == fill).all()), what + ": guard row written"


@pytest.mark.parametrize("M,N,K,layout,epi", [
    (4000, 3072, 768, "nn", "dgelu"),    # dGELU dgrad, 256-row tiles (the fc1.bias gradient)
    (4000 + 7, 768, 2304, "nn", "store"),  # 192-row tiles, ragged last tile
    (300, 512, 256, "nn", "store"),      # small M: not the large-tile kernel
    (4000, 2304, 768, "nt", "store")])   # LDS-staged epilogue
def test_gemm_colsum(M, N, K, layout, epi):
    """A GEMM, then the column sums of what it stored (pm_colsum_ws on the same stream): colsum[n] += sum_m C[m][n], the bias gradient
    of the Linear whose output gradient C is.  There is no fused form."""
    from ssl4polyp_amd._lib import EPI_DGELU, EPI_STORE
    k = _k("bf16")
    bf = torch.bfloat16
    A, B = rnd(M, K, seed=80, scale=0.5).to(bf), rnd(N, K, seed=81, scale=0.5).to(bf)
    acc = A.float() @ B.float().t()
    b_mat, ldb, bkm = (B, K, 0) if layout == "nt" else (B.t().contiguous(), N, 1)
    C = torch.full((M, N), float("nan"), device=DEV, dtype=bf)
    base = rnd(N, seed=82)
    cs = base.clone()
    if epi == "dgelu":
        pre = rnd(M, N, seed=83).to(bf)
        k.gemm(A, K, 0, b_mat, ldb, bkm, None, C, N, EPI_DGELU, M, N, K, aux=pre)
        p32 = pre.float().requires_grad_(True)
        F.gelu(p32).backward(acc)
        want = p32.grad
    else:
        k.gemm(A, K, 0, b_mat, ldb, bkm, None, C, N, EPI_STORE, M, N, K)
        want = acc
    k.colsum(C, cs, M, N)
    assert rel(C.float(), want) < 1e-2
    # the sums are over what was stored (after the bf16 rounding of C)
    assert rel(cs - base, want.sum(0)) < 2e-3
    assert rel(cs - base, C.float().sum(0)) < 2e-3


# ------------------------------------------------------------------------------------------------
def _attn_ref(qkv, B, N, H, dh):
    q, k_, v = qkv.float().reshape(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k_.transpose(-2, -1)) * dh ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * dh)
    return o, lse


@pytest.mark.parametrize("B,N,H,dh", [(2, 197, 3, 64), (3, 50, 2, 64), (2, 197, 4, 32), (2, 17, 2, 32), (1, 33, 1, 64),
                                      (1, 224, 1, 32),
                                      # ViT-H/14 (models_mae.py:239-244): 80-wide heads at N = 65 (masked) / 257, the decoder's
                                      # 32-wide heads and a 64-wide head at N = 257, and the shapes in between
                                      (2, 65, 3, 80), (2, 257, 2, 80), (1, 197, 2, 80), (2, 257, 4, 32), (1, 257, 2, 64),
                                      (1, 288, 1, 80), (1, 3, 1, 80),
                                      # more than one tile of padding (N = 100 runs the seven-tile instantiation)
                                      (2, 100, 2, 64), (1, 130, 2, 32), (1, 70, 1, 64),
                                      # B H = 259: workgroups of the persistent forward walk two heads, one walks one (the next
                                      # head's DMA addresses); one valid key / none padded in the last tile; the dh = 32 pair map
                                      (37, 197, 7, 64), (1, 193, 2, 64), (1, 224, 2, 64), (4, 50, 4, 32)])
@pytest.mark.parametrize("prec", PRECS)
def test_attention_fwd_bwd(B, N, H, dh, prec):
    k = _k(prec)
    dt = k.act_dtype
    D = H * dh
    qkv = rnd(B, N, 3 * D, seed=40, scale=1.5).to(dt)
    out = torch.full((B, N, D), float("nan"), dtype=dt, device=DEV)
    lse = torch.empty(B, H, N, device=DEV)
    k.attention_fwd(qkv, out, lse, B, N, H, dh)
    qr = qkv.float().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qr, B, N, H, dh)
    tol = ptol(prec, 1.5e-2, 2e-5)
    assert rel(out.float(), o_ref) < tol
    assert rel(lse, lse_ref) < 1e-5
    dout = rnd(B, N, D, seed=41).to(dt)
    o_ref.backward(dout.float())
    dqkv = torch.full((B, N, 3 * D), float("nan"), dtype=dt, device=DEV)
    delta = torch.empty(B, H, N, device=DEV)
    k.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, dh)
    got, want = dqkv.float().reshape(B, N, 3, D), qr.grad.reshape(B, N, 3, D)
    for j, nm in enumerate("qkv"):
        assert rel(got[:, :, j], want[:, :, j]) < ptol(prec, 3e-2, 5e-5), nm


def test_attention_softmax_spike():
    """One dominant key per query (large logits): exercises the max-subtraction path."""
    k = _k("fp32")
    B, N, H, dh = 1, 197, 2, 64
    qkv = rnd(B, N, 3 * H * dh, seed=42)
    qkv[:, :, : 2 * H * dh] *= 6.0
    out, lse = torch.empty(B, N, H * dh, device=DEV), torch.empty(B, H, N, device=DEV)
    k.attention_fwd(qkv, out, lse, B, N, H, dh)
    o_ref, lse_ref = _attn_ref(qkv, B, N, H, dh)
    assert torch.isfinite(out).all()
    assert rel(out, o_ref) < 1e-4 and rel(lse, lse_ref) < 1e-5


@pytest.mark.parametrize("N,dh", [(197, 64), (50, 64), (197, 32)])
@pytest.mark.parametrize("prec", PRECS)
def test_attention_bwd_all_scores_strongly_negative(N, dh, prec):
    """Regression (round 3, found by the head+2 fine-tune bench going NaN after ~60 steps): when EVERY real score of a query is
    strongly negative its log-sum-exp drops below -88, and a padded key (score 0 -- its K row is zero) got
    P = exp2(0 - lse * log2 e) = inf in the backward, whose dS = inf met the zero K row as inf x 0 = NaN in dQ.  q = +a u,
    k = -a u gives q . k * dh^-0.5 ~ -150 for every pair: dQ / dK / dV must be finite and equal the reference."""
    k = _k(prec)
    dt = k.act_dtype
    B, H = 2, 2
    D = H * dh
    g = torch.Generator(device=DEV).manual_seed(43)
    u = torch.randn(1, 1, H, dh, generator=g, device=DEV)
    u = u / u.norm(dim=-1, keepdim=True)
    a = (150.0 * dh ** 0.5) ** 0.5
    jitter = 0.05 * torch.randn(B, N, 2, H, dh, generator=g, device=DEV)
    qk = torch.stack([a * u.expand(B, N, H, dh), -a * u.expand(B, N, H, dh)], dim=2) + jitter
    v = torch.randn(B, N, 1, H, dh, generator=g, device=DEV)
    qkv = torch.cat([qk, v], dim=2).reshape(B, N, 3 * D).to(dt).contiguous()
    out = torch.empty(B, N, D, dtype=dt, device=DEV)
    lse = torch.empty(B, H, N, device=DEV)
    k.attention_fwd(qkv, out, lse, B, N, H, dh)
    assert lse.max().item() < -100.0, lse.max().item()   # the regime: exp2(-lse * log2 e) overflows f32
    qr = qkv.float().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qr, B, N, H, dh)
    assert rel(out.float(), o_ref) < ptol(prec, 1.5e-2, 5e-5) and rel(lse, lse_ref) < 1e-5
    dout = rnd(B, N, D, seed=44).to(dt)
    o_ref.backward(dout.float())
    dqkv = torch.full((B, N, 3 * D), float("nan"), dtype=dt, device=DEV)
    delta = torch.empty(B, H, N, device=DEV)
    k.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, dh)
    assert torch.isfinite(dqkv.float()).all(), "NaN / inf in dQ, dK or dV"
    got, want = dqkv.float().reshape(B, N, 3, D), qr.grad.reshape(B, N, 3, D)
    for j, nm in enumerate("qkv"):
        if prec != "fp32" and nm == "q":
            # dQ = sum_key dS[key] K[key] with sum_key dS = 0 and K[key] = -a u + jitter: the common part (|a u| = 35) cancels
            # exactly in f32, while the bf16 rounding of each dS term (2^-9 relative, the kernels' rounding point in front of
            # the dS K MFMA) leaves 35 x 2^-9 x |dS| of noise against a 0.05 x |dS| signal -- this construction is
            # ill-conditioned for ANY bf16 dS by design; finiteness (above) is what it checks for dQ
            continue
        # (f32 mode sees the same cancellation at f32 resolution: 35 x 2^-24 / 0.05 -> a few 1e-4 on dQ)
        assert rel(got[:, :, j], want[:, :, j]) < (ptol(prec, 5e-2, 0) if prec != "fp32" else (2e-3 if nm == "q" else 2e-4)), nm


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_colsum_cast_gradstats(prec):
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k(prec)
    x = rnd(777, 520, seed=50).to(k.act_dtype)
    out = torch.ones(520, device=DEV)
    k.colsum(x, out, 777, 520)
    assert rel(out, 1 + x.float().sum(0)) < 1e-5
    src = rnd(1027, seed=51)
    dst = torch.empty(1027, dtype=k.act_dtype, device=DEV)
    k.cast(src, dst)
    assert torch.equal(dst, src.to(k.act_dtype))
    g = rnd(100003, seed=52)
    g[17], g[99], g[100002] = float("nan"), float("inf"), float("-inf")
    stats = torch.zeros(3, device=DEV)
    _lib.check(k.lib.pm_grad_stats(_ptr(g), g.numel(), _ptr(stats), _stream()), "pm_grad_stats")
    assert stats[1].item() == 1 and stats[2].item() == 2
    g2 = rnd(4097, seed=53)
    stats.zero_()
    _lib.check(k.lib.pm_grad_stats(_ptr(g2), g2.numel(), _ptr(stats), _stream()), "pm_grad_stats")
    assert abs(stats[0].item() - (g2.double() ** 2).sum().item()) < 1e-3 * stats[0].item()


@pytest.mark.parametrize("img,p,D", [(224, 16, 768), (32, 8, 64), (56, 14, 128), (48, 12, 64)])
@pytest.mark.parametrize("prec", PRECS)
def test_patch_embed_path(img, p, D, prec):
    """im2col (+kept-patch gather) + GEMM + token assembly == Conv2d patch embed + pos + cls (+ gather)."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k(prec)
    B, C = 3, 3
    L = (img // p) ** 2
    keep = L // 4
    imgs = rnd(B, C, img, img, seed=60)
    W = rnd(D, C, p, p, seed=61, scale=0.05)
    bias, cls, pos = rnd(D, seed=62), rnd(D, seed=63), rnd(L + 1, D, seed=64)
    ref = F.conv2d(imgs.to(k.act_dtype).float(), W.to(k.act_dtype).float(), bias, stride=p).flatten(2).transpose(1, 2)
    ref = ref + pos[1:]
    g = torch.Generator().manual_seed(65)
    ids = torch.stack([torch.randperm(L, generator=g)[:keep] for _ in range(B)]).to(DEV)
    PE = C * p * p
    PEp = k.padded_k(PE)  # patch 14: 588 -> 640, zero columns in the patch rows and in the weight
    assert (PEp == PE) == (p not in (14, 12))   # 588 -> 640 (element-wise patch rows), 432 -> 448 (16-B patch rows + padding)
    for ids_keep, kp in ((None, L), (ids.int().contiguous(), keep)):
        cols = torch.full((B * kp, PEp), float("nan"), dtype=k.act_dtype, device=DEV)
        _lib.check(k.lib.pm_patch_im2col(_ptr(imgs), _ptr(ids_keep), _ptr(cols), PEp, k.act, B, C, img, p, kp, _stream()), "im2col")
        assert torch.equal(cols[:, PE:], torch.zeros(B * kp, PEp - PE, dtype=k.act_dtype, device=DEV))
        emb = torch.empty(B * kp, D, device=DEV)
        w = W.to(k.act_dtype).view(D, -1) if PEp == PE else k.pad_cast(W.view(D, PE).contiguous(), D, PEp)
        if PEp != PE:
            assert torch.equal(w[:, :PE], W.to(k.act_dtype).view(D, PE)) and not w[:, PE:].any()
            back = torch.ones(D, PE, device=DEV)
            k.unpad_add(w.float().contiguous(), back, True)
            assert torch.equal(back, 1 + W.to(k.act_dtype).view(D, PE).float())
        k.linear_fwd(cols, w, bias, emb, B * kp, D, PEp)
        x = torch.empty(B, kp + 1, D, device=DEV)
        _lib.check(k.lib.pm_assemble_tokens(_ptr(emb), _ptr(cls), _ptr(pos), _ptr(ids_keep), _ptr(x), B, kp, D, _stream()), "assemble")
        want = ref if ids_keep is None else torch.gather(ref, 1, ids.unsqueeze(-1).expand(-1, -1, D))
        want = torch.cat([(cls + pos[0]).expand(B, 1, D), want], 1)
        assert rel(x, want) < 2e-5
        # backward of the assembly
        dx = rnd(B, kp + 1, D, seed=66)
        demb = torch.empty(B * kp, D, dtype=k.act_dtype, device=DEV)
        dcls, dpos = torch.zeros(D, device=DEV), torch.zeros(L + 1, D, device=DEV)
        _lib.check(k.lib.pm_assemble_tokens_bwd(_ptr(dx), _ptr(ids_keep), _ptr(demb), k.act, _ptr(dcls), _ptr(dpos), B, kp, D,
                                                _stream()), "assemble_bwd")
        assert torch.equal(demb.view(B, kp, D), dx[:, 1:].to(k.act_dtype))
        assert rel(dcls, dx[:, 0].sum(0)) < 1e-5
        want_pos = torch.zeros(L + 1, D, device=DEV)
        want_pos[0] = dx[:, 0].sum(0)
        idx = torch.arange(L, device=DEV).expand(B, L) if ids_keep is None else ids
        want_pos.index_add_(0, (idx + 1).reshape(-1), dx[:, 1:].reshape(-1, D))
        assert rel(dpos, want_pos) < 1e-5


def test_mae_masking_and_unshuffle():
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k("bf16")
    B, L, keep, D = 5, 196, 49, 512
    noise = torch.rand(B, L, generator=torch.Generator().manual_seed(70)).to(DEV)
    noise[0, 5] = noise[0, 100]  # a tie: stable order must win
    ids_shuffle = torch.empty(B, L, dtype=torch.int32, device=DEV)
    ids_restore = torch.empty(B, L, dtype=torch.int32, device=DEV)
    mask = torch.empty(B, L, device=DEV)
    _lib.check(k.lib.pm_mae_masking(_ptr(noise), _ptr(ids_shuffle), _ptr(ids_restore), _ptr(mask), B, L, keep, _stream()), "masking")
    s_ref = torch.argsort(noise.cpu(), dim=1, stable=True)
    r_ref = torch.argsort(s_ref, dim=1)
    assert torch.equal(ids_shuffle.cpu().long(), s_ref) and torch.equal(ids_restore.cpu().long(), r_ref)
    m_ref = torch.ones(B, L)
    m_ref[:, :keep] = 0
    assert torch.equal(mask.cpu(), torch.gather(m_ref, 1, r_ref))
    emb, mtok, dpos = rnd(B, keep + 1, D, seed=71), rnd(D, seed=72), rnd(L + 1, D, seed=73)
    out = torch.empty(B, L + 1, D, device=DEV)
    _lib.check(k.lib.pm_mae_unshuffle(_ptr(emb), _ptr(mtok), _ptr(dpos), _ptr(ids_restore), _ptr(out), B, L, keep, D, _stream()), "unshuffle")
    er = emb.clone().requires_grad_(True)
    mr = mtok.clone().requires_grad_(True)
    x_ = torch.cat([er[:, 1:], mr.expand(B, L - keep, D)], 1)
    x_ = torch.gather(x_, 1, ids_restore.long().unsqueeze(-1).expand(-1, -1, D))
    want = torch.cat([er[:, :1], x_], 1) + dpos
    assert rel(out, want) < 1e-6
    dout = rnd(B, L + 1, D, seed=74)
    want.backward(dout)
    demb = torch.empty(B, keep + 1, D, device=DEV)
    dm = torch.zeros(D, device=DEV)
    ws = torch.empty(128 * D, device=DEV)
    _lib.check(k.lib.pm_mae_unshuffle_bwd(_ptr(dout), _ptr(ids_shuffle), _ptr(demb), 0, _ptr(dm), B, L, keep, D, _ptr(ws),
                                          ws.numel() * 4, _stream()), "unshuffle_bwd")
    dm2 = torch.zeros_like(dm)
    _lib.check(k.lib.pm_mae_unshuffle_bwd(_ptr(dout), _ptr(ids_shuffle), _ptr(demb), 0, _ptr(dm2), B, L, keep, D, None, 0,
                                          _stream()), "unshuffle_bwd")  # atomics fallback
    assert rel(demb, er.grad) < 1e-6 and rel(dm, mr.grad) < 1e-5 and rel(dm2, mr.grad) < 1e-5


@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("img,p", [(224, 16), (32, 8), (56, 14)])
def test_mae_loss(norm_pix, img, p):
    from oracle import vit_mae_ref as O
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k("fp32")
    B, C = 3, 3
    L, PE = (img // p) ** 2, p * p * C
    imgs = rnd(B, C, img, img, seed=80)
    pred_full = rnd(B, L + 1, PE, seed=81)
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(82)) < 0.75).float().to(DEV)
    pl = torch.empty(B * L, device=DEV)
    sums, loss = torch.empty(2, device=DEV), torch.empty(1, device=DEV)
    _lib.check(k.lib.pm_mae_loss_fwd(_ptr(imgs), _ptr(pred_full), PE, 1, _ptr(pl), B, C, img, p, norm_pix, _stream()), "loss_fwd")
    _lib.check(k.lib.pm_mae_loss_finish(_ptr(pl), _ptr(mask), B * L, _ptr(sums), _ptr(loss), _stream()), "loss_finish")
    cfg = O.ViTConfig(img_size=img, patch_size=p)
    pr = pred_full[:, 1:].cpu().clone().requires_grad_(True)
    want = O.mae_loss(imgs.cpu(), pr, mask.cpu(), cfg, bool(norm_pix))
    assert abs(loss.item() - want.item()) < 2e-6 * abs(want.item())
    want.backward()
    PEp = k.padded_k(PE)  # (row pitch of dpred: the reduction dimension of decoder_pred's backward GEMMs)
    dpred = torch.full((B, L + 1, PEp), float("nan"), device=DEV)
    dl = torch.full((1,), 0.5, device=DEV)
    _lib.check(k.lib.pm_mae_loss_bwd(_ptr(imgs), _ptr(pred_full), PE, 1, _ptr(mask), _ptr(sums), _ptr(dl), _ptr(dpred), PEp, 0, B, C,
                                     img, p, norm_pix, _stream()), "loss_bwd")
    assert torch.equal(dpred[:, 0], torch.zeros(B, PEp, device=DEV))
    assert not dpred[:, :, PE:].any()
    assert rel(dpred[:, 1:, :PE], 0.5 * pr.grad) < 1e-5


def test_cls_head_and_adamw():
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k("bf16")
    B, N, D, nc = 5, 197, 768, 2
    x = rnd(B, N, D, seed=90)
    gamma, beta = 1 + 0.1 * rnd(D, seed=91), 0.1 * rnd(D, seed=92)
    W, bias = rnd(nc, D, seed=93, scale=0.05), rnd(nc, seed=94)
    xn, mean, rstd = torch.empty(B, D, device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    logits = torch.empty(B, nc, device=DEV)
    _lib.check(k.lib.pm_cls_head_fwd(_ptr(x), N, _ptr(gamma), _ptr(beta), _ptr(W), _ptr(bias), _ptr(xn), _ptr(mean), _ptr(rstd),
                                     _ptr(logits), B, D, nc, 1e-6, _stream()), "cls_head_fwd")
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Wr, bbr = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    ref = F.linear(F.layer_norm(xr, (D,), gr, br, 1e-6)[:, 0], Wr, bbr)
    assert rel(logits, ref) < 1e-5
    dlog = rnd(B, nc, seed=95)
    ref.backward(dlog)
    dx = torch.full((B, N, D), float("nan"), device=DEV)
    dxa = torch.empty(B, N, D, dtype=torch.bfloat16, device=DEV)
    dW, dbias = torch.zeros(nc, D, device=DEV), torch.zeros(nc, device=DEV)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    _lib.check(k.lib.pm_cls_head_bwd(_ptr(dlog), _ptr(x), N, _ptr(gamma), _ptr(W), _ptr(xn), _ptr(mean), _ptr(rstd), _ptr(dx),
                                     _ptr(dxa), 1, _ptr(dW), _ptr(dbias), _ptr(dg), _ptr(db), B, D, nc, _stream()), "cls_head_bwd")
    assert rel(dx, xr.grad) < 1e-5 and rel(dW, Wr.grad) < 1e-5 and rel(dbias, bbr.grad) < 1e-5
    assert rel(dg, gr.grad) < 1e-5 and rel(db, br.grad) < 1e-5
    assert rel(dxa.float(), xr.grad) < 8e-3
    # AdamW, 3 steps, against torch.optim.AdamW
    n = 4096 + 64
    p0, p1 = rnd(n, seed=96), None
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    p1, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    for step in range(1, 4):
        g = rnd(n, seed=100 + step)
        pt.grad = g.clone()
        opt.step()
        _lib.check(k.lib.pm_adamw(_ptr(p1), _ptr(g), _ptr(m), _ptr(v), _ptr(shadow), 1, n, 1e-2, 0.9, 0.95, 1e-8, 0.05, step, 1.0,
                                  _stream()), "adamw")
    assert rel(p1, pt.detach()) < 2e-6
    assert torch.equal(shadow, p1.bfloat16())


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("head", [True, False])
@pytest.mark.parametrize("D,N,nc", [(768, 197, 2), (64, 17, 5), (512, 50, 11)])
def test_vit_head_pool_and_head_modes(pool, head, D, N, nc):
    """pm_vit_head_fwd / _bwd: final LayerNorm + token selection (cls row | mean of the patch rows) + optional lin_head
    (models.py:134-139, 216-221), every mode against autograd of the same torch expression."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    k = _k("bf16")
    B = 5
    x = rnd(B, N, D, seed=190, scale=1.5) + 0.3
    gamma, beta = 1 + 0.1 * rnd(D, seed=191), 0.1 * rnd(D, seed=192)
    W, bias = rnd(nc, D, seed=193, scale=0.05), rnd(nc, seed=194)
    feat = torch.empty(B, D, device=DEV)
    xhm = torch.empty(B, D, device=DEV) if pool else None
    mean = torch.empty(B * (N if pool else 1), device=DEV)
    rstd = torch.empty_like(mean)
    logits = torch.empty(B, nc, device=DEV) if head else None
    _lib.check(k.lib.pm_vit_head_fwd(_ptr(x), N, pool, _ptr(gamma), _ptr(beta), _ptr(W) if head else None,
                                     _ptr(bias) if head else None, _ptr(feat), _ptr(xhm), _ptr(mean), _ptr(rstd), _ptr(logits),
                                     B, D, nc if head else 0, 1e-6, _stream()), "vit_head_fwd")
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Wr, bbr = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    y = F.layer_norm(xr, (D,), gr, br, 1e-6)
    fr = y[:, 1:].mean(1) if pool else y[:, 0]
    assert rel(feat, fr) < 1e-5
    ref = F.linear(fr, Wr, bbr) if head else fr
    if head:
        assert rel(logits, ref) < 1e-5
    dout = rnd(*ref.shape, seed=195)
    ref.backward(dout)
    dx = torch.full((B, N, D), float("nan"), device=DEV)
    dxa = torch.empty(B, N, D, dtype=torch.bfloat16, device=DEV)
    dW, dbias = torch.zeros(nc, D, device=DEV), torch.zeros(nc, device=DEV)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    _lib.check(k.lib.pm_vit_head_bwd(_ptr(dout) if head else None, None if head else _ptr(dout), _ptr(x), N, pool, _ptr(gamma),
                                     _ptr(W) if head else None, _ptr(feat), _ptr(xhm), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dxa), 1,
                                     _ptr(dW) if head else None, _ptr(dbias) if head else None, _ptr(dg), _ptr(db), B, D,
                                     nc if head else 0, _stream()), "vit_head_bwd")
    assert rel(dx, xr.grad) < 2e-5 and rel(dg, gr.grad) < 2e-5 and rel(db, br.grad) < 2e-5
    assert rel(dxa.float(), xr.grad) < 8e-3
    if head:
        assert rel(dW, Wr.grad) < 1e-5 and rel(dbias, bbr.grad) < 1e-5
    # frozen backbone: parameter gradients only, dx == NULL
    dW2, dg2 = torch.zeros(nc, D, device=DEV), torch.zeros(D, device=DEV)
    _lib.check(k.lib.pm_vit_head_bwd(_ptr(dout) if head else None, None if head else _ptr(dout), _ptr(x), N, pool, _ptr(gamma),
                                     _ptr(W) if head else None, _ptr(feat), _ptr(xhm), _ptr(mean), _ptr(rstd), None, None, 1,
                                     _ptr(dW2) if head else None, None, _ptr(dg2), None, B, D, nc if head else 0, _stream()),
               "vit_head_bwd frozen")
    assert torch.equal(dg2, dg) and (not head or torch.equal(dW2, dW))


@pytest.mark.parametrize("B,nc", [(64, 2), (7, 2), (300, 2), (9, 5), (700, 3)])
def test_supervised_loss_op(B, nc, golden):
    """pm_supervised_loss_fwd + pm_scale through ssl4polyp_amd.supervised_loss: value and gradient against torch's
    BCEWithLogitsLoss(pos_weight) on l1 - l0 (two classes, tc.py:3347-3374,6090-6102) / CrossEntropyLoss(weight)
    (tc.py:6104), and against the reference-generated bce values of tests/golden/tables.npz."""
    import ssl4polyp_amd as A
    logits = rnd(B, nc, seed=200, scale=2.0)
    g = torch.Generator().manual_seed(201)
    y = torch.randint(0, nc, (B,), generator=g).to(DEV)
    lr = logits.clone().requires_grad_(True)
    if nc == 2:
        for pw in (None, 0.37, 2.5):
            lh = logits.clone().requires_grad_(True)
            got = A.supervised_loss(lh, y, pos_weight=pw)
            want = F.binary_cross_entropy_with_logits(lr[:, 1] - lr[:, 0], y.float(),
                                                      pos_weight=None if pw is None else torch.tensor(pw, device=DEV))
            assert abs(got.item() - want.item()) < 2e-6 * max(1.0, abs(want.item()))
            lr.grad = None
            (3.0 * want).backward()
            (3.0 * got).backward()
            assert rel(lh.grad, lr.grad) < 1e-5
    else:
        w = (0.5 + torch.rand(nc, generator=g)).to(DEV)
        for cw in (None, w):
            lh = logits.clone().requires_grad_(True)
            got = A.supervised_loss(lh, y, class_weights=cw)
            want = F.cross_entropy(lr, y, weight=cw)
            assert abs(got.item() - want.item()) < 2e-6 * max(1.0, abs(want.item()))
            lr.grad = None
            (0.5 * want).backward()
            (0.5 * got).backward()
            assert rel(lh.grad, lr.grad) < 1e-5
    if (B, nc) == (64, 2):  # the reference-generated table
        fx = golden("tables.npz")
        z, t = torch.from_numpy(fx["bce/logits"]).to(DEV), torch.from_numpy(fx["bce/targets"]).to(DEV)
        for pw in (1.0, 0.37, 2.5):
            np.testing.assert_allclose(A.supervised_loss(z, t, pos_weight=pw).item(), fx[f"bce/pw{pw}"], rtol=2e-6)


def test_registered_torch_ops_forward_and_autograd():
    """torch.ops.polypmae.{layernorm, linear_bias, linear_bias_gelu, linear_bias_residual, attention}: the C-ABI kernels as
    registered custom ops with autograd, against the same expression in plain torch (fp32 tensors -> exact-f32 MFMA mode)."""
    from ssl4polyp_amd import ops  # noqa: F401
    P = torch.ops.polypmae
    B, N, D, H = 3, 50, 128, 4
    x = rnd(B, N, D, seed=300).requires_grad_(True)
    g, b = (1 + 0.1 * rnd(D, seed=301)).requires_grad_(True), (0.1 * rnd(D, seed=302)).requires_grad_(True)
    Wq, bq = rnd(3 * D, D, seed=303, scale=0.08).requires_grad_(True), rnd(3 * D, seed=304, scale=0.1).requires_grad_(True)
    Wp, bp = rnd(D, D, seed=305, scale=0.08).requires_grad_(True), rnd(D, seed=306, scale=0.1).requires_grad_(True)
    W1, b1 = rnd(2 * D, D, seed=307, scale=0.08).requires_grad_(True), rnd(2 * D, seed=308, scale=0.1).requires_grad_(True)
    leaves = [x, g, b, Wq, bq, Wp, bp, W1, b1]

    def hip():
        y = P.layernorm(x, g, b, 1e-6, False)
        a = P.attention(P.linear_bias(y, Wq, bq), H)
        r = P.linear_bias_residual(a, Wp, bp, x)
        return P.linear_bias_gelu(r, W1, b1)

    def ref():
        y = F.layer_norm(x, (D,), g, b, 1e-6)
        qkv = F.linear(y, Wq, bq).reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
        att = ((qkv[0] @ qkv[1].transpose(-2, -1)) * (D // H) ** -0.5).softmax(-1)
        a = (att @ qkv[2]).transpose(1, 2).reshape(B, N, D)
        r = x + F.linear(a, Wp, bp)
        return F.gelu(F.linear(r, W1, b1))

    oh = hip()
    gh = torch.autograd.grad(oh.square().sum(), leaves)
    orf = ref()
    gr = torch.autograd.grad(orf.square().sum(), leaves)
    assert rel(oh, orf) < 1e-5
    for a, c, n in zip(gh, gr, "x g b Wq bq Wp bp W1 b1".split()):
        assert rel(a, c) < 2e-4, n
    # bf16 activations: the same chain runs on the bf16 MFMA kernels
    xb = x.detach().to(torch.bfloat16)
    ob = P.linear_bias_gelu(P.linear_bias(xb, Wq.detach()[:D].to(torch.bfloat16), bq.detach()[:D]), W1.detach().to(torch.bfloat16), b1.detach())
    want = F.gelu(F.linear(F.linear(xb.float(), Wq.detach()[:D].to(torch.bfloat16).float(), bq.detach()[:D]).to(torch.bfloat16).float(),
                           W1.detach().to(torch.bfloat16).float(), b1.detach()))
    assert ob.dtype == torch.bfloat16 and rel(ob.float(), want) < 2e-2


@pytest.mark.parametrize("K,dims", [
    (4032, [(768, 3072), (3072, 768), (768, 768), (2304, 768)]),     # ViT-B block: 108 tiles of 256x256
    (2048 + 64, [(512, 2048), (2048, 512), (512, 512), (1536, 512)]),  # MAE decoder block, short K: 256x128 tiles
    (16384 + 32, [(512, 2048), (2048, 512), (512, 512), (1536, 512)]),  # MAE decoder block, long K: 48 tiles x 4 ragged k-slices
    (2080, [(264, 136), (520, 648)])])                               # ragged tiles in both dimensions
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_wgrad_group(K, dims, prec):
    """pm_wgrad_group: every weight gradient of a block in one launch (full-K tiles, or k-slices + one reduce launch for a
    group of few tiles), store and accumulate, against torch.matmul in f32 on the same 16-bit operands; and bit-identical from
    run to run (no atomics: fixed reduction order)."""
    k = _k(prec)
    bf = k.act_dtype
    items, want = [], []
    for j, (n_out, n_in) in enumerate(dims):
        dy = rnd(K, n_out, seed=400 + j, scale=0.5).to(bf)
        x = rnd(K, n_in, seed=410 + j, scale=0.5).to(bf)
        acc = j % 2 == 1
        base = rnd(n_out, n_in, seed=420 + j) if acc else torch.full((n_out, n_in), float("nan"), device=DEV)
        dW = base.clone()
        db = rnd(n_out, seed=430 + j) if j != 2 else None  # bias gradient (+=) beside the GEMM for all but one problem
        items.append((dy, x, dW, acc, db))
        want.append((dy.float().t() @ x.float() + (base if acc else 0), None if db is None else db + dy.float().sum(0)))
    k.GROUP_MIN_TILES = 0  # (the engine groups only stacks with >= 64 tiles of 256x256; here every tile shape is exercised)
    assert k.can_group_wgrad(K, dims)
    assert k.wgrad_group(items, K)
    tol = 3e-5 * math.sqrt(K / 32)
    for (dy, x, dW, acc, db), (w, wb) in zip(items, want):
        assert rel(dW, w) < tol
        if db is not None:
            assert rel(db, wb) < 1e-5  # exact bf16 values summed in f32 on the matrix cores
    first = [(it[2].clone(), None if it[4] is None else it[4].clone()) for it in items]
    for j, (dy, x, dW, acc, db) in enumerate(items):
        if acc:
            dW.copy_(rnd(*dW.shape, seed=420 + j))
        if db is not None:
            db.copy_(rnd(db.numel(), seed=430 + j))
    assert k.wgrad_group(items, K)
    for (a, b), (_, _, dW, _, db) in zip(first, items):
        assert torch.equal(a, dW) and (db is None or torch.equal(b, db))
    # shapes outside the grouped kernel are refused with PM_ESHAPE (the engine then takes the per-GEMM path)
    assert not k.can_group_wgrad(2048 + 8, dims) and not k.can_group_wgrad(1024, dims)
    assert not k.wgrad_group(items, 1024)


def test_wgrad_group_whole_k_flag():
    """max_blocks = PM_GROUP_WHOLE_K (pm_vit_block_bwd's second launch: proj + qkv of a ViT-B block, 36 tiles): the plan would cut
    this group into k-slices; with the flag it runs whole-K 256x256 tiles without a workspace -- and every tile then sums in the
    same order as inside the unsliced four-problem group of the block, so the two agree bit for bit."""
    import ctypes
    from ssl4polyp_amd import _lib
    k = _k("bf16")
    bf = torch.bfloat16
    K, D = 12608, 768  # (64 x 197 tokens: long enough for the plan to slice the small group)
    dims = ((D, 4 * D), (4 * D, D), (D, D), (3 * D, D))
    ops = []
    for j, (n_out, n_in) in enumerate(dims):
        ops.append((rnd(K, n_out, seed=500 + j, scale=0.5).to(bf), rnd(K, n_in, seed=510 + j, scale=0.5).to(bf)))

    def items(sel, fill):
        out = []
        for j in sel:
            n_out, n_in = dims[j]
            out.append((ops[j][0], ops[j][1], torch.full((n_out, n_in), fill, device=DEV), False,
                        torch.zeros(n_out, device=DEV) if j in (1, 3) else None))
        return out

    def launch(its, max_blocks):
        n = len(its)
        arr = (_lib.WgradItem * n)()
        for j, (dy, x, dW, acc, db) in enumerate(its):
            n_out, n_in = dW.shape
            arr[j] = _lib.WgradItem(dy.data_ptr(), n_out, x.data_ptr(), n_in, dW.data_ptr(), n_in, n_out, n_in, 0,
                                    db.data_ptr() if db is not None else None)
        slices = ctypes.c_int(0)
        assert k.lib.pm_wgrad_group_plan(arr, n, K, _lib.PM_BF16, None, None, ctypes.byref(slices)) == 0
        _lib.check(k.lib.pm_wgrad_group(arr, n, K, _lib.PM_BF16, max_blocks, None, 0, torch.cuda.current_stream().cuda_stream),
                   "pm_wgrad_group")
        torch.cuda.synchronize()
        return slices.value

    whole = items(range(4), float("nan"))
    assert launch(whole, 0) == 1                      # 108 tiles: whole-K by itself
    small = items((2, 3), float("nan"))
    assert launch(small, _lib.PM_GROUP_WHOLE_K) > 1   # 36 tiles: the plan alone would slice ...
    for a, b in zip(small, whole[2:]):                # ... the flag keeps whole-K tiles: same bits as in the big group
        assert torch.equal(a[2], b[2])
        assert (a[4] is None) == (b[4] is None) and (a[4] is None or torch.equal(a[4], b[4]))
    assert rel(small[1][2], ops[3][0].float().t() @ ops[3][1].float()) < 3e-5 * math.sqrt(K / 32)


def test_mae_noise_is_the_counter_based_generator_bit_for_bit():
    """pm_mae_noise (Philox4x32-10, the noise of random_masking, models_mae.py:132) against oracle/noise_ref.py -- itself
    pinned by Random123's known-answer vectors -- for odd sizes, 64-bit seeds and several streams; and the model-level contract:
    re-seeding torch replays the same masks, consecutive forwards draw different ones."""
    import numpy as np
    from oracle.noise_ref import mae_noise
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    lib = _lib.load()
    for n, seed, sid in ((196 * 5, 0, 0), (1, 7, 3), (50177, 0xDEADBEEFCAFEF00D, 4000000000), (4096, 2 ** 63 + 5, 1)):
        out = torch.full((n,), -1.0, device=DEV)
        _lib.check(lib.pm_mae_noise(_ptr(out), n, seed, sid, _stream()), "pm_mae_noise")
        assert np.array_equal(out.cpu().numpy(), mae_noise(n, seed, sid)), (n, seed, sid)
    import ssl4polyp_amd as A
    m = A.MaskedAutoencoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                               decoder_num_heads=1, precision="fp32").to(DEV)
    x = torch.randn(4, 3, 32, 32, device=DEV)
    torch.manual_seed(5)
    with torch.no_grad():
        a1, a2 = m(x)[2].clone(), m(x)[2].clone()
        torch.manual_seed(5)
        b1 = m(x)[2].clone()
        torch.manual_seed(6)
        c1 = m(x)[2].clone()
    assert torch.equal(a1, b1) and not torch.equal(a1, a2) and not torch.equal(a1, c1)
    want = torch.from_numpy(mae_noise(4 * 16, 5, 0)).view(4, 16)   # seed 5, device-generator offset 0 right after the re-seed
    from oracle.vit_mae_ref import masking_from_noise
    assert torch.equal(a1.cpu(), masking_from_noise(want, 0.75)[1])
