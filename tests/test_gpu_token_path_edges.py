"""The token path of pm_misc.hip at its edges (tests/rowops_cases.py): im2col, pad_cast / unpad_add, token assembly and its
backward (every optional pointer, every trip count of cls_grad_kernel's loops), the row gather / scatter of the sparse top block and
the f32 -> 16-bit cast.  The data movers and single-rounding kernels are held to the bits of torch's own f32 add / .to(dtype)
(NaN by NaN-ness); dcls and dpos to n 2^-24 T per element (tests/rowops_ref.py, tests/test_rowops_ref_cpu.py).  Every output lies
NaN-filled between guards.  Each sum test prints its largest err / bound (`pytest -s`)."""
import pytest
import torch

import rowops_cases as C
import rowops_ref as R
from test_gpu_attention_edges import GUARD, _guarded, _guards_hold

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def abi(name, *args):
    """A C-ABI call with tensors passed as their device pointers and the current stream appended; -> the status."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _stream
    return getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream())


def code(dtype):
    from ssl4polyp_amd import _lib
    return _lib.dtype_code(dtype)


def status(name):
    from ssl4polyp_amd import _lib
    return getattr(_lib, "PM_" + name)


def _k(prec):
    from ssl4polyp_amd.engine import Kernels
    return Kernels(prec)


def untouched(buf):
    return bool(torch.isnan(buf[GUARD:-GUARD].float()).all())


# ---- im2col --------------------------------------------------------------------------------------
def _ids(mode, B, L):
    if mode == "null":
        return None, L
    keep = {"one": 1, "perm": L, "quarter": max(L // 4, 1)}[mode]
    return torch.stack([torch.randperm(L, generator=C.gen(60 + b))[:keep] for b in range(B)]).int().to(DEV), keep


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", C.IM2COL_KEEP)
@pytest.mark.parametrize("img,p,Cc", C.IM2COL)
def test_im2col(img, p, Cc, mode, B, prec):
    from ssl4polyp_amd.engine import Kernels
    imgs = C.randn(B, Cc, img, img, seed=3).to(DEV)
    ids, keep = _ids(mode, B, (img // p) ** 2)
    ld = Kernels.padded_k(Cc * p * p)
    dt = R.DTYPES[prec]
    buf, cols = _guarded((B * keep, ld), dt)
    assert abi("pm_patch_im2col", imgs, ids, cols, ld, code(dt), B, Cc, img, p, keep) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "im2col")
    assert torch.equal(cols, R.im2col(imgs, p, ids, ld, dt))


# ---- pad_cast / unpad_add ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("rows,cols,rows_pad,cols_pad,lds,ldd", [
    (5, 7, 8, 12, 9, 16),            # row and column padding together, both pitches wider
    (3, 588, 3, 640, 588, 640),      # the patch-14 operand
    (1027, 1000, 1030, 1024, 1000, 1024)])   # 1030 x 1024 elements > 4096 x 256: the grid-stride loop
def test_pad_cast(rows, cols, rows_pad, cols_pad, lds, ldd, prec):
    dt = R.DTYPES[prec]
    src = C.randn(rows, lds, seed=4).to(DEV)
    buf, dst = _guarded((rows_pad, ldd), dt)
    assert abi("pm_pad_cast", src, lds, dst, ldd, code(dt), rows, cols, rows_pad, cols_pad) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "pad_cast")
    want = torch.zeros(rows_pad, cols_pad, dtype=dt, device=DEV)
    want[:rows, :cols] = src[:, :cols].to(dt)
    assert torch.equal(dst[:, :cols_pad], want)
    assert bool(torch.isnan(dst[:, cols_pad:].float()).all())   # between cols_pad and ldd: the canary


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,cols,lds,ldd", [(5, 7, 12, 9), (1027, 1000, 1024, 1000), (3, 588, 640, 588)])
def test_unpad_add(rows, cols, lds, ldd, accumulate):
    src = C.randn(rows, lds, seed=5).to(DEV)
    buf, dst = _guarded((rows, ldd), f32)
    prior = C.randn(rows, ldd, seed=6).to(DEV)
    dst.copy_(prior)
    dst[:, cols:] = float("nan")
    assert abi("pm_unpad_add", src, lds, dst, ldd, rows, cols, accumulate) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "unpad_add")
    assert torch.equal(dst[:, :cols], prior[:, :cols] + src[:, :cols] if accumulate else src[:, :cols])
    assert bool(torch.isnan(dst[:, cols:]).all())   # the destination's padding


# ---- token assembly ------------------------------------------------------------------------------
def _keep_ids(B, keep, L, seed=70):
    return torch.stack([torch.randperm(L, generator=C.gen(seed + b))[:keep] for b in range(B)]).int().to(DEV)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("B,keep,D", C.ASSEMBLE)
def test_assemble_tokens(B, keep, D, with_ids):
    L = keep + 3 if with_ids else keep
    emb, cls, pos = C.randn(B * keep, D, seed=7).to(DEV), C.randn(D, seed=8).to(DEV), C.randn(L + 1, D, seed=9).to(DEV)
    ids = _keep_ids(B, keep, L) if with_ids else None
    buf, x = _guarded((B, keep + 1, D), f32)
    assert abi("pm_assemble_tokens", emb, cls, pos, ids, x, B, keep, D) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "assemble_tokens")
    assert torch.equal(x, R.assemble(emb, cls, pos, ids, B, keep, D))


def _assemble_bwd(B, keep, D, prec, ids, dcls, dpos, what):
    dx = C.randn(B, keep + 1, D, seed=10).to(DEV)
    buf, demb = _guarded((B * keep, D), R.DTYPES[prec])
    assert abi("pm_assemble_tokens_bwd", dx, ids, demb, code(demb.dtype), dcls, dpos, B, keep, D) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, what + " demb")
    return dx, demb


def _sum_check(got, want, t, n, what):
    r = R.ratio(got, want, R.sum_bound(n, t))
    print(f"{what}: err/bound {r:.3f}")
    assert r <= 1.0, f"{what} at {r:.3f} of its bound"


@pytest.mark.parametrize("D", C.CLS_D)
@pytest.mark.parametrize("B", C.CLS_B)
def test_cls_grad_loops(B, D):
    """dcls (with prior contents) at every trip count of cls_grad_kernel's unrolled body and tail, ragged column blocks; dpos = NULL:
    nothing else is written."""
    keep = 2
    pb, dcls = _guarded((D,), f32)
    prior = C.randn(D, seed=32, scale=3.0).to(DEV)
    dcls.copy_(prior)
    dx, demb = _assemble_bwd(B, keep, D, "fp32", None, dcls, None, "cls_grad")
    _guards_hold(pb, "dcls")
    ref = R.assemble_bwd(dx, None, B, keep, D, dcls0=prior)
    assert torch.equal(demb, ref["demb"])
    _sum_check(dcls, ref["dcls"], ref["t_dcls"], ref["n"], f"dcls B={B} D={D}")


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("mode", ["both", "both_prior", "dpos_only", "dcls_only", "neither"])
def test_assemble_bwd_optional_pointers(mode, prec):
    """Every combination of dcls / dpos, the same patch id drawn by several samples (17 samples, 5 of 8 ids each).  dcls = NULL with
    dpos given: dpos[0] still receives sum_b dx[b, 0] (the header's `dpos += scatter of dx`)."""
    B, keep, L, D = 17, 5, 8, 68
    ids = _keep_ids(B, keep, L)
    cb, dcls = _guarded((D,), f32)
    pb, dpos = _guarded((L + 1, D), f32)
    prior_c = C.randn(D, seed=33).to(DEV) if mode == "both_prior" else torch.zeros(D, device=DEV)
    prior_p = C.randn(L + 1, D, seed=34).to(DEV) if mode == "both_prior" else torch.zeros(L + 1, D, device=DEV)
    use_c, use_p = mode in ("both", "both_prior", "dcls_only"), mode in ("both", "both_prior", "dpos_only")
    if use_c:
        dcls.copy_(prior_c)
    if use_p:
        dpos.copy_(prior_p)
    dx, demb = _assemble_bwd(B, keep, D, prec, ids, dcls if use_c else None, dpos if use_p else None, mode)
    _guards_hold(cb, "dcls")
    _guards_hold(pb, "dpos")
    ref = R.assemble_bwd(dx, ids, B, keep, D, dcls0=prior_c, dpos0=prior_p)
    assert torch.equal(demb, ref["demb"].to(R.DTYPES[prec]))
    if use_c:
        _sum_check(dcls, ref["dcls"], ref["t_dcls"], ref["n"], f"dcls {mode}")
    else:
        assert untouched(cb)
    if use_p:
        _sum_check(dpos, ref["dpos"], ref["t_dpos"], ref["n"], f"dpos {mode}")
        if mode == "both":   # one sum, stored twice
            assert torch.equal(dpos[0], dcls)
    else:
        assert untouched(pb)


def test_assemble_bwd_grid_cap():
    B, keep, D = 130, 127, 4   # 16510 rows of demb: past the 4096-workgroup cap
    dx, demb = _assemble_bwd(B, keep, D, "bf16", None, None, None, "grid")
    assert torch.equal(demb, R.assemble_bwd(dx, None, B, keep, D)["demb"].to(torch.bfloat16))


# ---- gather / scatter ----------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", C.GATHER_ROW_BYTES)
@pytest.mark.parametrize("pad_bytes", [0, 8])
def test_gather_rows(row_bytes, pad_bytes):
    """Repeated and descending indices, a source pitch wider than the row."""
    rows, w, ldw = 9, row_bytes // 4, (row_bytes + pad_bytes) // 4
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, ldw), generator=C.gen(12), dtype=torch.int64).int().to(DEV)
    idx = torch.tensor([8, 7, 7, 3, 0, 0, 8, 1], dtype=torch.int32, device=DEV)
    buf = torch.full((idx.numel() * w + 2 * GUARD,), 7, dtype=torch.int32, device=DEV)
    dst = buf[GUARD:-GUARD].view(idx.numel(), w)
    assert abi("pm_gather_rows", src, ldw * 4, idx, dst, idx.numel(), row_bytes) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 7).all()) and bool((buf[-GUARD:] == 7).all())
    assert torch.equal(dst, src[idx.long(), :w])


@pytest.mark.parametrize("row_bytes", C.SCATTER_ROW_BYTES)
@pytest.mark.parametrize("mode", ["all", "none", "mixed"])
def test_scatter_rows_zero(row_bytes, mode):
    M, R_, w = 11, 4, row_bytes // 2
    src = C.randn(R_, w, seed=13).to(torch.bfloat16).to(DEV)
    inv = {"all": torch.full((M,), -1), "none": torch.arange(M) % R_, "mixed": torch.tensor([-1, 2, -1, -1, 0, 3, -1, 1, -1, -1, 2])}[mode].int().to(DEV)
    buf, dst = _guarded((M, w), torch.bfloat16)
    _k("bf16").scatter_rows_zero(src, inv, dst)
    torch.cuda.synchronize()
    _guards_hold(buf, "scatter_rows_zero")
    want = torch.where((inv >= 0)[:, None], src[inv.clamp_min(0).long()], torch.zeros_like(dst))
    assert torch.equal(dst, want)


def test_gather_scatter_round_trip_and_grid_caps():
    """One case past each grid cap (4096 and 8192 workgroups), through engine.Kernels, and scatter(gather(x, idx), inv) = x on the
    rows idx names, zero elsewhere."""
    k = _k("bf16")
    R_, rb = C.GATHER_GRID
    x = C.randn(R_ + 7, rb // 4, seed=14).to(DEV)
    idx = torch.randperm(R_ + 7, generator=C.gen(15))[:R_].int().to(DEV)
    got = k.gather_rows(x, idx)
    assert torch.equal(got, x[idx.long()])
    M, rb = C.SCATTER_GRID
    rows = torch.arange(0, M, 3, dtype=torch.int32, device=DEV)
    inv = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    inv[rows.long()] = torch.arange(rows.numel(), dtype=torch.int32, device=DEV)
    big = torch.randn(M, rb // 4, generator=C.gen(16)).to(DEV)
    packed = k.gather_rows(big, rows)
    buf, dst = _guarded((M, rb // 4), f32)
    k.scatter_rows_zero(packed, inv, dst)
    torch.cuda.synchronize()
    _guards_hold(buf, "scatter_rows_zero")
    want = torch.zeros_like(big)
    want[rows.long()] = big[rows.long()]
    assert torch.equal(dst, want)


@pytest.mark.parametrize("what", ["gather row_bytes", "gather ld_bytes", "gather src", "gather dst", "gather ld < row", "gather NULL",
                                  "scatter row_bytes", "scatter src", "scatter dst", "scatter NULL"])
def test_gather_scatter_refusals(what):
    src = torch.zeros(64, dtype=f32, device=DEV)
    buf, dst = _guarded((64,), f32)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    sp, dp = src.data_ptr(), dst.data_ptr()
    got, want = {
        "gather row_bytes": lambda: (abi("pm_gather_rows", sp, 16, idx, dp, 2, 6), "EALIGN"),
        "gather ld_bytes": lambda: (abi("pm_gather_rows", sp, 18, idx, dp, 2, 16), "EALIGN"),
        "gather src": lambda: (abi("pm_gather_rows", sp + 2, 16, idx, dp, 2, 16), "EALIGN"),
        "gather dst": lambda: (abi("pm_gather_rows", sp, 16, idx, dp + 2, 2, 16), "EALIGN"),
        "gather ld < row": lambda: (abi("pm_gather_rows", sp, 8, idx, dp, 2, 16), "ESHAPE"),
        "gather NULL": lambda: (abi("pm_gather_rows", sp, 16, None, dp, 2, 16), "EINVAL"),
        "scatter row_bytes": lambda: (abi("pm_scatter_rows_zero", sp, idx, dp, 2, 24), "EALIGN"),
        "scatter src": lambda: (abi("pm_scatter_rows_zero", sp + 8, idx, dp, 2, 16), "EALIGN"),
        "scatter dst": lambda: (abi("pm_scatter_rows_zero", sp, idx, dp + 8, 2, 16), "EALIGN"),
        "scatter NULL": lambda: (abi("pm_scatter_rows_zero", sp, None, dp, 2, 16), "EINVAL"),
    }[what]()
    torch.cuda.synchronize()
    assert got == status(want), what
    assert untouched(buf)


# ---- cast ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_cast_every_rounding_case(prec, tail):
    """327680 f32 bit patterns -- bf16 ties, fp16 ties and subnormals, overflow, infinities, NaNs -- and the exact fp16 half-way
    points, against torch's CPU conversion (round to nearest even; tests/test_rowops_ref_cpu.py holds that to integer arithmetic and
    numpy).  The table is rotated by `tail` and cut to n with n & 3 = tail, so the scalar tail `(T)v` meets tie values too."""
    dt = R.DTYPES[prec]
    table = torch.cat([C.cast_table(), C.fp16_tie_table()])
    table = torch.roll(table, 5 * tail + 2)
    n = (table.numel() & ~3) - 4 + tail
    src = table[:n].contiguous()
    buf, dst = _guarded((n,), dt)
    _k(prec).cast(src.to(DEV), dst)
    torch.cuda.synchronize()
    _guards_hold(buf, "cast")
    assert R.equal_bits(dst.cpu(), src.to(dt))


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_cast_fewer_than_four(n, prec):
    dt = R.DTYPES[prec]
    src = torch.tensor([0x3F808000, 0x3F818000, 0x38001000], dtype=torch.int32).view(f32)[:n].contiguous()   # bf16 ties to even / away, an fp16 subnormal tie
    buf, dst = _guarded((n,), dt)
    _k(prec).cast(src.to(DEV), dst)
    torch.cuda.synchronize()
    _guards_hold(buf, "cast")
    assert R.equal_bits(dst.cpu(), src.to(dt))


# ---- refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["im2col img % p", "im2col ldcols < PE", "im2col ldcols align", "im2col keep > L", "im2col NULL ids keep < L",
                                  "im2col dtype", "pad_cast ldd", "unpad lds", "assemble D", "assemble NULL", "assemble_bwd D",
                                  "assemble_bwd dtype", "cast n", "cast align"])
def test_refusals(what):
    """Rejected before any launch: the exact status, the NaN-filled output untouched."""
    src = torch.zeros(4096, dtype=f32, device=DEV)
    buf, dst = _guarded((4096,), f32)
    ids = torch.zeros(64, dtype=torch.int32, device=DEV)
    got, want = {
        "im2col img % p": lambda: (abi("pm_patch_im2col", src, None, dst, 48, 0, 1, 3, 18, 4, 16), "ESHAPE"),
        "im2col ldcols < PE": lambda: (abi("pm_patch_im2col", src, None, dst, 44, 0, 1, 3, 16, 4, 16), "ESHAPE"),
        "im2col ldcols align": lambda: (abi("pm_patch_im2col", src, None, dst, 50, 0, 1, 3, 16, 4, 16), "EALIGN"),
        "im2col keep > L": lambda: (abi("pm_patch_im2col", src, ids, dst, 48, 0, 1, 3, 16, 4, 17), "ESHAPE"),
        "im2col NULL ids keep < L": lambda: (abi("pm_patch_im2col", src, None, dst, 48, 0, 1, 3, 16, 4, 4), "ESHAPE"),
        "im2col dtype": lambda: (abi("pm_patch_im2col", src, None, dst, 48, 5, 1, 3, 16, 4, 16), "EINVAL"),
        "pad_cast ldd": lambda: (abi("pm_pad_cast", src, 8, dst, 8, 0, 4, 8, 4, 12), "ESHAPE"),
        "unpad lds": lambda: (abi("pm_unpad_add", src, 4, dst, 8, 4, 8, 0), "ESHAPE"),
        "assemble D": lambda: (abi("pm_assemble_tokens", src, src, src, None, dst, 2, 3, 6), "ESHAPE"),
        "assemble NULL": lambda: (abi("pm_assemble_tokens", src, None, src, None, dst, 2, 3, 8), "EINVAL"),
        "assemble_bwd D": lambda: (abi("pm_assemble_tokens_bwd", src, None, dst, 0, None, None, 2, 3, 6), "ESHAPE"),
        "assemble_bwd dtype": lambda: (abi("pm_assemble_tokens_bwd", src, None, dst, 9, None, None, 2, 3, 8), "EINVAL"),
        "cast n": lambda: (abi("pm_cast", src, dst, 1, 0), "ESHAPE"),
        "cast align": lambda: (abi("pm_cast", src.data_ptr() + 4, dst, 1, 16), "EALIGN"),
    }[what]()
    torch.cuda.synchronize()
    assert got == status(want), what
    assert untouched(buf)
