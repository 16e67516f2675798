"""The MAE kernels of pm_mae.hip at their edges (tests/rowops_cases.py): masking (every L that changes the elements per thread, mass
ties, keep = 0 and L), the decoder un-shuffle and its backward (three activation types, both mask-token reductions, the grid caps) and
the fused patchify + loss (every slot count, both row layouts, padded pitches, norm_pix with constant and offset patches, three
masks, d loss != 1).  Masking, the un-shuffle and demb are held to bits; dmask_token, patch_loss and the loss to n 2^-24 T; dpred to the
bound derived from the target's rounding points (tests/rowops_ref.py, tests/test_rowops_ref_cpu.py).  Outputs lie NaN-filled between
guards.  Each test prints its largest err / bound (`pytest -s`)."""
import pytest
import torch

import rowops_cases as C
import rowops_ref as R
from test_gpu_attention_edges import GUARD, _guarded, _guards_hold
from test_gpu_token_path_edges import abi, code, status, untouched

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _guarded_int(shape):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), 7, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(-1)
    return buf, view


def _int_guards_hold(buf, what):
    assert bool((buf[:GUARD] == 7).all()) and bool((buf[-GUARD:] == 7).all()), what + ": written outside the buffer"


# ---- masking -------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", C.NOISE)
@pytest.mark.parametrize("L", C.MASK_L)
def test_masking(L, regime):
    """ids_shuffle is torch.argsort(stable=True) of the noise, ids_restore its inverse, mask = rank >= len_keep: B = 1 and 3, every
    len_keep of {0, 1, L / 4, L}."""
    for B in (1, 3):
        noise = C.noise(B, L, regime)
        for keep in C.keeps(L):
            sb, ids_shuffle = _guarded_int((B, L))
            rb, ids_restore = _guarded_int((B, L))
            mb, mask = _guarded((B, L), f32)
            assert abi("pm_mae_masking", noise.to(DEV), ids_shuffle, ids_restore, mask, B, L, keep) == 0
            torch.cuda.synchronize()
            _int_guards_hold(sb, "ids_shuffle")
            _int_guards_hold(rb, "ids_restore")
            _guards_hold(mb, "mask")
            want_s, want_r, want_m = R.masking(noise, keep)
            assert torch.equal(ids_shuffle.cpu(), want_s), (B, L, keep, regime)
            assert torch.equal(ids_restore.cpu(), want_r)
            assert torch.equal(mask.cpu(), want_m)
            assert torch.equal(torch.gather(ids_restore.cpu().long(), 1, ids_shuffle.cpu().long()), torch.arange(L).expand(B, L))
            if regime == "equal":
                assert torch.equal(ids_shuffle.cpu(), torch.arange(L, dtype=torch.int32).expand(B, L))   # all ties: the identity
            assert mask.sum().item() == B * (L - keep)


@pytest.mark.parametrize("what,L,keep,null,want", [("L = 1025", 1025, 4, False, "ESHAPE"), ("keep > L", 16, 17, False, "ESHAPE"),
                                                   ("keep < 0", 16, -1, False, "ESHAPE"), ("mask NULL", 16, 4, True, "EINVAL")])
def test_masking_refusals(what, L, keep, null, want):
    noise = torch.zeros(2, 1025, device=DEV)
    sb, ids_shuffle = _guarded_int((2, 1025))
    rb, ids_restore = _guarded_int((2, 1025))
    mb, mask = _guarded((2, 1025), f32)
    assert abi("pm_mae_masking", noise, ids_shuffle, ids_restore, None if null else mask, 2, L, keep) == status(want), what
    torch.cuda.synchronize()
    assert bool((ids_shuffle == -1).all()) and bool((ids_restore == -1).all()) and untouched(mb)


# ---- un-shuffle ----------------------------------------------------------------------------------
def _perm(B, L, seed=80):
    ids_shuffle = torch.stack([torch.randperm(L, generator=C.gen(seed + b)) for b in range(B)])
    return ids_shuffle.int().to(DEV), torch.argsort(ids_shuffle, dim=1).int().to(DEV)


@pytest.mark.parametrize("B,L,keep,D", C.UNSHUFFLE)
def test_unshuffle(B, L, keep, D):
    _, ids_restore = _perm(B, L)
    emb, tok, dpos = C.randn(B, keep + 1, D, seed=81).to(DEV), C.randn(D, seed=82).to(DEV), C.randn(L + 1, D, seed=83).to(DEV)
    if keep == L:
        tok = torch.full((D,), float("nan"), device=DEV)   # never used
    buf, out = _guarded((B, L + 1, D), f32)
    assert abi("pm_mae_unshuffle", emb, tok, dpos, ids_restore, out, B, L, keep, D) == 0
    torch.cuda.synchronize()
    _guards_hold(buf, "unshuffle")
    assert torch.equal(out, R.unshuffle(emb, tok, dpos, ids_restore, B, L, keep, D))


def _ws_rows(B, L, keep):
    return min((B * (L - keep) + 63) // 64, 1024)


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("ws", ["exact", "short", "none"])
@pytest.mark.parametrize("B,L,keep,D", C.UNSHUFFLE[1:4] + ((3, 200, 50, 68),))
def test_unshuffle_bwd(B, L, keep, D, ws, prec):
    """demb in the three types (bits); dmask_token, with prior contents, through the partial rows of a workspace of exactly the needed
    size, and through the atomics of one 4 bytes short or absent."""
    ids_shuffle, _ = _perm(B, L)
    dout, prior = C.randn(B, L + 1, D, seed=84).to(DEV), C.randn(D, seed=85).to(DEV)
    need = _ws_rows(B, L, keep) * D * 4
    wbuf, wsp = _guarded((need // 4,), f32)
    db, demb = _guarded((B, keep + 1, D), R.DTYPES[prec])
    mb, dmask = _guarded((D,), f32)
    dmask.copy_(prior)
    nbytes = {"exact": need, "short": need - 4, "none": 0}[ws]
    assert abi("pm_mae_unshuffle_bwd", dout, ids_shuffle, demb, code(demb.dtype), dmask, B, L, keep, D, None if ws == "none" else wsp, nbytes) == 0
    torch.cuda.synchronize()
    for buf, name in ((wbuf, "workspace"), (db, "demb"), (mb, "dmask_token")):
        _guards_hold(buf, name)
    if ws != "exact":
        assert untouched(wbuf)   # too small a workspace is not used at all
    ref = R.unshuffle_bwd(dout, ids_shuffle, B, L, keep, D, prior)
    assert torch.equal(demb, ref["demb"].to(R.DTYPES[prec]))
    r = R.ratio(dmask, ref["dmask"], R.sum_bound(ref["n"], ref["t_dmask"]))
    print(f"dmask_token B={B} L={L} keep={keep} D={D} ws={ws}: err/bound {r:.3f}")
    assert r <= 1.0


def test_unshuffle_bwd_keep_all_and_row_cap():
    """keep = L: no masked position, dmask_token untouched (NaN).  B = 70, L = 1024, keep = 64: 67200 masked positions, the first
    stage capped at 1024 block rows; demb rows past the 4096-workgroup cap."""
    B, L, D = 2, 9, 68
    ids_shuffle, _ = _perm(B, L)
    dout = C.randn(B, L + 1, D, seed=86).to(DEV)
    db, demb = _guarded((B, L + 1, D), torch.bfloat16)
    mb, dmask = _guarded((D,), f32)
    assert abi("pm_mae_unshuffle_bwd", dout, ids_shuffle, demb, 1, dmask, B, L, L, D, None, 0) == 0
    torch.cuda.synchronize()
    assert untouched(mb)
    assert torch.equal(demb, R.unshuffle_bwd(dout, ids_shuffle, B, L, L, D, torch.zeros(D, device=DEV))["demb"].to(torch.bfloat16))
    B, L, keep, D = C.UNSHUFFLE_BWD_CAP
    assert _ws_rows(B, L, keep) == 1024 and B * (L - keep) > 65536
    ids_shuffle, _ = _perm(B, L)
    dout = C.randn(B, L + 1, D, seed=87).to(DEV)
    db, demb = _guarded((B, keep + 1, D), f32)
    dmask = torch.zeros(D, device=DEV)
    from ssl4polyp_amd.engine import Kernels
    Kernels("fp32").mae_unshuffle_bwd(dout, ids_shuffle, demb, dmask, B, L, keep, D)
    torch.cuda.synchronize()
    _guards_hold(db, "demb")
    ref = R.unshuffle_bwd(dout, ids_shuffle, B, L, keep, D, torch.zeros(D, device=DEV))
    assert torch.equal(demb, ref["demb"])
    r = R.ratio(dmask, ref["dmask"], R.sum_bound(ref["n"], ref["t_dmask"]))
    print(f"dmask_token row cap: err/bound {r:.3f}")
    assert r <= 1.0


# ---- loss ----------------------------------------------------------------------------------------
def _loss_run(imgs, pred, mask, p, norm_pix, hc, ldp, lddp, prec, dloss, what):
    """pred [B, L, PE] laid into NaN-filled rows of ldp (with a cls row when hc).  -> patch_loss, sums, loss, dpred [B, L + hc, lddp]."""
    B, Cc, img, _ = imgs.shape
    L, PE = pred.shape[1], pred.shape[2]
    full = torch.full((B, L + hc, ldp), float("nan"), device=DEV)
    full[:, hc:, :PE] = pred
    pb, patch_loss = _guarded((B, L), f32)
    sums, loss = torch.full((2,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    assert abi("pm_mae_loss_fwd", imgs, full, ldp, hc, patch_loss, B, Cc, img, p, norm_pix) == 0
    assert abi("pm_mae_loss_finish", patch_loss, mask, B * L, sums, loss) == 0
    db, dpred = _guarded((B, L + hc, lddp), R.DTYPES[prec])
    dl = torch.tensor([dloss], device=DEV)
    assert abi("pm_mae_loss_bwd", imgs, full, ldp, hc, mask, sums, dl, dpred, lddp, code(dpred.dtype), B, Cc, img, p, norm_pix) == 0
    torch.cuda.synchronize()
    _guards_hold(pb, what + " patch_loss")
    _guards_hold(db, what + " dpred")
    return patch_loss, sums, loss, dpred


def _loss_check(imgs, pred, mask, p, norm_pix, hc, ldp, lddp, prec, dloss, what):
    patch_loss, sums, loss, dpred = _loss_run(imgs, pred, mask, p, norm_pix, hc, ldp, lddp, prec, dloss, what)
    PE = pred.shape[2]
    ref = R.mae_loss(imgs, pred, mask, p, norm_pix, dloss)
    fin = R.loss_finish(patch_loss, mask)   # the scalar against the patch losses it was given
    assert sums[1].item() == mask.sum().item()
    r = {"patch_loss": R.ratio(patch_loss, ref["patch_loss"], ref["e_patch"]), "loss": R.ratio(loss[0], fin["loss"], fin["e_loss"]),
         "sums[0]": R.ratio(sums[0], fin["loss"] * fin["sum_mask"], fin["e_loss"] * fin["sum_mask"]),
         "dpred": R.ratio(dpred[:, hc:, :PE], ref["dpred"], R.store_bound(ref["e_dpred"], ref["dpred"], prec))}
    for k, v in r.items():
        print(f"{what} {k}: err/bound {v:.3f}")
    for k, v in r.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of its bound"
    zero = torch.zeros((), dtype=dpred.dtype, device=DEV)
    assert bool((dpred[:, :hc] == zero).all()), what + ": cls rows of dpred"
    assert bool((dpred[:, :, PE:] == zero).all()), what + ": row padding of dpred"
    assert bool((dpred[:, hc:][mask == 0] == zero).all()), what + ": kept patches of dpred"


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("img,p,Cc", C.LOSS)
def test_loss(img, p, Cc, norm_pix, prec):
    """Every slot count; per mask one layout: (cls row, ldp = PE, lddp padded) / (no cls row, ldp = PE + 4) / (cls row, both wider)."""
    B = 2
    imgs, pred, masks = C.loss_inputs(B, img, p, Cc)
    imgs, pred = imgs.to(DEV), pred.to(DEV)
    PE = p * p * Cc
    layouts = {"ones": (1, PE, (PE + 63) // 64 * 64), "single": (0, PE + 4, PE), "random": (1, PE + 4, PE + 8)}
    for mname, mask in masks.items():
        hc, ldp, lddp = layouts[mname]
        _loss_check(imgs, pred, mask.to(DEV), p, norm_pix, hc, ldp, lddp, prec, 0.37,
                    f"loss img={img} p={p} C={Cc} norm_pix={norm_pix} mask={mname} {prec}")


def test_loss_grid_cap():
    B, img, p, Cc = C.LOSS_GRID   # 33024 patches: past 4 x 8192
    imgs, pred, masks = C.loss_inputs(B, img, p, Cc)
    _loss_check(imgs.to(DEV), pred.to(DEV), masks["random"].to(DEV), p, 1, 1, 4, 4, "fp32", 1.0, "loss grid cap")


@pytest.mark.parametrize("what", ["fwd ldp < PE", "bwd ldp < PE", "bwd lddp < PE", "bwd lddp % 4", "fwd PE > 1024", "fwd PE % 4", "fwd img % p",
                                  "fwd NULL", "bwd dtype", "finish n"])
def test_loss_refusals(what):
    """Rejected before any launch (a row of pred shorter than a patch included): the exact status, outputs untouched."""
    src = torch.zeros(8192, device=DEV)
    buf, dst = _guarded((8192,), f32)
    got, want = {
        "fwd ldp < PE": lambda: (abi("pm_mae_loss_fwd", src, src, 44, 1, dst, 1, 3, 16, 4, 0), "ESHAPE"),
        "bwd ldp < PE": lambda: (abi("pm_mae_loss_bwd", src, src, 44, 1, src, src, src, dst, 48, 0, 1, 3, 16, 4, 0), "ESHAPE"),
        "bwd lddp < PE": lambda: (abi("pm_mae_loss_bwd", src, src, 48, 1, src, src, src, dst, 44, 0, 1, 3, 16, 4, 0), "ESHAPE"),
        "bwd lddp % 4": lambda: (abi("pm_mae_loss_bwd", src, src, 48, 1, src, src, src, dst, 50, 0, 1, 3, 16, 4, 0), "ESHAPE"),
        "fwd PE > 1024": lambda: (abi("pm_mae_loss_fwd", src, src, 1200, 1, dst, 1, 3, 40, 20, 0), "ESHAPE"),
        "fwd PE % 4": lambda: (abi("pm_mae_loss_fwd", src, src, 28, 1, dst, 1, 3, 9, 3, 0), "ESHAPE"),
        "fwd img % p": lambda: (abi("pm_mae_loss_fwd", src, src, 48, 1, dst, 1, 3, 18, 4, 0), "ESHAPE"),
        "fwd NULL": lambda: (abi("pm_mae_loss_fwd", src, None, 48, 1, dst, 1, 3, 16, 4, 0), "EINVAL"),
        "bwd dtype": lambda: (abi("pm_mae_loss_bwd", src, src, 48, 1, src, src, src, dst, 48, 6, 1, 3, 16, 4, 0), "EINVAL"),
        "finish n": lambda: (abi("pm_mae_loss_finish", src, src, 0, dst, dst), "ESHAPE"),
    }[what]()
    torch.cuda.synchronize()
    assert got == status(want), what
    assert untouched(buf)
