"""csrc/pm_augment.hip, the first-generation input pipeline, at its edges: every colour, every degenerate value, every op order, the
smallest legal blur, non-square and one-pixel rotations, resizes from one pixel and with many taps, strip crops, the refusals, and
grids that wrap.  The reference is Pillow called LIVE where Pillow has the routine (tests/augment_cases.py calls it as
tests/golden/make_augment_fixtures.py does), oracle/augment_ref.py for torchvision's Gaussian blur; tests/test_augment_edges_cpu.py holds
the oracle to Pillow at the same cases.  Bytes and f32 bit patterns only: no tolerance.  Every output buffer is filled with a pattern
before the launch, so an element a kernel skips shows.

Flat-grid wrap: aug_grid caps a launch at 8192 workgroups = 2,097,152 elements; the wrap tests run 2,162,688 (three 1024 x 704 frames),
so part of the grid takes a second trip through its grid-stride loop.  Two kernels have no wrap test here: occlude_kernel's grid is 64
workgroups per sample, so it already wraps on every rectangle above 16,384 bytes in tests/test_gpu_augment.py; jpeg_roundtrip_kernel's
cap of 65,535 workgroups x 64 blocks of 8 x 8 would need 268 M pixels."""
import numpy as np
import pytest
import torch

import augment_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_cache = {}


def _lib():
    from ssl4polyp_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _filled(shape, dtype=torch.uint8):
    """An output buffer no kernel result can be mistaken for: 0xA5 bytes, or NaNs."""
    return torch.full(shape, float("nan") if dtype == torch.float32 else 0xA5, dtype=dtype, device=DEV)


def _colours():
    if "host" not in _cache:
        _cache["host"] = C.all_colours()
        _cache["dev"] = _dev(_cache["host"][None])
    return _cache["host"], _cache["dev"]


def _jitter(xd, jit):
    L, lib = _lib()
    B, H, W, _ = xd.shape
    jd = _dev(jit)
    lsum = torch.zeros(B, dtype=torch.int64, device=DEV)
    out = _filled(xd.shape)
    L.check(lib.pm_aug_color_jitter_u8(xd.data_ptr(), out.data_ptr(), jd.data_ptr(), lsum.data_ptr(), B, H, W, _st()), "jitter")
    return out.cpu().numpy()


def _single_op(op, B, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0):
    bc = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))
    return C.jitter_records(np.tile(np.array([op, -1, -1, -1], dtype=np.int32), (B, 1)), bc(brightness), bc(contrast), bc(saturation), bc(hue))


# ---- 1. colour operations over their whole domain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,shift", C.HUE)
def test_hue_over_every_colour(factor, shift):
    """hue_shift on all 2^24 colours (one 4096 x 4096 frame) against convert("HSV"), a uint8 add on H, merge, convert("RGB")."""
    host, dev = _colours()
    jit = _single_op(3, 1, hue=factor)
    assert jit[0, 7] == shift
    C.assert_same_bytes(_jitter(dev, jit)[0], C.pil_hue(host, shift), f"hue shift {shift}")


@pytest.mark.parametrize("f", C.SATURATION)
def test_saturation_over_every_colour(f):
    host, dev = _colours()
    C.assert_same_bytes(_jitter(dev, _single_op(2, 1, saturation=f))[0], C.pil_saturation(host, f), f"saturation {f}")


def test_brightness_at_the_twentieths():
    """All 256 values of every channel at k / 20, k = 0 ... 40, one sample per factor in one launch, against ImageEnhance.Brightness."""
    a = C.brightness_frame()
    B = len(C.TWENTIETHS)
    got = _jitter(_dev(np.stack([a] * B)), _single_op(0, B, brightness=C.TWENTIETHS))
    for b, f in enumerate(C.TWENTIETHS):
        C.assert_same_bytes(got[b], C.pil_brightness(a, f), f"brightness {f}")


def test_contrast_at_every_degenerate_value_and_twentieth():
    """The blend against the mean luminance: every degenerate value 0 ... 255 occurs, 224 of them in a frame that also holds all 256
    pixel values (asserted below, with Pillow's own ImageStat), each at k / 20, k = 0 ... 40 -- both blend branches, both interval ends,
    the extrapolating side with its clamp, and the short decimals at which a fused multiply-add changes a byte.  One launch of
    41 x 264 small frames against ImageEnhance.Contrast per frame."""
    from PIL import Image, ImageEnhance
    frames = C.contrast_frames()
    means, full = C.contrast_coverage(frames)
    assert means == set(range(256)), sorted(set(range(256)) - means)
    assert len(full) >= 192, len(full)
    F, N = len(C.TWENTIETHS), len(frames)
    got = _jitter(_dev(np.tile(frames, (F, 1, 1, 1))), _single_op(1, F * N, contrast=np.repeat(C.TWENTIETHS, N))).reshape((F, N) + frames.shape[1:])
    for n in range(N):
        enh = ImageEnhance.Contrast(Image.fromarray(frames[n]))
        for k, f in enumerate(C.TWENTIETHS):
            C.assert_same_bytes(got[k, n], np.asarray(enh.enhance(f)), f"contrast {f}, frame {n}")


@pytest.mark.parametrize("H,W", C.ORDER_HW)
def test_every_op_order(H, W):
    """All 24 orders of the four ops (0, 1, 2 and 3 ops before the contrast inside the luminance pre-pass), the evaluation rows' order,
    an order without contrast (the pre-pass returns early), all-skip (identity) and a skip in front -- on an odd frame, on one pixel
    and on fewer pixels than a workgroup has threads."""
    B = len(C.PERMUTATIONS)
    x = C.noise((B, H, W, 3), 41 + H)
    xd = _dev(x)
    fac = C.order_factors(B)
    for orders in [C.PERMUTATIONS] + [(o,) * B for o in C.EXTRA_ORDERS]:
        got = _jitter(xd, C.jitter_records(np.array(orders, dtype=np.int32), *fac))
        for b in range(B):
            C.assert_same_bytes(got[b], C.pil_jitter(x[b], orders[b], *(v[b] for v in fac)), f"order {orders[b]}, sample {b}")
        if orders[0] == (-1, -1, -1, -1):
            C.assert_same_bytes(got, x, "all-skip is the identity")


def test_colour_jitter_and_occlusion_refuse_a_batch_past_the_grids_y_limit():
    """B is blockIdx.y: 65536 samples are refused with PM_ESHAPE before anything is enqueued (buffers of the true size, 1 x 1 frames)."""
    L, lib = _lib()
    B = 65536
    x = torch.zeros(B, 1, 1, 3, dtype=torch.uint8, device=DEV)
    out = _filled(x.shape)
    jit = _dev(_single_op(0, B, brightness=0.5))
    lsum = torch.zeros(B, dtype=torch.int64, device=DEV)
    rects = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    assert lib.pm_aug_color_jitter_u8(x.data_ptr(), out.data_ptr(), jit.data_ptr(), lsum.data_ptr(), B, 1, 1, _st()) == L.PM_ESHAPE
    assert lib.pm_aug_occlude_u8(out.data_ptr(), rects.data_ptr(), B, 1, 1, _st()) == L.PM_ESHAPE
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()), "a refused call wrote"
    assert lib.pm_aug_color_jitter_u8(x.data_ptr(), out.data_ptr(), jit.data_ptr(), lsum.data_ptr(), B - 1, 1, 1, _st()) == 0
    assert lib.pm_aug_occlude_u8(out.data_ptr(), rects.data_ptr(), B - 1, 1, 1, _st()) == 0
    torch.cuda.synchronize()
    assert bool((out[:B - 1] == 0).all()) and bool((out[B - 1] == 0xA5).all())


# ---- 2. Gaussian blur ----------------------------------------------------------------------------------------------------------------------
def _blur(x, ksize, sigmas):
    from ssl4polyp_amd.data import _gaussian_taps
    L, lib = _lib()
    B, H, W, _ = x.shape
    taps = _dev(_gaussian_taps(ksize, sigmas))
    assert taps.shape == (B, ksize)
    tmp = _filled((B, H, W, 3), torch.float32)
    out = _filled(x.shape)
    xd = _dev(x)   # (held until the call returns: a temporary's block could be handed to the next allocation)
    L.check(lib.pm_aug_gaussian_blur_u8(xd.data_ptr(), tmp.data_ptr(), out.data_ptr(), taps.data_ptr(), ksize, B, H, W, _st()), "blur")
    return out.cpu().numpy()


@pytest.mark.parametrize("ksize", C.BLUR_KSIZES)
@pytest.mark.parametrize("H,W", C.BLUR_HW)
def test_gaussian_blur_small_frames(H, W, ksize):
    """The smallest legal sides for 25 taps (every tap of a border pixel reflects), sigmas 0.001 ... 10 mixed in one batch (the taps of
    sample b start at taps + b * ksize), constant frames of 0 and 255, and 1 and 3 taps, against the oracle's separable f32 sum."""
    from oracle import augment_ref as R
    x, sigmas = C.blur_batch(H, W)
    got = _blur(x, ksize, sigmas)
    for b, sg in enumerate(sigmas):
        C.assert_same_bytes(got[b], R.gaussian_blur(x[b:b + 1], ksize, sg)[0], f"{H}x{W} ksize {ksize} sigma {sg}")


def test_gaussian_blur_refusals():
    L, lib = _lib()
    z = torch.zeros(1, 12, 40, 3, dtype=torch.uint8, device=DEV)
    t = torch.zeros(1, 12, 40, 3, dtype=torch.float32, device=DEV)
    taps = torch.zeros(1, 25, device=DEV)
    call = lambda k, H, W: lib.pm_aug_gaussian_blur_u8(z.data_ptr(), t.data_ptr(), z.data_ptr(), taps.data_ptr(), k, 1, H, W, _st())
    assert call(25, 12, 40) == L.PM_ESHAPE and call(25, 40, 12) == L.PM_ESHAPE   # a side of 12 under 25 taps: the pad reaches the size
    assert call(2, 12, 40) == L.PM_ESHAPE and call(24, 12, 40) == L.PM_ESHAPE     # even
    assert call(0, 12, 40) == L.PM_ESHAPE and call(-1, 12, 40) == L.PM_ESHAPE
    assert call(23, 12, 40) == 0                                                   # pad 11 < 12


# ---- 3. flips + rotation + normalise -------------------------------------------------------------------------------------------------------
def _geometry(x, geom, to_f32):
    L, lib = _lib()
    B, H, W, _ = x.shape
    out = _filled((B, 3, H, W), torch.float32) if to_f32 else _filled(x.shape)
    m, s = C.GEOM_MEAN, C.GEOM_STD
    xd, gd = _dev(x), _dev(geom)
    L.check(lib.pm_aug_geometry_u8(xd.data_ptr(), gd.data_ptr(), out.data_ptr(), 1 if to_f32 else 0, B, H, W, m[0], m[1], m[2],
                                   s[0], s[1], s[2], _st()), "geometry")
    return out.cpu()


def _geom_records(cases, H, W):
    from ssl4polyp_amd.data import _rotation_geom
    return np.array([_rotation_geom(a, W, H, f) for a, f in cases], dtype=np.int32)


@pytest.mark.parametrize("H,W", C.GEOM_HW)
def test_flips_and_rotation_on_small_and_non_square_frames(H, W):
    """18 angles x 4 flip combinations per size, one sample each, against Image.rotate of the flipped frame: on a non-square frame 90 and
    270 degrees take the fixed-point path (the transpose fast paths are legal for H = W only).  Then the same launch with to_f32 = 1
    against the oracle's ToTensor + Normalize of those bytes, with a mean and std that differ per channel."""
    from oracle.input_ref import to_tensor_normalize
    cases = C.geom_cases()
    x = C.noise((len(cases), H, W, 3), 7 * H + W)
    geom = _geom_records(cases, H, W)
    assert H == W or not np.isin(geom[:, 0], (3, 4)).any()
    assert H != W or {3, 4} <= set(geom[:, 0].tolist())
    want = np.stack([C.pil_flip_rotate(x[b], a, f) for b, (a, f) in enumerate(cases)])
    got = _geometry(x, geom, False).numpy()
    for b, case in enumerate(cases):
        C.assert_same_bytes(got[b], want[b], f"{H}x{W} (angle, flips) = {case}")
    f32 = _geometry(x, geom, True).numpy()
    C.assert_same_bytes(C.f32_bits(f32), C.f32_bits(to_tensor_normalize(torch.from_numpy(want), None, C.GEOM_MEAN, C.GEOM_STD).numpy()), f"{H}x{W} f32")


def test_geometry_refusals():
    L, lib = _lib()
    z = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    o = torch.zeros(1, 3, 8, 8, dtype=torch.float32, device=DEV)
    g = _dev(_geom_records([(0.0, 0)], 8, 8))
    call = lambda std, to_f32=1: lib.pm_aug_geometry_u8(z.data_ptr(), g.data_ptr(), o.data_ptr(), to_f32, 1, 8, 8, 0.5, 0.5, 0.5, *std, _st())
    for bad in (0.0, -0.25, float("nan")):
        for pos in range(3):
            std = [0.5, 0.5, 0.5]
            std[pos] = bad
            assert call(std) == L.PM_EINVAL, (bad, pos)
    assert call([0.5, 0.5, 0.5]) == 0 and call([0.0, 0.0, 0.0], 0) == 0   # (the u8 path does not read them)


# ---- 4. resampling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hs,Ws,S", C.RESIZE)
def test_resize_edges(Hs, Ws, S):
    from ssl4polyp_amd.data import DeviceAugmenter
    x = C.noise((1 if Hs * Ws > 1000000 else 2, Hs, Ws, 3), Hs + 3 * Ws)
    got = DeviceAugmenter(DEV, size=S).resize(_dev(x)).cpu().numpy()
    for b in range(len(x)):
        C.assert_same_bytes(got[b], C.pil_resize(x[b], S, S), f"{Hs}x{Ws}->{S}, frame {b}")


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("out", C.CROP_OUT)
def test_crop_edges(out, filt):
    """One-pixel and strip boxes, the whole frame (at 16: the largest tap count the workspace formula has to hold, so the "cannot happen"
    clamp of the tap count is checked by the bytes), against crop(...).resize(...)."""
    from ssl4polyp_amd.data import DeviceAugmenter
    H, W = C.CROP_HW
    boxes = np.array(C.CROP_BOXES, dtype=np.int32)
    x = C.noise((len(boxes), H, W, 3), 77 + out)
    got = DeviceAugmenter(DEV, size=out).random_resized_crop(_dev(x), boxes, bicubic=filt == "bicubic").cpu().numpy()
    for b, box in enumerate(boxes):
        C.assert_same_bytes(got[b], C.pil_resized_crop(x[b], box, out, filt), f"{tuple(box)}->{out} {filt}")


def test_crop_per_sample_grid_wraps():
    """B = 64: the per-sample cap is 128 workgroups = 32,768 threads against up to 300 x 224 outputs of the horizontal pass and 224 x 224 of
    the vertical one, so both loops take a second trip."""
    from ssl4polyp_amd.data import DeviceAugmenter
    B, (H, W) = 64, C.CROP_HW
    x = C.noise((B, H, W, 3), 64)
    boxes = C.drawn_boxes(B, H, W, 5)
    aug = DeviceAugmenter(DEV, size=224)
    xd = _dev(x)
    for filt in ("bicubic", "bilinear"):
        aug._scratch.exact("rrc_out", (B, 224, 224, 3), torch.uint8).fill_(0xA5)
        got = aug.random_resized_crop(xd, boxes, bicubic=filt == "bicubic").cpu().numpy()
        for b in range(B):
            C.assert_same_bytes(got[b], C.pil_resized_crop(x[b], boxes[b], 224, filt), f"sample {b} box {tuple(boxes[b])} {filt}")


@pytest.mark.parametrize("out", C.CROP_OUT)
def test_ragged_edges(out):
    """One packed batch of a 1 x 1, a 300 x 400, a 17 x 250 and a 250 x 17 frame: the Resize (whole frames, bilinear) and crops."""
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames
    frames = [C.noise((h, w, 3), h + w) for (h, w) in C.RAGGED_HW]
    rf = RaggedFrames.from_frames(frames).to(DEV)
    aug = DeviceAugmenter(DEV, size=out)
    got = aug.resize(rf).cpu().numpy()
    for b, f in enumerate(frames):
        C.assert_same_bytes(got[b], C.pil_resize(f, out, out), f"resize {f.shape[:2]}->{out}")
    boxes = np.array([(0, 0, 1, 1), (7, 9, 225, 223), (3, 100, 14, 150), (100, 3, 150, 14)], dtype=np.int32)
    for filt in ("bicubic", "bilinear"):
        got = aug.random_resized_crop(rf, boxes, bicubic=filt == "bicubic").cpu().numpy()
        for b, f in enumerate(frames):
            C.assert_same_bytes(got[b], C.pil_resized_crop(f, boxes[b], out, filt), f"crop {tuple(boxes[b])} of {f.shape[:2]}->{out} {filt}")


def test_resample_refusals():
    """One case for every refusing branch of pm_aug_resize_u8, pm_aug_resized_crop_u8 and pm_aug_resized_crop_ragged_u8."""
    from ssl4polyp_amd.data import _resample_coeffs
    L, lib = _lib()
    E, S = L.PM_EINVAL, L.PM_ESHAPE
    H, W, O = 9, 7, 4
    src = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    tmp = torch.zeros(1, H, O, 3, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(1, O, O, 3, dtype=torch.uint8, device=DEV)
    (bx, tx, kx), (by, ty, ky) = _resample_coeffs(W, O), _resample_coeffs(H, O)
    bx, tx, by, ty = (_dev(a) for a in (bx, tx, by, ty))
    p = lambda t: t.data_ptr()

    def resize(**kw):
        a = dict(src=p(src), tmp=p(tmp), dst=p(dst), bx=p(bx), tx=p(tx), kx=kx, by=p(by), ty=p(ty), ky=ky, B=1, Hs=H, Ws=W, Ho=O, Wo=O)
        a.update(kw)
        return lib.pm_aug_resize_u8(a["src"], a["tmp"], a["dst"], a["bx"], a["tx"], a["kx"], a["by"], a["ty"], a["ky"], a["B"], a["Hs"], a["Ws"],
                                    a["Ho"], a["Wo"], _st())
    assert resize(src=None) == E and resize(dst=None) == E and resize(tmp=None) == E
    assert resize(bx=None) == E and resize(tx=None) == E and resize(kx=0) == E
    assert resize(by=None) == E and resize(ty=None) == E and resize(ky=0) == E
    for k in ("B", "Hs", "Ws", "Ho", "Wo"):
        assert resize(**{k: 0}) == S, k
    assert resize() == 0
    # the resized crop, uniform and ragged
    need = int(lib.pm_aug_resized_crop_workspace_bytes(1, H, W, O))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    assert p(ws) % 16 == 0
    box = _dev(np.array([[0, 0, H, W]], dtype=np.int32))
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    hw = _dev(np.array([[H, W]], dtype=np.int32))

    def crop(ragged, **kw):
        a = dict(src=p(src), off=p(off), hw=p(hw), box=p(box), dst=p(dst), B=1, Hs=H, Ws=W, out=O, ws=p(ws), wsb=need)
        a.update(kw)
        tail = (a["box"], a["dst"], 1, a["B"], a["Hs"], a["Ws"], a["out"], a["ws"], a["wsb"], _st())
        if ragged:
            return lib.pm_aug_resized_crop_ragged_u8(a["src"], a["off"], a["hw"], *tail)
        return lib.pm_aug_resized_crop_u8(a["src"], *tail)
    for ragged in (False, True):
        assert crop(ragged, src=None) == E and crop(ragged, box=None) == E and crop(ragged, dst=None) == E and crop(ragged, ws=None) == E
        assert crop(ragged, wsb=need - 1) == E                    # short workspace
        assert crop(ragged, ws=p(ws) + 4) == E                    # not 16-byte aligned
        assert crop(ragged, B=65536) == S                         # the sample is blockIdx.y
        assert crop(ragged, out=0) == S and crop(ragged, B=0) == S and crop(ragged, Hs=0) == S and crop(ragged, Ws=0) == S
        assert crop(ragged) == 0
    assert crop(True, off=None) == E and crop(True, hw=None) == E
    assert lib.pm_aug_resized_crop_workspace_bytes(0, H, W, O) == 0 and lib.pm_aug_resized_crop_workspace_bytes(1, H, W, 0) == 0
    torch.cuda.synchronize()


# ---- 5. flat-grid wrap, one test per kernel family --------------------------------------------------------------------------------------------
def _wrap_frames(seed):
    H, W = C.WRAP_HW
    assert 3 * H * W > 8192 * 256
    return C.noise((3, H, W, 3), seed)


def test_gaussian_blur_grid_wraps():
    from oracle import augment_ref as R
    x = _wrap_frames(1)
    sigmas = (0.001, 2.0, 10.0)
    got = _blur(x, 25, sigmas)
    for b, sg in enumerate(sigmas):
        C.assert_same_bytes(got[b], R.gaussian_blur(x[b:b + 1], 25, sg)[0], f"sample {b} sigma {sg}")


def test_geometry_grid_wraps():
    from oracle.input_ref import to_tensor_normalize
    x = _wrap_frames(2)
    H, W = C.WRAP_HW
    geom = _geom_records(C.WRAP_ANGLES, H, W)
    want = np.stack([C.pil_flip_rotate(x[b], a, f) for b, (a, f) in enumerate(C.WRAP_ANGLES)])
    C.assert_same_bytes(_geometry(x, geom, False).numpy(), want, "u8")
    C.assert_same_bytes(C.f32_bits(_geometry(x, geom, True).numpy()),
                        C.f32_bits(to_tensor_normalize(torch.from_numpy(want), None, C.GEOM_MEAN, C.GEOM_STD).numpy()), "f32")


def test_pil_box_blur_grid_wraps():
    """The three-pass box blur against ImageFilter.GaussianBlur itself: one sample blurred mildly, one copied (radius < 0), one with a large
    sigma."""
    from ssl4polyp_amd.data import pil_box_blur_params
    L, lib = _lib()
    x = _wrap_frames(3)
    B, H, W, _ = x.shape
    prm = np.array([pil_box_blur_params(s, 3) if s is not None else (-1, 0, 0) for s in C.WRAP_BOX_SIGMAS], dtype=np.int64)
    assert prm[1, 0] < 0 and prm[2, 0] > prm[0, 0] >= 0
    prm_d = _dev((prm & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    tmp, out, xd = _filled(x.shape), _filled(x.shape), _dev(x)
    L.check(lib.pm_aug_pil_gaussian_blur_u8(xd.data_ptr(), tmp.data_ptr(), out.data_ptr(), prm_d.data_ptr(), 3, B, H, W, _st()), "box blur")
    got = out.cpu().numpy()
    for b, s in enumerate(C.WRAP_BOX_SIGMAS):
        C.assert_same_bytes(got[b], C.pil_gaussian_blur(x[b], s) if s is not None else x[b], f"sample {b} sigma {s}")


def test_resize_grid_wraps():
    """Three 700 x 900 frames to 1024 x 1024: both passes (3 x 700 x 1024 and 3 x 1024 x 1024 outputs) exceed the cap."""
    from ssl4polyp_amd.data import DeviceAugmenter
    Hs, Ws, S = C.WRAP_RESIZE
    x = C.noise((3, Hs, Ws, 3), 4)
    assert 3 * Hs * S > 8192 * 256
    aug = DeviceAugmenter(DEV, size=S)
    aug._scratch.exact("rs_tmp", (3, Hs, S, 3), torch.uint8).fill_(0xA5)
    aug._scratch.exact("rs_out", (3, S, S, 3), torch.uint8).fill_(0xA5)
    got = aug.resize(_dev(x)).cpu().numpy()
    for b in range(3):
        C.assert_same_bytes(got[b], C.pil_resize(x[b], S, S), f"frame {b}")
