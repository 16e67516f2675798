"""oracle/augment_ref.py -- the judge of tests/test_gpu_augment.py -- against LIVE Pillow at the edges tests/test_gpu_augment_edges.py
holds the kernels to (the case tables are tests/augment_cases.py): the colour ops over all 2^24 colours, every blend at the twentieths,
every contrast degenerate value, every op order, the rotations on non-square and one-pixel frames, the resizes from one pixel and
with many taps, the strip crops; the host tap builder against the oracle's; and the one place where the order of Image.resize's two
passes is not "horizontal first".  Bytes only: no tolerance.  No GPU."""
import numpy as np
import pytest

import augment_cases as C
from oracle import augment_ref as R

_cache = {}


def colours():
    if "c" not in _cache:
        _cache["c"] = C.all_colours()
    return _cache["c"]


def _chunks(a, n=8):
    step = a.shape[0] // n
    return [a[i:i + step] for i in range(0, a.shape[0], step)]


def test_hsv_conversions_over_every_colour():
    """rgb_to_hsv of all 2^24 colours equals convert("HSV"); hsv_to_rgb of all 2^24 (H, S, V) triples -- a superset of what any hue
    shift can produce from a colour -- equals Pillow's way back; then adjust_hue as a whole, factor in, at every shift of C.HUE
    (shift 0: the pure round trip, which is not the identity) on a slice holding every (G, B) pair under 16 values of R."""
    from PIL import Image
    a = colours()
    C.assert_same_bytes(np.concatenate([R.rgb_to_hsv(c) for c in _chunks(a)]), C.pil_hsv(a), "rgb_to_hsv")
    want = np.asarray(Image.fromarray(a, "HSV").convert("RGB"))   # the same array read as (H, S, V)
    C.assert_same_bytes(np.concatenate([R.hsv_to_rgb(c) for c in _chunks(a)]), want, "hsv_to_rgb")
    part = a[::256]
    assert not np.array_equal(C.pil_hue(part, 0), part)
    for factor, shift in C.HUE:
        assert C.hue_shift_of(factor) == shift
        C.assert_same_bytes(R.adjust_hue(part[None], factor)[0], C.pil_hue(part, shift), f"adjust_hue({factor})")


@pytest.mark.parametrize("f", C.SATURATION)
def test_saturation_over_every_colour(f):
    """adjust_saturation against ImageEnhance.Color over all 2^24 colours: interpolating, extrapolating, both ends."""
    a = colours()
    C.assert_same_bytes(np.concatenate([R.adjust_saturation(c[None], f)[0] for c in _chunks(a)]), C.pil_saturation(a, f), f"saturation {f}")


def test_brightness_at_the_twentieths():
    a = C.brightness_frame()
    assert all(len(np.unique(a[..., c])) == 256 for c in range(3))
    for f in C.TWENTIETHS:
        C.assert_same_bytes(R.adjust_brightness(a[None], f)[0], C.pil_brightness(a, f), f"brightness {f}")


def test_contrast_at_every_degenerate_value_and_twentieth():
    """The contrast frames cover what they claim (by Pillow's own ImageStat), and adjust_contrast equals ImageEnhance.Contrast on each
    of them at k / 20, k = 0 ... 40."""
    frames = C.contrast_frames()
    means, full = C.contrast_coverage(frames)
    assert means == set(range(256)) and len(full) >= 192
    for f in C.TWENTIETHS:
        got = R.adjust_contrast(frames, f)
        for b in range(0, len(frames), 3 if f not in (0.6, 1.4) else 1):   # every frame at two factors, a third of them at the others
            C.assert_same_bytes(got[b], C.pil_contrast(frames[b], f), f"contrast {f} frame {b}")


@pytest.mark.parametrize("H,W", C.ORDER_HW)
def test_every_op_order(H, W):
    B = len(C.PERMUTATIONS)
    x = C.noise((B, H, W, 3), 41 + H)
    fac = C.order_factors(B)
    orders = [C.PERMUTATIONS] + [(o,) * B for o in C.EXTRA_ORDERS]
    for order in orders:
        for b in range(B):
            args = (order[b],) + tuple(v[b] for v in fac)
            C.assert_same_bytes(C.oracle_jitter(R, x[b], *args), C.pil_jitter(x[b], *args), f"order {order[b]} sample {b}")
    C.assert_same_bytes(C.oracle_jitter(R, x[0], (-1,) * 4, *(v[0] for v in fac)), x[0], "all-skip is the identity")


@pytest.mark.parametrize("H,W", C.GEOM_HW)
def test_rotations_and_flips(H, W):
    """rotate_nearest against Image.rotate: non-square frames (90 and 270 degrees take the fixed-point path there), one-pixel lines."""
    from ssl4polyp_amd.data import _rotation_geom
    cases = C.geom_cases()
    x = C.noise((len(cases), H, W, 3), 7 * H + W)
    for b, (angle, flips) in enumerate(cases):
        C.assert_same_bytes(C.oracle_flip_rotate(R, x[b], angle, flips), C.pil_flip_rotate(x[b], angle, flips), f"{H}x{W} {angle} {flips}")
        mode = _rotation_geom(angle, W, H, flips)[0]
        assert mode in (0, 1, 2) or H == W, "the transpose fast paths are legal on square frames only"


@pytest.mark.parametrize("Hs,Ws,S", C.RESIZE)
def test_resize_edges(Hs, Ws, S):
    x = C.noise((Hs, Ws, 3), Hs + 3 * Ws)
    C.assert_same_bytes(R.resize_bilinear(x[None], S, S)[0], C.pil_resize(x, S, S), f"{Hs}x{Ws}->{S}")


def test_host_tap_builder_equals_the_oracles():
    from ssl4polyp_amd.data import _resample_coeffs
    for n_in, n_out in C.coeff_pairs():
        b, t, k = _resample_coeffs(n_in, n_out)
        rb, rt, rk = R._resample_coeffs(n_in, n_out)
        assert k == rk and np.array_equal(b, rb) and np.array_equal(t, rt), (n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k).all()


@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("out", C.CROP_OUT)
def test_crop_edges(out, filt):
    H, W = C.CROP_HW
    x = C.noise((H, W, 3), 77)
    for box in C.CROP_BOXES:
        C.assert_same_bytes(R.resized_crop(x[None], [box], out, out, filt)[0], C.pil_resized_crop(x, box, out, filt), f"{box}->{out} {filt}")
    for (h, w) in C.RAGGED_HW:
        f = C.noise((h, w, 3), h + w)
        C.assert_same_bytes(R.resize(f[None], out, out, filt)[0], C.pil_resize(f, out, out, filt), f"{h}x{w}->{out} {filt}")


def test_pil_box_blur_on_the_wrap_frame_and_on_lines():
    """pil_gaussian_blur (what the box-blur kernel is held to) against ImageFilter.GaussianBlur on 1 x N and N x 1 frames and at a
    large sigma."""
    for (h, w) in ((1, 40), (40, 1), (33, 47)):
        x = C.noise((h, w, 3), h * w)
        for sigma in (0.3, 1.5, 12.0):
            C.assert_same_bytes(R.pil_gaussian_blur(x, sigma), C.pil_gaussian_blur(x, sigma), f"{h}x{w} sigma {sigma}")


# ---- the order of Image.resize's two passes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_pass_order_edge(filt):
    """Each pass rounds to uint8, so the order of the passes is visible in the bytes.  Image.resize runs the horizontal pass first except
    for frames MORE than 100 times as tall as wide whose height shrinks (found by bisection on the CPU against Pillow 12.2, both filters,
    widths 2, 9 and 30, outputs 224 and 16: the last agreeing heights were 200, 900 and 3000; wide frames agree to 1 : 400 at least).
    Here: at the last shape on either side of that edge the oracle's order -- R.vertical_pass_first -- gives Pillow's bytes; where the
    label says "v" and both passes run, horizontal-first does not (that is what the device computes there: DESIGN.md)."""
    for (H, W, oh, ow), label in C.ORDER_EDGE:
        x = C.noise((H, W, 3), H + W)
        want = C.pil_resize(x, oh, ow, filt)
        assert R.vertical_pass_first(H, W, oh) == (label == "v"), (H, W, oh)
        C.assert_same_bytes(R.resize(x[None], oh, ow, filt)[0], want, f"{H}x{W}->{oh}x{ow} {filt}")
        C.assert_same_bytes(R.resize(x[None], oh, ow, filt, order=label)[0], want, f"{H}x{W}->{oh}x{ow} {filt} order {label}")
        if label == "v":
            assert not np.array_equal(R.resize(x[None], oh, ow, filt, order="h")[0], want), (H, W, "the order does not show here")
