"""The device validation transform of the MAE recipes, without a GPU: the numpy restatement the kernel follows
(tests/val_transform_ref.py) against Pillow itself with ==, five plausible mistakes that Pillow tells apart, and the plumbing -- the
C header, the ctypes signatures, the host window table, the flags of both parsers and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

import val_transform_ref as V
from ssl4polyp_amd.data import center_crop_windows   # (the host side of the device transform: this file is about it)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = V.SMALL + V.LARGE


@pytest.fixture(scope="module")
def pillow():
    """shape -> (noise frame, Pillow's Resize + CenterCrop of it), computed once."""
    out = {}
    for h, w, resize, crop in SHAPES:
        frame = V.noise_frame(h, w)
        out[(h, w, resize, crop)] = (frame, V.pillow_resize_center_crop(frame, resize, crop))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_pillow(pillow, shape):
    frame, want = pillow[shape]
    got = V.resize_center_crop(frame, shape[2], shape[3])
    assert got.shape == want.shape == (shape[3], shape[3], 3) and got.dtype == np.uint8
    assert (got == want).all()
    # the window the host uploads for this frame is the one the restatement evaluated
    assert tuple(center_crop_windows([shape[:2]], shape[2], shape[3])[0]) == V.window(*shape)


def test_val_frames_runs_the_same_pillow_sequence(tmp_path):
    """The authority of this file is what mae_recipe._ValFrames does with a decoded file (a PNG: lossless)."""
    from PIL import Image
    from ssl4polyp_amd.mae_recipe import _ValFrames
    os.makedirs(tmp_path / "c0")
    shapes = [(37, 53), (53, 37), (33, 32), (32, 32)]
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(V.noise_frame(h, w)).save(str(tmp_path / "c0" / f"{i}.png"))
    ds = _ValFrames(str(tmp_path), resize=32, crop=29)
    for i, (h, w) in enumerate(shapes):
        got, label = ds[i]
        assert label == 0 and (got == V.pillow_resize_center_crop(V.noise_frame(h, w), 32, 29)).all()


@pytest.mark.parametrize("variant", V.VARIANTS)
def test_wrong_variant_differs_from_pillow(pillow, variant):
    differs = [s for s in SHAPES if not np.array_equal(V.resize_center_crop(pillow[s][0], s[2], s[3], variant), pillow[s][1])]
    print(f"{variant}: differs on {len(differs)} of {len(SHAPES)} shapes")
    assert differs, f"{variant} equals Pillow on every shape: the shapes do not tell it apart"


def test_the_two_rounding_witnesses(pillow):
    """(33, 32) at resize 32, crop 28: the offset (33 - 28) / 2 = 2.5 rounds to 2 (half to even), not 3.  (53, 37) at resize 32: the
    long side 32 * 53 / 37 = 45.84 is truncated to 45, not rounded to 46."""
    assert V.window(33, 32, 32, 28)[2] == 2 and V.window(33, 32, 32, 28, "offset_half_up")[2] == 3
    assert V.window(53, 37, 32, 28)[0] == 45 and V.window(53, 37, 32, 28, "round_long_side")[0] == 46
    frame = V.noise_frame(33, 32)
    want = V.pillow_resize_center_crop(frame, 32, 28)
    assert (V.resize_center_crop(frame, 32, 28) == want).all()
    assert not np.array_equal(V.resize_center_crop(frame, 32, 28, "offset_half_up"), want)
    frame, want = pillow[(53, 37, 32, 28)]
    assert not np.array_equal(V.resize_center_crop(frame, 32, 28, "round_long_side"), want)


def test_host_window_table_is_the_reference_arithmetic():
    for resize, crop in ((32, 27), (32, 28), (32, 29), (32, 32), (256, 224)):
        hw = np.array([(h, w) for h, w, _, _ in SHAPES] + [(1, 5), (5, 1), (500, 375), (256, 256)])
        got = center_crop_windows(hw, resize, crop)
        assert got.dtype == np.int32 and got.shape == (len(hw), 4)
        for row, (h, w) in zip(got, hw):
            assert tuple(row) == V.window(int(h), int(w), resize, crop)
            nh, nw, top, left = (int(v) for v in row)
            assert min(nh, nw) >= resize and 0 <= top <= nh - crop and 0 <= left <= nw - crop
    assert tuple(center_crop_windows([(33, 32)], 32, 28)[0]) == (33, 32, 2, 2)
    assert tuple(center_crop_windows([(53, 37)], 32, 28)[0]) == (45, 32, 8, 2)


def test_crop_larger_than_resize_raises():
    with pytest.raises(ValueError):
        center_crop_windows([(40, 40)], 32, 33)
    with pytest.raises(ValueError):
        center_crop_windows([(40, 40)], 32, 0)


def test_header_and_signatures_declare_both_symbols():
    from ssl4polyp_amd import _lib
    with open(os.path.join(REPO, "include", "polypmae.h")) as f:
        header = f.read()
    for name, n_args in (("pm_aug_resize_center_crop_workspace", 6), ("pm_aug_resize_center_crop_ragged_u8", 13)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name + " is not declared in include/polypmae.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name])
    assert _lib.ABI_VERSION == 16
    with open(os.path.join(REPO, "ssl4polyp_amd", "csrc", "pm_augment.hip")) as f:
        src = f.read()
    assert 'extern "C" int pm_aug_resize_center_crop_ragged_u8(' in src and 'extern "C" int pm_aug_resize_center_crop_workspace(' in src


def test_both_parsers_take_the_flags():
    from ssl4polyp_amd import main_finetune_mae, main_linprobe
    for mod in (main_linprobe, main_finetune_mae):
        p = mod.get_args_parser()
        a = p.parse_args([])
        assert a.decode == "host" and a.val_transform == "host"
        a = p.parse_args(["--decode", "device", "--val_transform", "device"])
        assert a.decode == "device" and a.val_transform == "device"
        with pytest.raises(SystemExit):
            p.parse_args(["--val_transform", "gpu"])


def test_prefetcher_refusals():
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher
    aug = DeviceAugmenter("cuda", size=224)   # (no device is touched before the first batch)
    with pytest.raises(ValueError, match="fused_decode"):
        DevicePrefetcher([], "cuda", augment=aug, transform="mae_eval", fused_decode=True)
    with pytest.raises(ValueError, match="DeviceAugmenter"):
        DevicePrefetcher([], "cuda", transform="mae_eval")
    assert DevicePrefetcher([], "cuda", augment=aug, transform="mae_eval").transform == "mae_eval"
