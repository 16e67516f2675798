"""timm's RandAugment and random erasing, the part that needs no GPU: the numpy restatement of the device arithmetic
(tests/randaug_ref.py) against Pillow itself, byte for byte, with three wrong variants that must not pass; the protocol of
ssl4polyp_amd/timm_aug.py against values written out by hand; the C-ABI declarations; and that the recipe without a TrainAugment
makes the calls it made before."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import randaug_ref as R
from ssl4polyp_amd import timm_aug as TA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = (0.485, 0.456, 0.406)
SIZES = [(32, 48), (224, 224)]   # (h, w)
ERASE_SEED, ERASE_COUNTER = R.ERASE_SEED, R.ERASE_COUNTER   # the fixed key of tests/test_gpu_timm_aug.py
# Frames found by search (solve the cubic for an integer value, then try the neighbouring doubles of the root): in column 1 the
# bicubic value of a TranslateX by `shift` lies so close to an integer that the rounding of the single products decides the byte.
# A fused multiply-add lands on the other side.  (taps of columns 0..3, shift, Pillow's byte)
TIES = [((193, 183, 131, 91), float.fromhex("0x1.6ebadc7b706dcp-1"), 151), ((220, 251, 239, 146), float.fromhex("0x1.c5f8055d336acp-1"), 248)]


def _tie_frame(taps):
    f = np.full((4, 6, 3), 77, np.uint8)
    f[:, :4, :] = np.array(taps, np.uint8)[None, :, None]
    return f


# ------------------------------------------------------------------------------------------------ (b) numpy == Pillow
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_arithmetic_equals_pillow_byte_for_byte(hw):
    h, w = hw
    fr = R.frames(h, w)
    n = 0
    for name, arg in R.op_cases(w, h):
        rec = TA.op_record(name, arg, w, h)
        for fname, f in fr.items():
            want = R.pil_apply(f, name, arg)
            got = R.np_apply(f, rec)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), f"{name}({arg}) on the {fname} frame {h}x{w}: {(got != want).sum()} bytes differ"
            n += 1
    assert n == len(R.op_cases(w, h)) * 5


def test_what_pillow_does_at_the_ends_of_the_ranges():
    f = R.frames(32, 48)["random"]
    assert not R.pil_apply(f, "Posterize", 0).any()                              # posterize 0: black
    assert np.array_equal(R.pil_apply(f, "Solarize", 256), f)                    # threshold 256: nothing inverted
    assert np.array_equal(R.pil_apply(f, "Solarize", 0), 255 - f)
    assert np.array_equal(R.pil_apply(f, "Rotate", 0), f) and np.array_equal(R.pil_apply(f, "ShearX", 0), f)
    assert np.array_equal(R.pil_apply(f, "TranslateXRel", 0), f)
    const = R.frames(32, 48)["constant"]
    assert np.array_equal(R.pil_apply(const, "AutoContrast"), const) and np.array_equal(R.pil_apply(const, "Equalize"), const)
    assert tuple(R.pil_apply(R.frames(224, 224)["random"], "Rotate", 27)[0, 0]) == R.FILL   # the corner keeps the fill colour
    # the op records of those ends
    assert int(TA.op_record("Rotate", 0, 48, 32)["op"]) == TA.OP_IDENTITY
    assert (int(TA.op_record("Rotate", 180, 48, 32)["op"]), int(TA.op_record("Rotate", 180, 48, 32)["iarg"])) == (TA.OP_TRANSPOSE, 2)
    assert int(TA.op_record("Rotate", 90, 48, 32)["op"]) == TA.OP_AFFINE          # not square: Pillow goes through the transform
    assert (int(TA.op_record("Rotate", 90, 224, 224)["op"]), int(TA.op_record("Rotate", 90, 224, 224)["iarg"])) == (TA.OP_TRANSPOSE, 3)
    assert int(TA.op_record("Rotate", -90, 224, 224)["iarg"]) == 4
    assert int(TA.op_record("Posterize", 8, 48, 32)["op"]) == TA.OP_IDENTITY       # auto_augment.posterize returns the image


def test_wrong_variants_do_not_pass():
    """The comparison is sharp enough to see (1) a source coordinate without the + 0.5, (2) a fused multiply-add in the bicubic
    polynomial, (3) Equalize starting its running sum at 0 instead of step // 2."""
    h, w = 32, 48
    fr = R.frames(h, w)
    for name, arg in (("ShearX", 0.27), ("Rotate", 27), ("TranslateYRel", 0.405), ("TranslateXRel", 0.45)):
        rec = TA.op_record(name, arg, w, h)
        assert not np.array_equal(R.np_apply(fr["random"], rec, variant="no_half"), R.pil_apply(fr["random"], name, arg)), name
    rec = TA.op_record("Equalize", None, w, h)
    for fname in ("random", "ramp"):
        assert np.array_equal(R.np_apply(fr[fname], rec), R.pil_apply(fr[fname], "Equalize"))
        assert not np.array_equal(R.np_apply(fr[fname], rec, variant="equalize_no_half_step"), R.pil_apply(fr[fname], "Equalize")), fname
    for taps, shift, byte in TIES:
        f = _tie_frame(taps)
        rec = TA.op_record("TranslateX", shift, 6, 4)
        want = R.pil_apply(f, "TranslateX", shift)
        assert int(want[1, 1, 0]) == byte
        assert np.array_equal(R.np_apply(f, rec), want)
        fused = R.np_apply(f, rec, variant="fma")
        assert not np.array_equal(fused, want) and abs(int(fused[1, 1, 0]) - byte) == 1


def test_flip_comes_before_the_op():
    f = R.frames(32, 48)["random"]
    for name, arg in (("ShearX", 0.27), ("Sharpness", 1.81), ("Rotate", 180), ("Equalize", None)):
        rec = TA.op_record(name, arg, 48, 32)
        assert np.array_equal(R.np_apply(f, rec, hflip=True), R.pil_sequence(f, [(name, arg)], hflip=True)), name


# ------------------------------------------------------------------------------------------------ (c) the protocol
def test_parser_and_its_refusals():
    ra = TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN)
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.increasing, ra.prob) == (9, 2, 0.5, True, 0.5)
    assert ra.ops == TA.RAND_INCREASING_TRANSFORMS and len(ra.ops) == 15 and ra.fill == (124, 116, 104) == R.FILL
    plain = TA.RandAugment("rand-m7-n3", MEAN)
    assert (plain.magnitude, plain.num_layers, plain.magnitude_std, plain.increasing) == (7, 3, 0.0, False)
    assert plain.ops == TA.RAND_TRANSFORMS and "Posterize" in plain.ops and "PosterizeIncreasing" not in plain.ops
    assert [a for a, b in zip(TA.RAND_TRANSFORMS, TA.RAND_INCREASING_TRANSFORMS) if a != b] == \
        ["Posterize", "Solarize", "Color", "Contrast", "Brightness", "Sharpness"]
    for cfg, gap in (("rand-m9-w0", "weighted"), ("rand-m9-inc0", "inc0"), ("rand-m9-foo3", "foo"), ("rand-m9-mstd1e999", "uniform")):
        with pytest.raises(NotImplementedError, match=gap):
            TA.RandAugment(cfg, MEAN)
    assert TA.RandAugment("rand-m9-mstdinf", MEAN).magnitude_std == 0.0   # (no number in the section: timm skips it)
    with pytest.raises(NotImplementedError, match="AutoAugment"):
        TA.RandAugment("original-mstd0.5", MEAN)
    with pytest.raises(NotImplementedError, match="bicubic"):
        TA.RandAugment("rand-m9", MEAN, interpolation="bilinear")
    with pytest.raises(NotImplementedError, match="resplit"):
        TA.RandomErasing(0.25, num_splits=2)
    for cls in (TA.RandAugment, TA.RandomErasing):
        assert "NOT checked against timm itself" in " ".join(cls.__doc__.split())
    assert "has not been checked against timm itself" in " ".join(TA.__doc__.split())


def test_level_to_argument_at_m9_by_hand():
    L = TA.level_to_arg
    assert L("Rotate", 9.0) == 27.0 and L("Rotate", 9.0, True) == -27.0
    assert L("ShearX", 9.0) == 0.27 and L("ShearY", 9.0, True) == -0.27
    assert L("TranslateXRel", 9.0) == 0.405 and L("TranslateYRel", 9.0, True) == -0.405
    assert L("ColorIncreasing", 9.0) == 1.0 + 0.81 and L("SharpnessIncreasing", 9.0, True) == 1.0 - 0.81
    assert L("Contrast", 9.0) == 0.9 * 1.8 + 0.1 and L("Brightness", 0.0) == 0.1 and L("Color", 10.0) == 1.8 + 0.1
    assert L("PosterizeIncreasing", 9.0) == 1 and L("Posterize", 9.0) == 3 and L("PosterizeIncreasing", 0.0) == 4
    assert L("PosterizeIncreasing", 10.0) == 0
    assert L("SolarizeIncreasing", 9.0) == 26 and L("Solarize", 9.0) == 230 and L("SolarizeIncreasing", 0.0) == 256
    assert L("SolarizeAdd", 9.0) == 99 and L("SolarizeAdd", 10.0) == 110
    assert L("AutoContrast", 9.0) is None
    # ... and the records they become on a 224 x 224 frame
    assert TA.op_record("TranslateXRel", 0.405, 224, 224)["a"].tolist() == [1.0, 0.0, 0.405 * 224, 0.0, 1.0, 0.0]
    assert TA.op_record("TranslateYRel", -0.405, 224, 200)["a"].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, -0.405 * 200]
    assert TA.op_record("ShearX", 0.27, 224, 224)["a"].tolist() == [1.0, 0.27, 0.0, 0.0, 1.0, 0.0]
    assert TA.op_record("ShearY", -0.27, 224, 224)["a"].tolist() == [1.0, 0.0, 0.0, -0.27, 1.0, 0.0]
    assert float(TA.op_record("ContrastIncreasing", 1.81, 224, 224)["farg"]) == float(np.float32(1.81))
    rot = TA.op_record("Rotate", 27.0, 224, 224)["a"]
    c, s = round(math.cos(math.radians(27.0)), 15), round(math.sin(math.radians(27.0)), 15)
    assert rot[0] == c and rot[1] == -s and rot[3] == s and rot[4] == c
    assert rot[2] == c * -112.0 + -s * -112.0 + 0.0 + 112.0 and rot[5] == s * -112.0 + c * -112.0 + 0.0 + 112.0


class Script:
    """A generator that hands out scripted values and records who asked for what."""

    def __init__(self, values):
        self.values, self.calls = list(values), []

    def _next(self, call):
        self.calls.append(call)
        return self.values.pop(0)

    def random_sample(self):
        return self._next(("random_sample",))

    def uniform(self, lo, hi):
        return self._next(("uniform", lo, hi))

    def normal(self, loc, scale):
        return self._next(("normal", loc, scale))

    def randint(self, lo, hi, size=None):
        return self._next(("randint", lo, hi) if size is None else ("randint", lo, hi, size))


def test_randaugment_draw_order_clipping_and_skip():
    ra = TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN)
    rng = Script([np.array([3, 4]), 0.2, 9.0, 0.9, 0.7, 9.0, 0.1,        # sample 0: Rotate applied at 9, negated; layer 1 skipped
                  np.array([5, 11]), 0.5, 12.5, 0.3, 0.0, -2.0, 0.6])   # sample 1: Solarize at 12.5 -> 10; ShearX at -2 -> 0
    plan = ra.draw(2, rng, 224)
    assert plan.shape == (2, 2) and plan.dtype == TA.OP_DTYPE and not rng.values
    assert rng.calls[0] == ("randint", 0, 15, 2) and rng.calls[1:4] == [("random_sample",), ("normal", 9, 0.5), ("random_sample",)]
    assert len(rng.calls) == 14
    assert plan[0, 0] == TA.op_record("Rotate", -27.0, 224, 224)
    assert int(plan[0, 1]["op"]) == TA.OP_IDENTITY                      # random_sample() = 0.7 > 0.5: skipped
    assert plan[1, 0] == TA.op_record("SolarizeIncreasing", 0, 224, 224)   # magnitude clipped to 10: 256 - 256; 0.5 is not > 0.5
    assert (int(plan[1, 0]["op"]), int(plan[1, 0]["iarg"])) == (TA.OP_SOLARIZE, 0)
    assert plan[1, 1] == TA.op_record("ShearX", 0.0, 224, 224)          # magnitude clipped to 0 (the sign no longer matters)
    # a sign drawn for an op without one changes nothing
    rng = Script([np.array([6]), 0.0, 9.0, 0.99])
    assert TA.RandAugment("rand-m9-n1-mstd0.5", MEAN).draw(1, rng, 224)[0, 0] == TA.op_record("SolarizeAdd", 99, 224, 224)


def test_plans_are_a_function_of_seed_and_epoch():
    ra = TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN)
    aug = TA.TrainAugment(ra, TA.RandomErasing(0.25))
    aug.reseed(3, 1)
    a, ba = ra.draw(16, aug.rng), aug.random_erasing.draw(16, (3, 224, 224), aug.rng)
    keys = [aug.next_key(), aug.next_key()]
    aug.reseed(3, 1)
    b, bb = ra.draw(16, aug.rng), aug.random_erasing.draw(16, (3, 224, 224), aug.rng)
    assert a.tobytes() == b.tobytes() and np.array_equal(ba, bb) and keys == [(3, 1 << 32), (3, (1 << 32) | 1)]
    assert aug.next_key() == keys[0]
    aug.reseed(3, 2)
    c = ra.draw(16, aug.rng)
    assert a.tobytes() != c.tobytes() and aug.next_key() == (3, 2 << 32)
    ops = a["op"].reshape(-1)
    assert 0 < (ops == TA.OP_IDENTITY).sum() < ops.size          # the 0.5 skip happens, and not always
    assert set(np.unique(ops)) <= set(range(13))


def test_random_erasing_boxes_by_hand():
    la = math.log(0.3)
    re = TA.RandomErasing(0.25)
    assert (re.min_count, re.max_count, re.mode) == (1, 1, "pixel") and re.log_aspect_ratio == (la, math.log(1 / 0.3))
    # sample 0: 0.3 > 0.25, no box.  sample 1: area 0.1 * 224 * 224 = 5017.6, aspect e^0 = 1: h = w = round(70.83...) = 71
    rng = Script([0.3, 0.25, 0.1, 0.0, 10, 20])
    boxes = re.draw(2, (3, 224, 224), rng)
    assert boxes.dtype == np.int32 and boxes.tolist() == [[[0, 0, 0, 0]], [[10, 20, 71, 71]]] and not rng.values
    assert rng.calls == [("random_sample",), ("random_sample",), ("uniform", 0.02, 1 / 3), ("uniform", la, math.log(1 / 0.3)),
                         ("randint", 0, 154), ("randint", 0, 154)]
    # aspect: area 0.05 * 50176 = 2508.8, ratio e^0.5: h = round(sqrt(2508.8 * 1.6487...)) = 64, w = round(sqrt(2508.8 / 1.6487...)) = 39
    rng = Script([0.0, 0.05, 0.5, 1, 2])
    assert re.draw(1, (3, 224, 224), rng).tolist() == [[[1, 2, 64, 39]]]
    assert rng.calls[-2:] == [("randint", 0, 224 - 64 + 1), ("randint", 0, 224 - 39 + 1)]
    # ten attempts that do not fit (area 1/3 at aspect 1 / 0.3: h = round(sqrt(16725.3 * 3.33)) = 236 >= 224): no box, 21 draws
    rng = Script([0.0] + [1 / 3, math.log(1 / 0.3)] * 10)
    assert not re.draw(1, (3, 224, 224), rng).any() and len(rng.calls) == 21 and not rng.values
    # the ninth attempt fails, the tenth fits
    rng = Script([0.0] + [1 / 3, math.log(1 / 0.3)] * 9 + [0.1, 0.0, 5, 6])
    assert re.draw(1, (3, 224, 224), rng).tolist() == [[[5, 6, 71, 71]]]
    # count > 1: a count draw in [1, 3], every box's area divided by the count: 0.2 * 50176 / 2 = 5017.6 again
    re2 = TA.RandomErasing(1.0, mode="rand", min_count=1, max_count=3)
    rng = Script([0.9, 2, 0.2, 0.0, 3, 4, 0.2, 0.0, 100, 150])
    assert re2.draw(1, (3, 224, 224), rng).tolist() == [[[3, 4, 71, 71], [100, 150, 71, 71], [0, 0, 0, 0]]]
    assert rng.calls[1] == ("randint", 1, 4)
    with pytest.raises(ValueError):
        TA.RandomErasing(0.5, mode="noise")


def test_erase_reference_words_and_normals():
    """The float64 reference of the GPU erasing test passes its own statistical bounds at the key that test uses, and reads the
    words the header documents."""
    n = 3 * 64 * 64
    z, rad = R.erase_normals64(ERASE_SEED, ERASE_COUNTER, 0, n)
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    w = R.erase_words(ERASE_SEED, ERASE_COUNTER, 0, 8)
    assert (w[0] == w[1]).all() and (w[2] == w[3]).all() and not (w[0] == w[2]).all() and not (w[0] == w[4]).all()
    from oracle.noise_ref import philox4x32_10
    first = philox4x32_10([0, 0, ERASE_COUNTER & 0xFFFFFFFF, ERASE_COUNTER >> 32], [ERASE_SEED & 0xFFFFFFFF, ERASE_SEED >> 32])
    assert [int(w[0, 0]), int(w[0, 1]), int(w[2, 0]), int(w[2, 1])] == [int(v) for v in first]
    z1, _ = R.erase_normals64(ERASE_SEED, ERASE_COUNTER, 1, 64)
    assert not np.array_equal(z1, z[:64])


# ------------------------------------------------------------------------------------------------ declarations
def test_symbols_are_declared_in_the_header_and_the_binding():
    from ssl4polyp_amd import _lib
    import __graft_entry__ as g
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polypmae.h")).read(), flags=re.S)
    for name, nargs in (("pm_randaug_workspace", 2), ("pm_randaug_stats", 9), ("pm_randaug_apply", 14), ("pm_random_erase_f32", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared in include/polypmae.h"
        assert len(_lib.SIGNATURES[name]) == nargs
    assert "pm_timm_aug.hip" in g.SOURCES and g.SOURCE_FLAGS["pm_timm_aug.hip"] == ["-ffp-contract=off"]
    assert g.SOURCE_FLAGS["pm_augment.hip"] == ["-ffp-contract=off"] and _lib.ABI_VERSION == 16
    assert TA.OP_DTYPE.itemsize == 64 and TA.OP_DTYPE.fields["a"][1] == 16


def test_workspace_query_answers_without_a_gpu():
    import __graft_entry__ as g
    from ssl4polyp_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    assert _lib.workspace_bytes("pm_randaug_workspace", 64) == 64 * (768 * 4 + 8 + 24)
    with pytest.raises(_lib.PolypMaeError):
        _lib.workspace_bytes("pm_randaug_workspace", 0)


# ------------------------------------------------------------------------------------------------ (d) unchanged behaviour
def test_command_line_still_refuses_the_two_flags():
    from ssl4polyp_amd import main_finetune_mae
    parse = main_finetune_mae.get_args_parser().parse_args
    with pytest.raises(NotImplementedError, match="RandAugment"):
        main_finetune_mae.check_supported(parse(["--aa", "rand-m9-mstd0.5-inc1"]))
    with pytest.raises(NotImplementedError, match="random erasing"):
        main_finetune_mae.check_supported(parse(["--reprob", "0.25"]))
    main_finetune_mae.check_supported(parse([]))
    assert parse([]).aa is None and parse([]).reprob == 0.0 and parse([]).drop_path == 0.0
    assert "train_aug" in main_finetune_mae.run.__doc__ and "one later change" in main_finetune_mae.__doc__


class _Frames:
    def __init__(self, sizes):
        self.sizes = np.asarray(sizes, dtype=np.int64)

    def __len__(self):
        return len(self.sizes)

    def to(self, device, non_blocking=False):
        return self


def _spied_epochs(monkeypatch, train_aug):
    """run_epochs over two epochs of two batches with everything that needs a GPU replaced by recorders -> the call log."""
    from ssl4polyp_amd import data, folder, mae_recipe
    log = []
    real_boxes = data.draw_linprobe_boxes

    def boxes(B, h, w, gen):
        out = real_boxes(B, h, w, gen)
        log.append(("boxes", np.asarray(out).tolist()))
        return out

    class Aug:
        def __init__(self, device, size=224):
            pass

        def random_resized_crop(self, frames, boxes=None):
            return frames

        def mae_tail(self, x, hflip=None, generator=None, out=None):
            log.append(("mae_tail", torch.rand(len(x), generator=generator).tolist()))
            return "images"

        def timm_tail(self, x, aug, plan=None, boxes=None, hflip=None, generator=None, rng=None, out=None):
            log.append(("timm_tail", torch.rand(len(x), generator=generator).tolist(), aug.epoch, float(aug.rng.random_sample())))
            return "images"

    batches = [(_Frames([(300, 400), (256, 256), (500, 375)]), torch.tensor([0, 1, 0])), (_Frames([(280, 350)]), torch.tensor([1]))]
    loader = types.SimpleNamespace(sampler=types.SimpleNamespace(set_epoch=lambda e: log.append(("sampler", e))))
    monkeypatch.setattr(data, "draw_linprobe_boxes", boxes)
    monkeypatch.setattr(data, "DeviceAugmenter", Aug)
    monkeypatch.setattr(data, "DeviceJpegDecoder", lambda device: None)
    monkeypatch.setattr(folder, "folder_loader", lambda *a, **k: loader)
    monkeypatch.setattr(mae_recipe, "evaluate_probe", lambda *a: {"samples": 0, "acc1": 0.0})

    def train_epoch(epoch, ld, prepare):
        assert ld is loader
        for b in batches:
            images, labels = prepare(b)
            assert images == "images"
        return {"loss": 0.0}

    args = types.SimpleNamespace(resume="", eval=False, start_epoch=0, epochs=2, seed=3, output_dir="", data_path="x", batch_size=4,
                                 num_workers=0, pin_mem=False, decode="host", val_transform="host")
    kw = {} if train_aug is None else {"train_aug": train_aug}
    mae_recipe.run_epochs(args, None, None, torch.device("cpu"), train_epoch, crop_size=224, train_loader=None, val_loader=object(),
                          prepare_given=False, **kw)
    return log, batches


def test_recipe_without_train_aug_makes_the_calls_it_made(monkeypatch):
    from ssl4polyp_amd import data
    real_boxes = data.draw_linprobe_boxes
    log, batches = _spied_epochs(monkeypatch, None)
    want = []
    for epoch in (0, 1):
        g = torch.Generator().manual_seed(3 + epoch)      # the crop generator of epoch e: boxes, then flips, batch after batch
        want.append(("sampler", 3 + epoch))
        for frames, _ in batches:
            want.append(("boxes", np.asarray(real_boxes(len(frames), frames.sizes[:, 0], frames.sizes[:, 1], g)).tolist()))
            want.append(("mae_tail", torch.rand(len(frames), generator=g).tolist()))
    assert log == want
    # with a TrainAugment the torch generator sees the same sequence; the tail is timm_tail, reseeded from (seed, epoch)
    aug = TA.TrainAugment(TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN), TA.RandomErasing(0.25))
    log2, _ = _spied_epochs(monkeypatch, aug)
    assert [e[:2] for e in log2] == [("timm_tail", e[1]) if e[0] == "mae_tail" else e for e in want]
    tails = [e for e in log2 if e[0] == "timm_tail"]
    assert [e[2] for e in tails] == [0, 0, 1, 1]
    fresh = TA.TrainAugment()
    fresh.reseed(3, 1)
    assert tails[2][3] == float(fresh.rng.random_sample()) and tails[0][3] != tails[2][3]
