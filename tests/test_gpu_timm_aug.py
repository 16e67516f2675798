"""timm's RandAugment and random erasing on the device (csrc/pm_timm_aug.hip, ssl4polyp_amd/timm_aug.py): every op of the policy
against Pillow's own call byte for byte, a mixed two-layer batch behind the flip, DeviceAugmenter.timm_tail, the erasing kernel
(exact outside the boxes, the Philox words with ==, the normals within a derived element-wise bound of a float64 Box-Muller,
statistics at a fixed key), and main_finetune_mae.run(train_aug=...) end to end.  Outputs lie between guard bytes and the sources
are checked afterwards.  The yardstick is tests/randaug_ref.py (pil_apply: Pillow itself)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import randaug_ref as R
from ssl4polyp_amd import timm_aug as TA

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
MEAN = (0.485, 0.456, 0.406)
TINY = dict(embed_dim=64, depth=2, num_heads=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_hold(buf, fill, what):
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), what + ": written outside the buffer"


def _layer(frames: np.ndarray, records, hflip=None):
    """One pm_randaug_stats + pm_randaug_apply over frames uint8 [B, H, W, 3] with one record per sample -> uint8 [B, H, W, 3] (numpy);
    the output lies between guard bytes, the source must come back unmodified."""
    from ssl4polyp_amd import _lib
    lib = _lib.load()
    B, H, W, _ = frames.shape
    plan = np.stack(records).reshape(B).astype(TA.OP_DTYPE)
    src = torch.from_numpy(frames).to(DEV)
    keep = src.clone()
    plan_d = torch.from_numpy(plan.view(np.uint8).reshape(B, 64).copy()).to(DEV)
    flip_d = torch.from_numpy(np.asarray(hflip, dtype=np.uint8)).to(DEV) if hflip is not None else None
    ws = _lib.workspace_bytes("pm_randaug_workspace", B)
    sbuf, stats = _guarded((ws // 8,), torch.int64, 0x55)
    stats.fill_(-1)   # (stale values: nothing may depend on what the workspace held)
    obuf, out = _guarded((B, H, W, 3), torch.uint8, 0xA5)
    out.fill_(0x3C)
    need = bool(np.isin(plan["op"], TA.STATS_OPS).any())
    if need:
        _lib.check(lib.pm_randaug_stats(src.data_ptr(), plan_d.data_ptr(), 1, stats.data_ptr(), ws, B, H, W, _stream()), "stats")
    _lib.check(lib.pm_randaug_apply(src.data_ptr(), out.data_ptr(), plan_d.data_ptr(), 1, flip_d.data_ptr() if flip_d is not None else None,
                                    stats.data_ptr() if need else None, ws if need else 0, B, H, W, *R.FILL, _stream()), "apply")
    torch.cuda.synchronize()
    _guards_hold(obuf, 0xA5, "pm_randaug_apply")
    _guards_hold(sbuf, 0x55, "pm_randaug_stats")
    assert torch.equal(src, keep), "the source was modified"
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ every op alone
OP_ARGS = {}
for _name, _arg in R.op_cases(48, 32):
    OP_ARGS.setdefault(_name, []).append(_arg)


@functools.lru_cache(maxsize=None)
def _small_frames():
    fr = R.frames(32, 48)
    extra = np.random.RandomState(7).randint(0, 256, (32, 48, 3)).astype(np.uint8)
    return [fr["random"], fr["constant"], fr["two_level"], fr["ramp"], fr["outlier"], extra]


@pytest.mark.parametrize("name", sorted(OP_ARGS))
def test_every_op_alone_equals_pillow(name):
    """B = 6 frames of 32 x 48 (not square: a 90 degree rotation goes through the bicubic transform), every sample another argument
    of the op's table and another kind of frame; an op with more than six arguments takes a second batch, one with fewer repeats
    them on other frames."""
    frames = _small_frames()
    args = OP_ARGS[name]
    for first in range(0, max(len(args), 1), 6):
        batch = [args[(first + i) % len(args)] for i in range(6)]
        order = [(i + first // 6) % 6 for i in range(6)]
        src = np.stack([frames[j] for j in order])
        got = _layer(src, [TA.op_record(name, a, 48, 32) for a in batch])
        assert got.shape == src.shape
        for i, a in enumerate(batch):
            want = R.pil_apply(src[i], name, a)
            assert torch.equal(torch.from_numpy(got[i]), torch.from_numpy(want)), \
                f"{name}({a}) on frame {order[i]}: {(got[i] != want).sum()} bytes differ"


def test_flip_is_applied_before_the_op():
    frames = _small_frames()
    steps = [("ShearX", 0.27), ("Sharpness", 1.81), ("Rotate", 180), ("Equalize", None), ("Identity", None), ("Rotate", -27)]
    flips = [1, 1, 1, 1, 1, 0]
    got = _layer(np.stack(frames), [TA.op_record(n, a, 48, 32) for n, a in steps], hflip=flips)
    for i, (n, a) in enumerate(steps):
        assert np.array_equal(got[i], R.pil_sequence(frames[i], [(n, a)], hflip=bool(flips[i]))), n


def test_refusals():
    from ssl4polyp_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    y = torch.zeros_like(x)
    plan = torch.zeros(2, 64, dtype=torch.uint8, device=DEV)
    st = _stream()
    assert lib.pm_randaug_apply(x.data_ptr(), x.data_ptr(), plan.data_ptr(), 1, None, None, 0, 2, 8, 8, 0, 0, 0, st) == _lib.PM_EINVAL
    assert lib.pm_randaug_apply(x.data_ptr(), y.data_ptr(), None, 1, None, None, 0, 2, 8, 8, 0, 0, 0, st) == _lib.PM_EINVAL
    assert lib.pm_randaug_apply(x.data_ptr(), y.data_ptr(), plan.data_ptr(), 0, None, None, 0, 2, 8, 8, 0, 0, 0, st) == _lib.PM_ESHAPE
    assert lib.pm_randaug_apply(x.data_ptr(), y.data_ptr(), plan.data_ptr(), 1, None, None, 0, 2, 8, 8, 256, 0, 0, st) == _lib.PM_EINVAL
    assert lib.pm_randaug_apply(x.data_ptr(), y.data_ptr(), plan.data_ptr(), 1, None, None, 0, 0, 8, 8, 0, 0, 0, st) == _lib.PM_ESHAPE
    ws = torch.zeros(2 * 776 * 4, dtype=torch.uint8, device=DEV)
    assert lib.pm_randaug_stats(x.data_ptr(), plan.data_ptr(), 1, ws.data_ptr(), ws.numel() - 1, 2, 8, 8, st) == _lib.PM_EINVAL
    assert lib.pm_randaug_stats(x.data_ptr(), plan.data_ptr(), 1, ws.data_ptr() + 4, ws.numel(), 2, 8, 8, st) == _lib.PM_EALIGN
    f = torch.zeros(2, 3, 8, 8, device=DEV)
    boxes = torch.zeros(2, 1, 4, dtype=torch.int32, device=DEV)
    assert lib.pm_random_erase_f32(f.data_ptr(), boxes.data_ptr(), 1, 4, 0, 0, 2, 3, 8, 8, st) == _lib.PM_EINVAL
    assert lib.pm_random_erase_f32(f.data_ptr(), boxes.data_ptr(), 0, 0, 0, 0, 2, 3, 8, 8, st) == _lib.PM_ESHAPE
    assert lib.pm_random_erase_f32(f.data_ptr(), None, 1, 0, 0, 0, 2, 3, 8, 8, st) == _lib.PM_EINVAL
    torch.cuda.synchronize()
    assert not y.any() and not f.any()


# ------------------------------------------------------------------------------------------------ mixed batch
M9 = [("AutoContrast", None), ("Equalize", None), ("Invert", None), ("Rotate", 27.0), ("PosterizeIncreasing", 1),
      ("SolarizeIncreasing", 26), ("SolarizeAdd", 99), ("ColorIncreasing", 1.81), ("ContrastIncreasing", 0.19),
      ("BrightnessIncreasing", 1.81), ("SharpnessIncreasing", 1.81), ("ShearX", -0.27), ("ShearY", 0.27), ("TranslateXRel", 0.405),
      ("TranslateYRel", -0.405)]


def _picture(rng, h, w):
    """a smooth colour field with texture and a bright blob: every op has something to act on"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([90 + 70 * np.sin(xx / 23.0 + rng.uniform(0, 6)), 110 + 60 * np.cos(yy / 17.0 + rng.uniform(0, 6)),
                     70 + 50 * np.sin((xx + yy) / 31.0)], axis=-1)
    base += rng.normal(0, 9, base.shape)
    base[h // 3:h // 3 + 20, w // 2:w // 2 + 30] += 90
    return np.clip(base, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _mixed():
    """16 frames of 224 x 224, two layers each: all fifteen ops in both layers, skipped layers, flips; and Pillow's result."""
    rng = np.random.RandomState(21)
    B, S = 16, 224
    frames = np.stack([_picture(rng, S, S) for _ in range(B)])
    steps = []
    for i in range(B):
        first = M9[i % 15] if i != 5 else ("Identity", None)                 # (sample 5: the first layer skipped)
        second = M9[(7 * i + 3) % 15] if i % 4 != 2 else ("Identity", None)   # (samples 2, 6, 10, 14: the second layer skipped)
        steps.append([first, second])
    steps[15] = [M9[5], M9[0]]                                                # (Solarize was skipped by sample 5)
    flips = np.array([i % 3 == 0 for i in range(B)], dtype=np.uint8)
    assert {n for s in steps for n, _ in s} >= {n for n, _ in M9}
    plan = np.zeros((B, 2), dtype=TA.OP_DTYPE)
    for i in range(B):
        for l in range(2):
            plan[i, l] = TA.op_record(steps[i][l][0], steps[i][l][1], S, S)
    want = np.stack([R.pil_sequence(frames[i], steps[i], hflip=bool(flips[i])) for i in range(B)])
    return frames, plan, flips, want


def test_mixed_batch_two_layers_behind_the_flip():
    frames, plan, flips, want = _mixed()
    ra = TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN)
    x = torch.from_numpy(frames).to(DEV)
    keep = x.clone()
    a = ra.apply(x, plan, hflip=flips).clone()
    b = ra.apply(x, plan, hflip=flips).clone()
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and torch.equal(a, b)
    got = a.cpu().numpy()
    for i in range(len(frames)):
        assert np.array_equal(got[i], want[i]), f"sample {i}: {(got[i] != want[i]).sum()} bytes differ from the Pillow sequence"
    assert not np.array_equal(got, frames)


def test_timm_tail_without_erasing_is_preprocess_of_the_pillow_frames():
    from ssl4polyp_amd.data import DeviceAugmenter, preprocess_u8
    frames, plan, flips, want = _mixed()
    aug = DeviceAugmenter(torch.device(DEV, 0), size=224)
    x = torch.from_numpy(frames).to(DEV)
    got = aug.timm_tail(x, TA.TrainAugment(TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN), None), plan=plan, hflip=flips)
    assert got.shape == (16, 3, 224, 224) and got.dtype == torch.float32
    assert torch.equal(got, preprocess_u8(torch.from_numpy(want).to(DEV)))
    # no policy, no erasing: mae_tail, draw for draw
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert torch.equal(aug.timm_tail(x, TA.TrainAugment(), generator=g1).clone(), aug.mae_tail(x, generator=g2))
    assert torch.equal(torch.rand(3, generator=g1), torch.rand(3, generator=g2))
    # drawn plans: the device result is the numpy restatement's (and so Pillow's) for whatever the generator draws
    ta = TA.TrainAugment(TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN), None)
    ta.reseed(1, 0)
    small = x[:4]
    out = aug.timm_tail(small, ta, hflip=np.zeros(4, np.uint8))
    ta.reseed(1, 0)
    plan4 = ta.rand_augment.draw(4, ta.rng, 224)
    ref = np.stack([R.np_sequence(frames[i], list(plan4[i])) for i in range(4)])
    assert torch.equal(out, preprocess_u8(torch.from_numpy(ref).to(DEV)))


# ------------------------------------------------------------------------------------------------ erasing
SEED, COUNTER = R.ERASE_SEED, R.ERASE_COUNTER
EB, EC, EH, EW = 4, 3, 40, 56
# sample 0: no box; 1: one box; 2: two overlapping boxes (the later one holds where they overlap); 3: a box in the bottom right
# corner, and one that leaves the frame (skipped)
EBOXES = np.array([[[0, 0, 0, 0], [0, 0, 0, 0]], [[5, 7, 13, 22], [0, 0, 0, 0]], [[3, 4, 20, 30], [10, 20, 25, 17]],
                   [[31, 45, 9, 11], [35, 50, 9, 11]]], dtype=np.int32)


def _erase(mode, boxes=EBOXES, shape=(EB, EC, EH, EW), seed=SEED, counter=COUNTER):
    from ssl4polyp_amd import _lib
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    buf, x = _guarded(shape, torch.float32, 12345.0)
    x.copy_(x0)
    bd = torch.from_numpy(np.ascontiguousarray(boxes)).to(DEV)
    _lib.check(_lib.load().pm_random_erase_f32(x.data_ptr(), bd.data_ptr(), boxes.shape[1], mode, seed, counter, *shape, _stream()),
               "pm_random_erase_f32")
    torch.cuda.synchronize()
    _guards_hold(buf, 12345.0, "pm_random_erase_f32")
    return x0.cpu().numpy(), x.cpu().numpy()


def _owner(boxes, shape):
    """int [B, H, W]: the index of the box whose value an element holds (the last valid box that covers it), -1 outside."""
    B, _, H, W = shape
    own = np.full((B, H, W), -1, dtype=np.int64)
    for b in range(B):
        for k, (top, left, h, w) in enumerate(boxes[b]):
            if h > 0 and w > 0 and top >= 0 and left >= 0 and top + h <= H and left + w <= W:
                own[b, top:top + h, left:left + w] = k
    return own


def _expected(boxes, shape, mode, fn):
    """float64 [B, C, H, W] of fn(sid, n) -> n values per stream laid out as the kernel lays them out, NaN outside the boxes."""
    B, C, H, W = shape
    own = _owner(boxes, shape)
    out = np.full(shape, np.nan)
    for b in range(B):
        for k, (top, left, h, w) in enumerate(boxes[b]):
            inside = own[b] == k
            if not inside.any():
                continue
            sid = b * boxes.shape[1] + k
            vals = fn(sid, C * h * w).reshape(C, h, w) if mode != 1 else np.broadcast_to(fn(sid, C)[:, None, None], (C, h, w))
            full = np.full((C, H, W), np.nan)
            full[:, top:top + h, left:left + w] = vals
            out[b][:, inside] = full[:, inside]
    return out


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["const", "rand", "pixel", "uniforms"])
def test_erasing_exact_parts(mode):
    shape = (EB, EC, EH, EW)
    x0, x = _erase(mode)
    own = _owner(EBOXES, shape)
    inside = np.broadcast_to((own >= 0)[:, None], shape)
    assert (own[0] < 0).all() and (own[3] == 1).sum() == 0 and (own[2] == 0).any() and (own[2] == 1).sum() == 25 * 17
    assert np.array_equal(x[~inside].view(np.uint32), x0[~inside].view(np.uint32)), "a byte outside the boxes changed"
    if mode == 0:
        assert not x[inside].any() and not np.signbit(x[inside]).any()
        return
    assert np.isfinite(x[inside]).all() and not np.array_equal(x[inside], x0[inside])
    if mode == 1:   # one value per channel and box
        for b in range(EB):
            for k in range(EBOXES.shape[1]):
                for c in range(EC):
                    v = x[b, c][own[b] == k]
                    assert v.size == 0 or (v == v[0]).all()
        ref = _expected(EBOXES, shape, 1, lambda sid, n: R.erase_normals64(SEED, COUNTER, sid, n)[0])
        rad = _expected(EBOXES, shape, 1, lambda sid, n: R.erase_normals64(SEED, COUNTER, sid, n)[1])
        assert (np.abs(x[inside] - ref[inside]) <= normal_bound(ref[inside], rad[inside])).all()
    if mode == 3:   # the words themselves: u1 of the pair for an even element, u2 for an odd one, exact 24-bit values
        def uniforms(sid, n):
            w = R.erase_words(SEED, COUNTER, sid, n)
            u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
            u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
            return np.where(np.arange(n) & 1, u2, u1)
        ref = _expected(EBOXES, shape, 3, uniforms)
        assert np.array_equal(x[inside].astype(np.float64), ref[inside]), "the Philox words are not the host restatement's"
    # the same key gives the same bits
    assert np.array_equal(_erase(mode)[1].view(np.uint32), x.view(np.uint32))


def normal_bound(z64, rad64):
    """|device normal - float64 Box-Muller of the same words|, from the rounding points of the device's f32 chain (ulp = 2^-23 of the
    value at most; the uniforms are exact 24-bit values):
      angle = fl(fl(2 pi) u2):   fl(2 pi) is off by 2.8e-8 < 2^-25 relative, the product by 2^-24  ->  <= 2 pi * 1.5 * 2^-24 absolute
      sincosf:                   <= 4 ulp of a value <= 1 (the OpenCL bound the device library documents)  ->  4 * 2^-23
      logf: <= 3 ulp; the factor -2 is exact; sqrtf halves the relative error and adds <= 3 ulp of its own  ->  4.5 ulp on the radius
      the last product:          0.5 ulp
    so |dz| <= radius * (2 pi * 1.5 * 2^-24 + 4 * 2^-23) + |z| * 5 * 2^-23, plus 1 % for the second-order terms."""
    return 1.01 * (rad64 * (2 * math.pi * 1.5 * 2.0 ** -24 + 4 * 2.0 ** -23) + np.abs(z64) * 5 * 2.0 ** -23) + 1e-12


def test_erasing_normals_within_the_derived_bound():
    shape = (2, 3, 70, 70)
    boxes = np.array([[[0, 0, 64, 64]], [[3, 5, 33, 47]]], dtype=np.int32)
    _, x = _erase(2, boxes, shape)
    worst = 0.0
    for b in range(2):
        top, left, h, w = boxes[b, 0]
        z, rad = R.erase_normals64(SEED, COUNTER, b, 3 * h * w)
        got = x[b, :, top:top + h, left:left + w].reshape(-1).astype(np.float64)
        ratio = np.abs(got - z) / normal_bound(z, rad)
        worst = max(worst, float(ratio.max()))
    print(f"erasing normals: largest |device - float64| / bound = {worst:.3f}")
    assert worst <= 1.0   # largest observed ratio on the MI355X: 0.377


def test_erasing_statistics_and_keys():
    """A fixed-key box of 3 x 64 x 64: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n) -- deterministic for this key, and
    tests/test_randaug_cpu.py checks that the float64 reference alone passes them.  Another sample index gives other values."""
    shape = (2, 3, 64, 64)
    boxes = np.array([[[0, 0, 64, 64]], [[0, 0, 64, 64]]], dtype=np.int32)
    _, x = _erase(2, boxes, shape)
    n = 3 * 64 * 64
    z = x[0].reshape(-1).astype(np.float64)
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    assert not np.array_equal(x[0], x[1]) and abs(np.corrcoef(z, x[1].reshape(-1))[0, 1]) < 5 / math.sqrt(n)
    _, again = _erase(2, boxes, shape)
    assert np.array_equal(again.view(np.uint32), x.view(np.uint32))
    _, other = _erase(2, boxes, shape, counter=COUNTER + 1)
    assert not np.array_equal(other[0], x[0])


def test_a_batch_without_boxes_launches_nothing(monkeypatch):
    from ssl4polyp_amd import _lib
    re = TA.RandomErasing(0.25)
    x = torch.randn(3, 3, 16, 16, device=DEV)
    keep = x.clone()

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_launch)
    assert re.apply(x, np.zeros((3, 1, 4), np.int32), (1, 2)) is x
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


def test_random_erasing_class_draws_and_erases():
    re = TA.RandomErasing(1.0, mode="const", min_count=2)
    rng = np.random.RandomState(4)
    boxes = re.draw(5, (3, 48, 64), rng)
    assert boxes.shape == (5, 2, 4) and (boxes[..., 2] > 0).all()
    x = torch.randn(5, 3, 48, 64, device=DEV)
    keep = x.clone()
    re.apply(x, boxes, (3, 0))
    own = torch.from_numpy(_owner(boxes, (5, 3, 48, 64)) >= 0).to(DEV)[:, None].expand(5, 3, 48, 64)
    assert not x[own].any() and torch.equal(x[~own], keep[~own])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """DATA/train: two classes of four JPEGs of mixed sizes; DATA/val: two classes of two."""
    from PIL import Image
    root = tmp_path_factory.mktemp("timm_aug_data")
    rng = np.random.RandomState(31)
    for split, n in (("train", 4), ("val", 2)):
        for c in range(2):
            d = root / split / f"class{c}"
            os.makedirs(d)
            for i in range(n):
                h, w = int(rng.randint(240, 300)), int(rng.randint(240, 300))
                pic = _picture(rng, h, w)
                pic[..., c] //= 2
                Image.fromarray(pic).save(str(d / f"{i}.jpg"), quality=90, subsampling=2 * (i % 2))
    return root


def _train_aug():
    return TA.TrainAugment(TA.RandAugment("rand-m9-mstd0.5-inc1", MEAN), TA.RandomErasing(0.25))


def test_main_finetune_mae_with_train_aug_end_to_end(folder, tmp_path, monkeypatch):
    from ssl4polyp_amd import data, main_finetune_mae, models_vit
    from ssl4polyp_amd.folder import folder_loader
    monkeypatch.setattr(models_vit, "vit_test_patch16", functools.partial(models_vit.VisionTransformer, **TINY), raising=False)
    first_batches, seen = [], set()
    real_epoch = main_finetune_mae.finetune_one_epoch

    def spying_epoch(model, loader, opt, device, epoch, args, prepare=None, **kw):
        def spy(batch):
            out = prepare(batch)
            if (id(model), epoch) not in seen:   # the first batch of every epoch of every run
                seen.add((id(model), epoch))
                first_batches.append((epoch, out[0].clone(), out[1].clone()))
            return out
        return real_epoch(model, loader, opt, device, epoch, args, prepare=spy, **kw)

    monkeypatch.setattr(main_finetune_mae, "finetune_one_epoch", spying_epoch)

    def args(out, **kw):
        a = main_finetune_mae.get_args_parser().parse_args(
            ["--model", "vit_test_patch16", "--batch_size", "4", "--epochs", "2", "--warmup_epochs", "1", "--nb_classes", "2",
             "--data_path", str(folder), "--output_dir", str(out), "--num_workers", "0", "--blr", "0.05", "--precision", "fp32",
             "--seed", "3", "--mixup", "0.8", "--cutmix", "1.0", "--smoothing", "0.1"])
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    model, _, hist = main_finetune_mae.run(args(tmp_path / "a"), train_aug=_train_aug())
    assert [h["epoch"] for h in hist] == [0, 1] and all(np.isfinite(h["train"]["loss"]) for h in hist)
    assert hist[0]["train"]["samples"] == 8 and hist[0]["test"]["samples"] == 4
    with_aug = first_batches[0][1]
    # resumed after epoch 0: the second epoch is the uninterrupted run's, bit for bit (plans, boxes and normals depend on (seed, epoch))
    first = tmp_path / "a" / "ckpts" / "checkpoint-0.pth"
    model_b, _, hist_b = main_finetune_mae.run(args(tmp_path / "b", resume=str(first)), train_aug=_train_aug())
    assert [h["epoch"] for h in hist_b] == [1] and hist_b[0]["train"]["loss"] == hist[1]["train"]["loss"]
    assert hist_b[0]["test"] == hist[1]["test"]
    for (k, a), b in zip(model.state_dict().items(), model_b.state_dict().values()):
        assert torch.equal(a, b), k
    assert [e for e, _, _ in first_batches] == [0, 1, 1]
    assert torch.equal(first_batches[1][1], first_batches[2][1]), "epoch 1's first batch differs after the resume"
    # without a TrainAugment the first training batch is the crop -> flip -> normalise of before
    first_batches.clear()
    main_finetune_mae.run(args(tmp_path / "c", epochs=1))
    plain, labels = first_batches[0][1], first_batches[0][2]
    dev = torch.device(DEV, 0)
    loader = folder_loader(os.path.join(str(folder), "train"), 4, 1, 0, 3, 0, True, decode="host")
    loader.sampler.set_epoch(3)
    frames, lab = next(iter(loader))
    frames = frames.to(dev)
    gen = torch.Generator().manual_seed(3)
    aug = data.DeviceAugmenter(dev, size=224)
    boxes = data.draw_linprobe_boxes(len(frames), frames.sizes[:, 0], frames.sizes[:, 1], gen)
    want = aug.mae_tail(aug.random_resized_crop(frames, boxes=boxes), generator=gen)
    assert torch.equal(plain, want) and torch.equal(labels.cpu(), lab)
    assert with_aug.shape == plain.shape and not torch.equal(with_aug, plain)
