"""The validation transform of the MAE recipes on the device: pm_aug_resize_center_crop_ragged_u8 against Pillow itself with
torch.equal (Resize(resize, bicubic) + CenterCrop(crop) as mae_recipe._ValFrames runs it; tests/val_transform_ref.py holds the
Pillow sequence), outputs between guard bytes, the workspace past its queried size poisoned and checked, every refusal with the
output untouched; then what is built on it -- DeviceAugmenter.resize_center_crop, DevicePrefetcher(transform="mae_eval"),
mae_recipe.build_val_loader and the --decode / --val_transform flags of main_linprobe and main_finetune_mae, whose batches and
records must not depend on where the work runs.  No tolerance anywhere: every comparison is == or torch.equal."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import val_transform_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL, POISON = 256, 0x5A, 0xA5
TINY = dict(embed_dim=64, depth=2, num_heads=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


# ---------------------------------------------------------------------------------------------------- kernel
SMALL_HW = [(h, w) for h, w, _, _ in V.SMALL] + [(1, 5), (5, 1)]
LARGE_HW = [(375, 500), (500, 375), (256, 256), (100, 300), (257, 256), (1080, 1350)]


@functools.lru_cache(maxsize=None)
def _frames(hws):
    return tuple(V.noise_frame(h, w, seed=i) for i, (h, w) in enumerate(hws))


@functools.lru_cache(maxsize=None)
def _pillow(hws, resize, crop):
    """Pillow's Resize + CenterCrop of every frame of the batch, computed once per (batch, resize, crop): uint8 [B, crop, crop, 3]."""
    return torch.from_numpy(np.stack([V.pillow_resize_center_crop(f, resize, crop) for f in _frames(hws)]))


def _ragged(hws):
    from ssl4polyp_amd.data import RaggedFrames
    return RaggedFrames.from_frames(_frames(hws)).to(DEV)


def _query(B, Hmax, Wmax, resize, crop):
    from ssl4polyp_amd import _lib
    size = ctypes.c_size_t(0)
    st = _lib.load().pm_aug_resize_center_crop_workspace(B, Hmax, Wmax, resize, crop, ctypes.byref(size))
    return st, int(size.value)


def _call(rf, win, dst, B, Hmax, Wmax, resize, crop, ws, ws_bytes, null=None):
    """The C entry; `null` names one pointer argument to pass as NULL."""
    from ssl4polyp_amd import _lib
    ptr = {"src": rf.data.data_ptr(), "offset": rf.offset.data_ptr(), "hw": rf.hw.data_ptr(), "win": win.data_ptr(),
           "dst": dst.data_ptr(), "workspace": ws if isinstance(ws, int) else ws.data_ptr()}
    if null is not None:
        ptr[null] = None
    return _lib.load().pm_aug_resize_center_crop_ragged_u8(ptr["src"], ptr["offset"], ptr["hw"], ptr["win"], ptr["dst"], B, Hmax, Wmax,
                                                           resize, crop, ptr["workspace"], ws_bytes,
                                                           torch.cuda.current_stream().cuda_stream)


def _guarded_out(B, crop):
    buf = torch.full((B * crop * crop * 3 + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + B * crop * crop * 3].view(B, crop, crop, 3)


def _run_kernel(hws, resize, crop):
    """One call over the ragged batch of `hws` -> the output; the guards and the poisoned workspace tail are checked here."""
    from ssl4polyp_amd.data import center_crop_windows
    rf = _ragged(hws)
    B = len(hws)
    Hmax, Wmax = max(h for h, _ in hws), max(w for _, w in hws)
    st, need = _query(B, Hmax, Wmax, resize, crop)
    assert st == 0 and need > 0 and need % 16 == 0
    win = torch.from_numpy(center_crop_windows(rf.sizes, resize, crop)).to(DEV)
    buf, out = _guarded_out(B, crop)
    wsb = torch.full((GUARD + need + 4096,), POISON, dtype=torch.uint8, device=DEV)
    ws = wsb[GUARD:]
    assert ws.data_ptr() % 16 == 0
    assert _call(rf, win, out, B, Hmax, Wmax, resize, crop, ws, need) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all()), "written outside the output"
    assert bool((wsb[:GUARD] == POISON).all()), "written in front of the workspace"
    assert bool((ws[need:] == POISON).all()), "written past the queried workspace size"
    return out


@pytest.mark.parametrize("crop", [27, 28, 29, 32])
def test_small_batch_equals_pillow(crop):
    hws = tuple(SMALL_HW)
    got = _run_kernel(hws, 32, crop).cpu()
    want = _pillow(hws, 32, crop)
    for b, hw in enumerate(hws):
        assert torch.equal(got[b], want[b]), f"frame {hw} at resize 32, crop {crop}"


@pytest.mark.parametrize("hw,crop", [((37, 53), 28), ((300, 17), 28), ((7, 9), 32), ((1, 5), 27), ((5, 1), 32), ((33, 32), 28)])
def test_single_frame_equals_pillow(hw, crop):
    assert torch.equal(_run_kernel((hw,), 32, crop).cpu(), _pillow((hw,), 32, crop))


def test_large_batch_equals_pillow():
    hws = tuple(LARGE_HW)
    got = _run_kernel(hws, 256, 224).cpu()
    want = _pillow(hws, 256, 224)
    for b, hw in enumerate(hws):
        assert torch.equal(got[b], want[b]), f"frame {hw} at resize 256, crop 224"


def test_refusals_leave_the_output_untouched():
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.data import center_crop_windows
    hws = ((37, 53), (53, 37), (20, 70))
    rf = _ragged(hws)
    B, Hmax, Wmax, resize, crop = 3, 53, 70, 32, 28
    st, need = _query(B, Hmax, Wmax, resize, crop)
    assert st == 0
    win = torch.from_numpy(center_crop_windows(rf.sizes, resize, crop)).to(DEV)
    buf, out = _guarded_out(B, crop)
    out.fill_(7)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    good = dict(B=B, Hmax=Hmax, Wmax=Wmax, resize=resize, crop=crop)

    def call(ws_arg=ws, ws_bytes=need, null=None, **kw):
        a = {**good, **kw}
        return _call(rf, win, out, a["B"], a["Hmax"], a["Wmax"], a["resize"], a["crop"], ws_arg, ws_bytes, null)

    for name in ("src", "offset", "hw", "win", "dst", "workspace"):
        assert call(null=name) == _lib.PM_EINVAL, name
    assert call(ws_bytes=need - 1) == _lib.PM_EINVAL
    assert call(ws_bytes=0) == _lib.PM_EINVAL
    assert call(ws_arg=ws.data_ptr() + 4) == _lib.PM_EALIGN
    assert call(ws_arg=ws.data_ptr() + 1, ws_bytes=need) == _lib.PM_EALIGN
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(crop=0), dict(crop=-3), dict(crop=33), dict(resize=0), dict(resize=27),
               dict(Hmax=0), dict(Wmax=0), dict(Hmax=-5)):
        assert call(**kw) == _lib.PM_ESHAPE, kw
    # the workspace query refuses the same shapes, and a missing result pointer
    lib = _lib.load()
    size = ctypes.c_size_t(0)
    for a in ((0, 53, 70, 32, 28), (65536, 53, 70, 32, 28), (3, 0, 70, 32, 28), (3, 53, 0, 32, 28), (3, 53, 70, 0, 28), (3, 53, 70, 32, 0),
              (3, 53, 70, 32, 33)):
        assert lib.pm_aug_resize_center_crop_workspace(*a, ctypes.byref(size)) == _lib.PM_ESHAPE, a
    assert lib.pm_aug_resize_center_crop_workspace(3, 53, 70, 32, 28, None) == _lib.PM_EINVAL
    assert lib.pm_aug_resize_center_crop_workspace(65535, 53, 70, 32, 28, ctypes.byref(size)) == 0 and size.value > 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())
    # the same buffers with every argument in order: the call runs
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _pillow(hws, resize, crop))


def test_augmenter_method():
    """DeviceAugmenter.resize_center_crop: crop=None is the augmenter's size; a second, larger batch grows the scratch; crop > resize
    and a host batch are refused."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames
    aug = DeviceAugmenter(DEV, size=28)
    small = ((37, 53), (33, 32))
    assert torch.equal(aug.resize_center_crop(_ragged(small), resize=32).cpu(), _pillow(small, 32, 28))
    hws = tuple(SMALL_HW)
    assert torch.equal(aug.resize_center_crop(_ragged(hws), resize=32, crop=29).cpu(), _pillow(hws, 32, 29))
    assert torch.equal(aug.resize_center_crop(_ragged(small), resize=32).cpu(), _pillow(small, 32, 28))
    with pytest.raises(ValueError):
        aug.resize_center_crop(_ragged(small), resize=32, crop=33)
    with pytest.raises(_lib.PolypMaeError):
        aug.resize_center_crop(RaggedFrames.from_frames(_frames(small)), resize=32)
    with pytest.raises(TypeError):
        aug.resize_center_crop(torch.zeros(2, 40, 40, 3, dtype=torch.uint8, device=DEV), resize=32)


# ---------------------------------------------------------------------------------------------------- pipeline
MODES = [dict(val_transform="host", decode="host"), dict(val_transform="device", decode="host"),
         dict(val_transform="device", decode="device")]


def _picture(rng, h, w, c):
    """A smooth picture with some texture (so that JPEG keeps it recognisable), brighter for class 1."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 70 + 90 * c + 40 * np.sin(yy / 17.0)[..., None] + 30 * np.cos(xx / 23.0)[..., None] + rng.normal(0, 12, (h, w, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """DATA/val: two classes, thirteen files of mixed sizes -- baseline JPEGs in 4:4:4 and 4:2:0, and the device decoder's host
    fallbacks: a greyscale JPEG, a progressive JPEG, a PNG.  DATA/train: eight baseline JPEGs."""
    from PIL import Image
    root = tmp_path_factory.mktemp("val_transform_data")
    rng = np.random.default_rng(11)
    val = [(300, 400, dict(subsampling=0)), (400, 300, dict(subsampling=2)), (256, 256, dict(subsampling=0)),
           (257, 256, dict(subsampling=2)), (100, 300, dict(subsampling=2)), (375, 500, dict(subsampling=0)),
           (333, 517, dict(subsampling=2)), (301, 299, "L"), (280, 350, dict(progressive=True)), (290, 310, "png"),
           (256, 341, dict(subsampling=2)), (512, 256, dict(subsampling=0)), (270, 263, dict(subsampling=2))]
    for i, (h, w, kind) in enumerate(val):
        c = i % 2
        d = root / "val" / f"class{c}"
        os.makedirs(d, exist_ok=True)
        img = Image.fromarray(_picture(rng, h, w, c))
        if kind == "png":
            img.save(str(d / f"{i:02d}.png"))
        elif kind == "L":
            img.convert("L").save(str(d / f"{i:02d}.jpg"), quality=90)
        else:
            img.save(str(d / f"{i:02d}.jpg"), quality=90, **kind)
    for c in range(2):
        d = root / "train" / f"class{c}"
        os.makedirs(d)
        for i in range(4):
            h, w = int(rng.integers(260, 340)), int(rng.integers(260, 340))
            Image.fromarray(_picture(rng, h, w, c)).save(str(d / f"{i}.jpg"), quality=90, subsampling=2 * (i % 2))
    return root


def _val_batches(folder, mode, batch_size=5):
    from ssl4polyp_amd import mae_recipe
    args = types.SimpleNamespace(data_path=str(folder), batch_size=batch_size, num_workers=0, pin_mem=True, **mode)
    loader, prepare = mae_recipe.build_val_loader(args, torch.device(DEV, 0), 224)   # (an indexed device, as mae_recipe.start gives)
    out = []
    for batch in loader:
        imgs, labels = prepare(batch)
        out.append((imgs.clone(), labels.clone()))   # (the device path yields a per-slot buffer)
    torch.cuda.synchronize()
    return out


def test_val_batches_do_not_depend_on_where_the_work_runs(folder):
    host = _val_batches(folder, MODES[0])
    assert [len(l) for _, l in host] == [5, 5, 3] and host[0][0].shape == (5, 3, 224, 224) and host[0][0].dtype == torch.float32
    assert torch.cat([l for _, l in host]).tolist() == [0] * 7 + [1] * 6
    for mode in MODES[1:]:
        got = _val_batches(folder, mode)
        assert len(got) == len(host)
        for i, ((a, la), (b, lb)) in enumerate(zip(host, got)):
            assert a.is_cuda and b.is_cuda and torch.equal(la, lb), (mode, i)
            assert torch.equal(a, b), f"{mode}: batch {i} differs from the host transform"


def _tiny(monkeypatch):
    from ssl4polyp_amd import models_vit
    monkeypatch.setattr(models_vit, "vit_test_patch16", functools.partial(models_vit.VisionTransformer, **TINY), raising=False)
    return models_vit


def _cli(mod, folder, out, *extra, **mode):
    return mod.get_args_parser().parse_args(
        ["--model", "vit_test_patch16", "--batch_size", "5", "--nb_classes", "2", "--data_path", str(folder), "--output_dir", str(out),
         "--num_workers", "0", "--precision", "fp32", "--seed", "3", "--val_transform", mode["val_transform"], "--decode", mode["decode"],
         *extra])


def test_eval_records_do_not_depend_on_where_the_work_runs(folder, tmp_path, monkeypatch):
    from ssl4polyp_amd import main_finetune_mae, main_linprobe
    models_vit = _tiny(monkeypatch)
    torch.manual_seed(5)
    probe = models_vit.VisionTransformer(num_classes=2, **TINY)
    torch.nn.init.normal_(probe.head.weight, std=0.5)
    models_vit.add_probe_head(probe)
    tuned = models_vit.VisionTransformer(num_classes=2, global_pool=True, **TINY)
    torch.nn.init.normal_(tuned.head.weight, std=0.5)
    for mod, model, name in ((main_linprobe, probe, "probe.pth"), (main_finetune_mae, tuned, "tuned.pth")):
        torch.save({"model": model.state_dict()}, tmp_path / name)
        records = []
        for mode in MODES:
            _, _, hist = mod.run(_cli(mod, folder, tmp_path / "out", "--eval", "--resume", str(tmp_path / name), **mode))
            records.append(hist[0]["test"])
        print(mod.__name__, records[0])
        assert records[0]["samples"] == 13 and np.isfinite(records[0]["loss"])
        assert abs(records[0]["loss"] - np.log(2.0)) > 1e-3, "the logits do not depend on the images: the comparison shows nothing"
        assert records[1] == records[0] and records[2] == records[0]


def test_one_linprobe_epoch_with_device_decoding(folder, tmp_path, monkeypatch):
    from ssl4polyp_amd import main_linprobe
    models_vit = _tiny(monkeypatch)
    torch.manual_seed(1)
    pre = models_vit.VisionTransformer(num_classes=2, **TINY)
    ckpt = tmp_path / "pretrain.pth"
    torch.save({"model": {k: v for k, v in pre.state_dict().items() if not k.startswith("head.")}}, ckpt)
    hists = []
    for i, mode in enumerate((dict(val_transform="host", decode="host"), dict(val_transform="host", decode="device"),
                              dict(val_transform="device", decode="device"))):
        a = _cli(main_linprobe, folder, tmp_path / f"run{i}", "--epochs", "1", "--warmup_epochs", "0", "--blr", "10.0", "--finetune",
                 str(ckpt), **mode)
        a.batch_size = 4
        _, _, hist = main_linprobe.run(a)
        rec = hist[0]
        rec["train"].pop("seconds", None)
        hists.append(rec)
    print(hists[0])
    assert hists[0]["train"]["samples"] == 8 and hists[0]["test"]["samples"] == 13 and np.isfinite(hists[0]["train"]["loss"])
    for h in hists[1:]:
        assert h["train"] == hists[0]["train"] and h["test"] == hists[0]["test"]
