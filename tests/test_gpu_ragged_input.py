"""Mixed-size frames on the device (pm_aug_resized_crop_ragged_u8, RaggedFrames, the ragged paths of DeviceAugmenter /
DevicePerturber / DevicePrefetcher) and MAE pre-training from an image folder (mae/main_pretrain.py:156-190): every image result
against Pillow itself, frame by frame, BYTE FOR BYTE."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(576, 720), (1080, 1920), (224, 224), (150, 333), (333, 150)]


def _frame(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / (7.0 + seed) + c) * np.cos(yy / 11.0 - c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 20, (H, W, 3)), 0, 255).astype(np.uint8)


def _pil_crop_resize(frame, box, S, bicubic):
    from PIL import Image
    t, l, h, w = (int(v) for v in box)
    img = Image.fromarray(frame).crop((l, t, l + w, t + h))
    return np.asarray(img.resize((S, S), Image.BICUBIC if bicubic else Image.BILINEAR))


def _pil_resize(frame, S):
    from PIL import Image
    return np.asarray(Image.fromarray(frame).resize((S, S), Image.BILINEAR))


def test_ragged_resized_crop_equals_pillow_per_frame():
    """One batch of five native sizes (portrait, landscape, 1080p, identity, upscale): the device crop + resize of every frame equals
    Pillow's crop((l, t, l + w, t + h)).resize((224, 224), BICUBIC | BILINEAR) of that frame."""
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames, draw_rrc_boxes
    frames = [_frame(H, W, i) for i, (H, W) in enumerate(SIZES)]
    rf = RaggedFrames.from_frames(frames).to(DEV)
    boxes = draw_rrc_boxes(len(frames), [h for h, _ in SIZES], [w for _, w in SIZES], torch.Generator().manual_seed(3))
    boxes[2] = (0, 0, 224, 224)          # the identity
    boxes[3] = (150 - 19, 333 - 23, 19, 23)  # a small corner: strong upscaling
    aug = DeviceAugmenter(DEV, size=224)
    for bicubic in (True, False):
        got = aug.random_resized_crop(rf, boxes, bicubic=bicubic).cpu().numpy()
        for b, f in enumerate(frames):
            assert np.array_equal(got[b], _pil_crop_resize(f, boxes[b], 224, bicubic)), (bicubic, b)
    assert np.array_equal(got[2], frames[2])
    # boxes drawn by the augmenter from each frame's own size
    g = torch.Generator().manual_seed(9)
    got = aug.random_resized_crop(rf, generator=g).cpu().numpy()
    drawn = draw_rrc_boxes(len(frames), [h for h, _ in SIZES], [w for _, w in SIZES], torch.Generator().manual_seed(9))
    for b, f in enumerate(frames):
        assert np.array_equal(got[b], _pil_crop_resize(f, drawn[b], 224, True)), b
    with pytest.raises(ValueError):   # a 300 x 300 box fits the two large frames only
        aug.random_resized_crop(rf, np.tile(np.array([[0, 0, 300, 300]], dtype=np.int32), (5, 1)))


def test_ragged_entry_on_a_uniform_batch_equals_the_uniform_entry():
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames, draw_rrc_boxes
    B, H, W = 6, 576, 720
    x = np.stack([_frame(H, W, 20 + b) for b in range(B)])
    boxes = draw_rrc_boxes(B, H, W, torch.Generator().manual_seed(4))
    aug = DeviceAugmenter(DEV, size=224)
    uni = aug.random_resized_crop(torch.from_numpy(x).to(DEV), boxes).clone()
    rag = aug.random_resized_crop(RaggedFrames.from_frames(list(x)).to(DEV), boxes)
    assert torch.equal(uni, rag)
    # the C entry refuses bad scalars and missing tables
    lib = _lib.load()
    rf = RaggedFrames.from_frames(list(x[:1])).to(DEV)
    box = torch.from_numpy(boxes[:1]).to(DEV)
    ws = torch.empty(int(lib.pm_aug_resized_crop_workspace_bytes(1, H, W, 224)), dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 224, 224, 3, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    args = lambda **kw: [rf.data.data_ptr(), kw.get("off", rf.offset.data_ptr()), kw.get("hw", rf.hw.data_ptr()),
                         box.data_ptr(), out.data_ptr(), 1, kw.get("B", 1), kw.get("Hm", H), W, 224, ws.data_ptr(),
                         kw.get("wsb", ws.numel()), st]
    assert lib.pm_aug_resized_crop_ragged_u8(*args(off=None)) == -1
    assert lib.pm_aug_resized_crop_ragged_u8(*args(hw=None)) == -1
    assert lib.pm_aug_resized_crop_ragged_u8(*args(B=0)) == _lib.PM_ESHAPE
    assert lib.pm_aug_resized_crop_ragged_u8(*args(Hm=0)) == _lib.PM_ESHAPE
    assert lib.pm_aug_resized_crop_ragged_u8(*args(wsb=ws.numel() - 1)) == -1
    assert lib.pm_aug_resized_crop_ragged_u8(*args()) == 0
    assert torch.equal(out[0], uni[0])


def test_ragged_resize_and_cls_chain_equal_pillow_then_the_oracle():
    from oracle import augment_ref as R
    from oracle.input_ref import to_tensor_normalize
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames, draw_train_params
    frames = [_frame(H, W, 40 + i) for i, (H, W) in enumerate(SIZES)]
    rf = RaggedFrames.from_frames(frames).to(DEV)
    aug = DeviceAugmenter(DEV, size=224)
    resized = np.stack([_pil_resize(f, 224) for f in frames])
    assert np.array_equal(aug.resize(rf).cpu().numpy(), resized)
    p = draw_train_params(len(frames), torch.Generator().manual_seed(5))
    want_u8 = R.train_augment(resized, p)
    assert np.array_equal(aug(rf, params=p, to_f32=False).cpu().numpy(), want_u8)
    got = aug(rf, params=p)
    assert got.shape == (5, 3, 224, 224) and torch.equal(got.cpu(), to_tensor_normalize(torch.from_numpy(want_u8)))


def test_perturber_eval_transform_on_a_ragged_batch():
    from ssl4polyp_amd.data import DevicePerturber, RaggedFrames
    frames = [_frame(H, W, 60 + i) for i, (H, W) in enumerate(SIZES)]
    rows = [{"variant": v, "frame_id": i} for i, v in enumerate(("blur_1p5", "clean", "bc_b1p3_c0p7", "occ_a0p2", "jpeg_q40"))]
    rows[4]["jpeg_q"] = 40
    pt = DevicePerturber(DEV)
    got = pt.eval_transform(RaggedFrames.from_frames(frames).to(DEV), rows)
    want = pt.eval_transform(torch.from_numpy(np.stack([_pil_resize(f, 224) for f in frames])).to(DEV), rows)
    assert torch.equal(got, want)
    labels = torch.arange(5)
    (x, lab, r), = list(pt.batches([(RaggedFrames.from_frames(frames), labels, rows)]))
    assert torch.equal(x, want) and torch.equal(lab.cpu(), labels) and r == rows


def _folder(root, n_per_size=4):
    """JPEG + PNG at three native sizes under one class directory."""
    from PIL import Image
    d = os.path.join(root, "unlabelled")
    os.makedirs(d)
    k = 0
    for H, W in ((120, 160), (200, 90), (64, 64)):
        for i in range(n_per_size):
            Image.fromarray(_frame(H, W, 80 + k)).save(os.path.join(d, f"{k:03d}." + ("jpg" if k % 2 else "png")), quality=90)
            k += 1
    return root


def test_prefetcher_over_an_image_folder_mae_transform(tmp_path):
    from oracle.input_ref import to_tensor_normalize
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher, draw_rrc_boxes
    from ssl4polyp_amd.folder import folder_loader
    root = _folder(str(tmp_path))
    B = 4
    ld = folder_loader(root, batch_size=B, world=1, rank=0, seed=0, num_workers=2, pin_memory=True)
    ld.sampler.set_epoch(0)
    order = list(iter(ld.sampler))
    ds = ld.dataset

    def run(seed):
        pf = DevicePrefetcher(ld, DEV, augment=DeviceAugmenter(DEV), transform="mae", generator=torch.Generator().manual_seed(seed))
        out = [(x.clone(), y.clone()) for x, y in pf]
        assert pf._pin == [{}, {}]   # the loader pinned the batches: no second staging copy
        return out
    a, b = run(7), run(7)
    assert len(a) == len(order) // B == 3
    for i, (x, y) in enumerate(a):
        assert x.shape == (B, 3, 224, 224) and x.dtype == torch.float32 and x.is_cuda and y.is_cuda
        assert y.cpu().tolist() == [ds.targets[j] for j in order[i * B:(i + 1) * B]]
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a, b))
    # batch 0 on the host: the same generator draws (boxes per frame, then the flips), Pillow crop + resize(BICUBIC), flip,
    # ToTensor + Normalize
    g = torch.Generator().manual_seed(7)
    fr = [ds[j][0] for j in order[:B]]
    boxes = draw_rrc_boxes(B, [f.shape[0] for f in fr], [f.shape[1] for f in fr], g)
    hflip = torch.rand(B, generator=g) < 0.5
    want_u8 = np.stack([_pil_crop_resize(f, boxes[k], 224, True) for k, f in enumerate(fr)])
    assert torch.equal(a[0][0].cpu(), to_tensor_normalize(torch.from_numpy(want_u8), hflip.to(torch.uint8)))


def test_prefetcher_ragged_staging_buffers_only_grow():
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher, RaggedFrames
    big = [_frame(300, 400, 1), _frame(280, 200, 2)]
    small = [_frame(100, 120, 3), _frame(90, 60, 4)]
    batches = [(RaggedFrames.from_frames(f), torch.arange(2) + i) for i, f in enumerate((big, big, small, small, small))]
    pf = DevicePrefetcher(batches, DEV, augment=DeviceAugmenter(DEV), transform="train", generator=torch.Generator().manual_seed(1))
    ptrs = None
    n = 0
    for i, (x, y) in enumerate(pf):
        assert x.shape == (2, 3, 224, 224) and torch.equal(y.cpu(), torch.arange(2) + i)
        if i == 1:   # both slots have staged a big batch
            ptrs = [(pf._pin[s]["data"].data_ptr(), pf._dev[s]["data"].data_ptr()) for s in (0, 1)]
        n += 1
    assert n == 5
    nbig = batches[0][0].data.numel()
    for s in (0, 1):
        assert (pf._pin[s]["data"].data_ptr(), pf._dev[s]["data"].data_ptr()) == ptrs[s]
        assert pf._pin[s]["data"].numel() == pf._dev[s]["data"].numel() == nbig
    assert pf.augment._scratch.bufs["crop_ws"].numel() >= 1


def test_prefetcher_mixed_batch_kinds_share_slots():
    """Uniform, ragged and compressed batches interleaved through one prefetcher, whose two slots keep their staging buffers by
    name: two kinds carry arrays called `offset` and `hw`, the uniform frames share a name with the int32 `frames` table of a
    compressed batch, batch sizes change between the visits of a slot and a smaller batch follows a larger one of its kind.
    transform="eval" draws nothing, so every batch must come out as a fresh prefetcher yields it alone -- decoded in two steps
    or fused."""
    from pack_files import encode
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher, RaggedFrames
    from ssl4polyp_amd.jpeg import JpegBatch
    jpg = lambda H, W, seed: encode(_frame(H, W, seed), quality=90)
    ragged = lambda: RaggedFrames.from_frames([_frame(40, 56, 3), _frame(64, 48, 4)])
    jb3 = JpegBatch.from_bytes([jpg(48, 64, 5), jpg(33, 47, 6), encode(_frame(30, 20, 7), "png")])
    jb2 = JpegBatch.from_bytes([jpg(33, 47, 8), jpg(16, 24, 9)])
    assert jb3.meta["fallback"] == [2] and jb2.meta["fallback"] == []
    g = torch.Generator().manual_seed(12)
    frames = [torch.randint(0, 256, (3, 48, 64, 3), dtype=torch.uint8, generator=g), ragged(), jb3,
              torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8, generator=g), ragged(), jb2]
    batches = [(f, torch.arange(len(f)) + i) for i, f in enumerate(frames)]

    def run(loader, fused=False):
        pf = DevicePrefetcher(loader, DEV, augment=DeviceAugmenter(DEV, size=32), transform="eval", fused_decode=fused)
        return [(x.clone(), y.clone()) for x, y in pf]
    alone = [run([b])[0] for b in batches]
    for fused in (False, True):
        mixed = run(batches, fused)
        assert len(mixed) == 6
        for i, ((x, y), (xa, ya)) in enumerate(zip(mixed, alone)):
            assert x.shape == (len(frames[i]), 3, 32, 32) and torch.equal(x, xa), (fused, i)
            assert torch.equal(y.cpu(), batches[i][1]) and torch.equal(ya.cpu(), batches[i][1]), (fused, i)


def test_main_pretrain_from_an_image_folder(tmp_path):
    """python -m ssl4polyp_amd.main_pretrain --data_path <folder> --no_train_dir: one epoch, a finite loss, a loadable checkpoint."""
    root = _folder(str(tmp_path / "data"))
    out = tmp_path / "out"
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    p = subprocess.run([sys.executable, "-m", "ssl4polyp_amd.main_pretrain", "--data_path", root, "--no_train_dir", "--epochs", "1",
                        "--batch_size", "8", "--num_workers", "2", "--output_dir", str(out), "--log_every", "1"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    rec = [json.loads(ln) for ln in open(out / "log.txt")]
    assert len(rec) == 1 and math.isfinite(rec[0]["train_loss"]) and rec[0]["epoch"] == 0
    import ssl4polyp_amd as A
    from ssl4polyp_amd.train import load_mae_checkpoint
    ck = out / "ckpts" / "checkpoint-0.pth"
    m = A.mae_vit_base_patch16()
    assert load_mae_checkpoint(ck, m) == 0
    sd = torch.load(ck, map_location="cpu", weights_only=False)["model"]
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())
