"""Image-folder input on the host (no GPU): torchvision ImageFolder's discovery and pil_loader restated by
ssl4polyp_amd.folder, the packed RaggedFrames batch, per-frame RandomResizedCrop boxes, the pre-training CLI's data flags and the
ragged augmenter's refusal of host frames (mae/main_pretrain.py:156-190)."""
import os

import numpy as np
import pytest
import torch


def _save(path, arr, mode=None):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    img = Image.fromarray(arr)
    if mode is not None:
        img = img.convert(mode)
    img.save(path)


def _rgb(h, w, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture
def tree(tmp_path):
    """b/ (class 1) and a/ (class 0): nested directory, upper-case extension, a text file, a symlinked directory, grey and
    palette PNGs."""
    root = tmp_path / "root"
    _save(str(root / "b" / "x.png"), _rgb(9, 7, 1))
    _save(str(root / "b" / "sub" / "deep.JPG"), _rgb(16, 24, 2))
    _save(str(root / "a" / "grey.png"), _rgb(11, 5, 3), "L")
    _save(str(root / "a" / "pal.png"), _rgb(6, 13, 4), "P")
    _save(str(root / "a" / "c.bmp"), _rgb(4, 4, 5))
    (root / "a" / "notes.txt").write_text("not an image")
    _save(str(tmp_path / "elsewhere" / "linked.png"), _rgb(5, 8, 6))
    os.symlink(str(tmp_path / "elsewhere"), str(root / "a" / "zlink"))
    return root


def test_image_folder_discovery_and_decoding(tree):
    from PIL import Image
    from ssl4polyp_amd.folder import ImageFolderFrames
    ds = ImageFolderFrames(str(tree))
    assert ds.classes == ["a", "b"] and ds.class_to_idx == {"a": 0, "b": 1}
    rel = [(os.path.relpath(p, str(tree)), t) for p, t in ds.samples]
    assert rel == [("a/c.bmp", 0), ("a/grey.png", 0), ("a/pal.png", 0), (os.path.join("a", "zlink", "linked.png"), 0),
                   ("b/x.png", 1), (os.path.join("b", "sub", "deep.JPG"), 1)]
    assert len(ds) == 6 and ds.targets == [0, 0, 0, 0, 1, 1]
    for i, (p, t) in enumerate(ds.samples):
        frame, label = ds[i]
        want = np.asarray(Image.open(p).convert("RGB"))
        assert label == t and frame.dtype == np.uint8 and frame.shape == want.shape and np.array_equal(frame, want)
    assert ds[1][0].shape == (11, 5, 3) and ds[2][0].shape == (6, 13, 3)   # grey / palette come back as RGB


def test_image_folder_without_images_raises(tmp_path):
    from ssl4polyp_amd.folder import ImageFolderFrames
    (tmp_path / "only" / "cls").mkdir(parents=True)
    (tmp_path / "only" / "cls" / "readme.txt").write_text("x")
    with pytest.raises(FileNotFoundError):
        ImageFolderFrames(str(tmp_path / "only"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        ImageFolderFrames(str(tmp_path / "empty"))


def test_ragged_collate_packs_frames():
    from ssl4polyp_amd.data import RaggedFrames
    from ssl4polyp_amd.folder import ragged_collate
    frames = [_rgb(5, 7, 1), _rgb(3, 2, 2), _rgb(8, 8, 3)]
    rf, labels = ragged_collate([(f, i + 3) for i, f in enumerate(frames)])
    assert isinstance(rf, RaggedFrames) and len(rf) == 3 and not rf.is_cuda
    assert labels.dtype == torch.int64 and labels.tolist() == [3, 4, 5]
    assert rf.offset.tolist() == [0, 105, 123] and rf.hw.tolist() == [[5, 7], [3, 2], [8, 8]]
    assert rf.data.numel() == 105 + 18 + 192 and rf.data.dtype == torch.uint8
    for b, f in enumerate(frames):
        assert np.array_equal(rf.frame(b).numpy(), f)
    t = RaggedFrames.from_frames([torch.from_numpy(f) for f in frames])
    assert torch.equal(t.data, rf.data) and torch.equal(t.offset, rf.offset)
    with pytest.raises(ValueError):
        RaggedFrames(rf.data[:200], rf.offset, rf.hw)        # the last frame would run past the data
    with pytest.raises(ValueError):
        RaggedFrames.from_frames([np.zeros((2, 2, 3), dtype=np.float32)])


def test_folder_loader_batches(tree):
    from ssl4polyp_amd.data import RaggedFrames
    from ssl4polyp_amd.folder import folder_loader
    ld = folder_loader(str(tree), batch_size=4, world=1, rank=0, seed=3, num_workers=0, pin_memory=False)
    assert len(ld) == 1   # drop_last: 6 images -> one batch of 4
    ld.sampler.set_epoch(0)
    (rf, labels), = list(ld)
    order = list(iter(ld.sampler))[:4]
    assert isinstance(rf, RaggedFrames) and len(rf) == 4
    assert labels.tolist() == [ld.dataset.targets[i] for i in order]
    for b, i in enumerate(order):
        assert np.array_equal(rf.frame(b).numpy(), ld.dataset[i][0])


def test_draw_rrc_boxes_per_frame_sizes():
    from ssl4polyp_amd.data import draw_rrc_boxes
    B = 9
    a = draw_rrc_boxes(B, 576, 720, torch.Generator().manual_seed(5))
    b = draw_rrc_boxes(B, [576] * B, np.full(B, 720), torch.Generator().manual_seed(5))
    assert np.array_equal(a, b)
    hs = [576, 1080, 224, 150, 333, 1, 50]
    ws = [720, 1920, 224, 333, 150, 50, 1]
    boxes = draw_rrc_boxes(len(hs), hs, ws, torch.Generator().manual_seed(6))
    for (t, l, h, w), H, W in zip(boxes, hs, ws):
        assert h > 0 and w > 0 and t >= 0 and l >= 0 and t + h <= H and l + w <= W
    # 1 x 50 and 50 x 1: no try can fit, so get_params takes its central-crop fallback (in_ratio outside the ratio range)
    assert tuple(boxes[5]) == (0, 24, 1, 1)
    assert tuple(boxes[6]) == (24, 0, 1, 1)
    with pytest.raises(ValueError):
        draw_rrc_boxes(3, [10, 10], [10, 10, 10])


def test_pretrain_cli_data_flags_default_as_the_reference():
    from ssl4polyp_amd.main_pretrain import get_args_parser
    a = get_args_parser().parse_args([])
    assert a.data_path == "/datasets01/imagenet_full_size/061417/"
    assert a.no_train_dir is False and a.num_workers == 10 and a.pin_mem is True
    b = get_args_parser().parse_args(["--data_path", "/x", "--no_train_dir", "--num_workers", "3", "--no_pin_mem"])
    assert (b.data_path, b.no_train_dir, b.num_workers, b.pin_mem) == ("/x", True, 3, False)
    assert get_args_parser().parse_args(["--pin_mem"]).pin_mem is True


def test_ragged_augmenter_refuses_host_frames():
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePerturber, RaggedFrames
    rf = RaggedFrames.from_frames([_rgb(30, 40, 1), _rgb(20, 10, 2)])
    aug = DeviceAugmenter("cpu", size=16)
    boxes = np.array([[0, 0, 30, 40], [0, 0, 20, 10]], dtype=np.int32)
    for call in (lambda: aug.resize(rf), lambda: aug.random_resized_crop(rf, boxes), lambda: aug.mae_transform(rf, boxes),
                 lambda: aug(rf), lambda: DevicePerturber("cpu").eval_transform(rf, size=16)):
        with pytest.raises(_lib.PolypMaeError):
            call()


@pytest.mark.parametrize("uniform", [False, True])
def test_check_boxes_accepts_full_frames_and_refuses_each_violation(uniform):
    """The one crop-box check: per-frame sizes, and a uniform batch's one size broadcast to [B, 2]."""
    from ssl4polyp_amd.data import _check_boxes, _whole_frame_boxes
    hw = np.broadcast_to((5, 7), (3, 2)) if uniform else np.array([(5, 7), (4, 4), (9, 2)], dtype=np.int64)
    full = _whole_frame_boxes(hw)
    assert full.tolist() == [[0, 0, h, w] for h, w in hw.tolist()]
    for given in (full, full.astype(np.int64), full.tolist(), np.asfortranarray(full)):
        got = _check_boxes(given, hw)
        assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.shape == (3, 4) and np.array_equal(got, full)
    H, W = (int(v) for v in hw[1])
    for bad in ((0, 0, 0, W),            # h = 0
                (0, -1, H, 1),           # left = -1
                (1, 0, H, W),            # top + h = H + 1
                (0, 1, H, W)):           # left + w = W + 1
        boxes = full.copy()
        boxes[1] = bad
        with pytest.raises(ValueError):
            _check_boxes(boxes, hw)
    for wrong_shape in (full[:2], full[:, :3], full.reshape(-1)):
        with pytest.raises(ValueError):
            _check_boxes(wrong_shape, hw)


def test_scratch_exact_and_grow_on_the_host():
    """_Scratch without a GPU (upload needs one): grow never shrinks, exact follows shape and dtype."""
    from ssl4polyp_amd.data import _Scratch
    sc = _Scratch("cpu")
    a = sc.grow("ws", 100, torch.uint8)
    assert a.ndim == 1 and a.numel() >= 100 and a.dtype == torch.uint8 and a.device.type == "cpu"
    assert sc.grow("ws", 10, torch.uint8).data_ptr() == a.data_ptr() and sc.grow("ws", 10, torch.uint8).numel() == a.numel()
    assert sc.grow("ws", 100, torch.uint8) is a
    b = sc.grow("ws", 101, torch.uint8)
    assert b.numel() >= 101 and b is not a and sc.bufs["ws"] is b
    assert sc.grow("empty", 0, torch.int16).numel() >= 1   # (a pointer the C entries accept)
    x = sc.exact("x", (2, 3), torch.uint8)
    assert x.shape == (2, 3) and sc.exact("x", (2, 3), torch.uint8) is x
    y = sc.exact("x", (3, 2), torch.uint8)
    assert y is not x and y.shape == (3, 2)
    z = sc.exact("x", (3, 2), torch.int32)
    assert z is not y and z.dtype == torch.int32 and sc.bufs["x"] is z
    assert sc.exact("other", (3, 2), torch.int32) is not z
