"""Decoding straight into the resized crop (DeviceJpegDecoder.resized_crop: pm_jpeg_decode_planes + pm_jpeg_resized_crop_u8, and
DevicePrefetcher(fused_decode=True)): every result against Pillow's own decode -> crop -> resize of the FILE, byte for byte, and
against the two-step path (decode to RGB frames, then the ragged resized crop)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pack_files import FALLBACK, SIZES, encode, frame, make_files, pil_resized

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = 32


@pytest.fixture(scope="module")
def files():
    return [d for _, d in make_files()]


@pytest.fixture(scope="module")
def batch(files):
    from ssl4polyp_amd.jpeg import JpegBatch
    b = JpegBatch.from_bytes(files)
    assert b.meta["fallback"] == FALLBACK and b.meta["n_subseq"] > 0
    return b.to(DEV)


def _whole(sizes):
    boxes = np.zeros((len(sizes), 4), dtype=np.int32)
    boxes[:, 2:] = sizes
    return boxes


def _boxes():
    """Frames 0, 4: odd top and left, reaching the bottom-right pixel; frame 7: a 19 x 23 box with odd top / left that does (strong
    upscaling); the rest drawn as RandomResizedCrop draws them."""
    from ssl4polyp_amd.data import draw_rrc_boxes
    boxes = draw_rrc_boxes(len(SIZES), [h for h, _ in SIZES], [w for _, w in SIZES], torch.Generator().manual_seed(11))
    for b, (t, l) in ((0, (3, 5)), (4, (7, 1))):
        boxes[b] = (t, l, SIZES[b][0] - t, SIZES[b][1] - l)
    boxes[7] = (160 - 19, 200 - 23, 19, 23)
    assert all(boxes[b][0] % 2 == 1 and boxes[b][1] % 2 == 1 for b in (0, 4, 7))
    return boxes


def test_whole_frame_bilinear_equals_pillow_per_file(files, batch):
    from ssl4polyp_amd.data import DeviceJpegDecoder
    dec = DeviceJpegDecoder(DEV)
    got = dec.resized_crop(batch, _whole(SIZES), S, False)
    assert got.shape == (10, S, S, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    for b, f in enumerate(files):
        want = pil_resized(f, S)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    assert "out" not in dec._scratch.bufs   # no full-size RGB buffer
    assert dec.stats()["subsequences"] == batch.meta["n_subseq"]


def test_per_frame_boxes_equal_pillow_and_the_sequential_way_out(files, batch):
    from ssl4polyp_amd.data import DeviceAugmenter, DeviceJpegDecoder
    boxes = _boxes()
    dec, seq = DeviceJpegDecoder(DEV), DeviceJpegDecoder(DEV, sync_rounds=0)
    two_step = DeviceAugmenter(DEV, size=S)
    for bicubic in (True, False):
        got = dec.resized_crop(batch, boxes, S, bicubic)
        assert torch.equal(seq.resized_crop(batch, boxes, S, bicubic), got)
        assert torch.equal(two_step._resized_crop(DeviceJpegDecoder(DEV)(batch), boxes, bicubic, "t"), got)
        got = got.cpu().numpy()
        for b, f in enumerate(files):
            want = pil_resized(f, S, boxes[b], bicubic)
            assert np.array_equal(got[b], want), (bicubic, b, boxes[b].tolist(), int((got[b] != want).sum()))
    # a caller's output tensor is written in place; boxes outside their frame are refused on the host
    mine = torch.zeros(10, S, S, 3, dtype=torch.uint8, device=DEV)
    assert dec.resized_crop(batch, boxes, S, False, out=mine) is mine and np.array_equal(mine.cpu().numpy(), got)
    bad = boxes.copy()
    bad[1] = (0, 0, 6, 3)
    with pytest.raises(ValueError):
        dec.resized_crop(batch, bad, S, False)


def test_fallback_frames_between_device_frames(files):
    """The host-built source table (frame row, or -1 - k for fallback row k) with the host-decoded frames first and in the middle of
    the batch, not at its end."""
    from ssl4polyp_amd.data import DeviceJpegDecoder, draw_rrc_boxes
    from ssl4polyp_amd.jpeg import JpegBatch
    order = [8, 0, 7, 9, 4, 6, 2]
    fs = [files[i] for i in order]
    b = JpegBatch.from_bytes(fs)
    assert b.meta["fallback"] == [0, 3]
    sizes = [SIZES[i] for i in order]
    dec = DeviceJpegDecoder(DEV)
    boxes = draw_rrc_boxes(len(fs), [h for h, _ in sizes], [w for _, w in sizes], torch.Generator().manual_seed(2))
    for bx, bicubic in ((_whole(sizes), False), (boxes, True)):
        got = dec.resized_crop(b.to(DEV), bx, S, bicubic).cpu().numpy()
        for k, f in enumerate(fs):
            want = pil_resized(f, S, bx[k], bicubic)
            assert np.array_equal(got[k], want), (bicubic, k, order[k], int((got[k] != want).sum()))


def test_large_frames_at_224():
    """Long tap rows (1920 -> 224) and a grid of many blocks."""
    from ssl4polyp_amd.data import DeviceJpegDecoder
    from ssl4polyp_amd.jpeg import JpegBatch
    sizes = [(576, 720), (1080, 1920)]
    fs = [encode(frame(H, W, 30 + i), subsampling=2, quality=90) for i, (H, W) in enumerate(sizes)]
    b = JpegBatch.from_bytes(fs)
    assert b.meta["fallback"] == []
    got = DeviceJpegDecoder(DEV).resized_crop(b.to(DEV), _whole(sizes), 224, False).cpu().numpy()
    for i, f in enumerate(fs):
        want = pil_resized(f, 224)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))


def test_c_entry_refuses_bad_arguments(files, batch):
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.data import DeviceJpegDecoder
    lib = _lib.load()
    dec = DeviceJpegDecoder(DEV)
    boxes = _whole(SIZES)
    want = dec.resized_crop(batch, boxes, S, False).clone()   # (leaves the decoded planes in dec._scratch.bufs["planes"])
    B, t, m = 10, batch.t, batch.meta
    Hm, Wm = int(m["hw"][:, 0].max()), int(m["hw"][:, 1].max())
    need = ctypes.c_size_t(0)
    assert lib.pm_jpeg_resized_crop_workspace(B, Hm, Wm, S, ctypes.byref(need)) == 0
    assert need.value == lib.pm_aug_resized_crop_workspace_bytes(B, Hm, Wm, S)
    assert lib.pm_jpeg_resized_crop_workspace(0, Hm, Wm, S, ctypes.byref(need)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_resized_crop_workspace(B, Hm, Wm, 0, ctypes.byref(need)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_resized_crop_workspace(65536, Hm, Wm, S, ctypes.byref(need)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_resized_crop_workspace(B, Hm, Wm, S, None) == _lib.PM_EINVAL
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(B, S, S, 3, dtype=torch.uint8, device=DEV)
    source = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, -1, -2], dtype=torch.int32, device=DEV)
    box = torch.from_numpy(boxes).to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    planes = dec._scratch.bufs["planes"]

    def call(**kw):
        g = lambda k, v: kw.get(k, v)
        return lib.pm_jpeg_resized_crop_u8(g("planes", planes.data_ptr()), g("blocks", m["blocks"]), g("frames", t["frames"].data_ptr()),
                                           g("n_frames", 8), g("fallback", t["fallback"].data_ptr()), t["fallback"].numel(),
                                           g("table", t["fallback_table"].data_ptr()), g("n_fallback", 2),
                                           g("source", source.data_ptr()), g("hw", t["hw"].data_ptr()), g("box", box.data_ptr()),
                                           g("out", out.data_ptr()), 0, g("B", B), g("Hm", Hm), Wm, g("S", S),
                                           g("ws", ws.data_ptr()), g("wsb", need.value), st)
    for k in ("source", "hw", "box", "out", "ws", "frames", "planes", "table", "fallback"):
        assert call(**{k: None}) == _lib.PM_EINVAL, k
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(Hm=0), dict(S=0), dict(blocks=-1), dict(n_frames=-1), dict(n_fallback=-1)):
        assert call(**kw) == _lib.PM_ESHAPE, kw
    assert call(wsb=need.value - 1) == _lib.PM_EINVAL          # short
    assert call(ws=ws.data_ptr() + 8) == _lib.PM_EINVAL        # misaligned
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                 # nothing was launched
    assert call() == 0
    assert torch.equal(out, want)
    # the planes-only decode entry validates as pm_jpeg_decode_parallel does
    assert lib.pm_jpeg_decode_planes(t["entropy"].data_ptr(), t["entropy"].numel(), t["intervals"].data_ptr(), t["intervals"].shape[0],
                                     t["frames"].data_ptr(), 8, t["huff"].data_ptr(), t["huff"].shape[0], t["quant"].data_ptr(),
                                     t["quant"].shape[0], dec._scratch.bufs["coef"].data_ptr(), planes.data_ptr(), m["blocks"],
                                     t["subseq"].data_ptr(), t["subseq"].numel(), 9, ws.data_ptr(), ws.numel(), None, st) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode_planes(t["entropy"].data_ptr(), t["entropy"].numel(), t["intervals"].data_ptr(), t["intervals"].shape[0],
                                     t["frames"].data_ptr(), 8, t["huff"].data_ptr(), t["huff"].shape[0], t["quant"].data_ptr(),
                                     t["quant"].shape[0], dec._scratch.bufs["coef"].data_ptr(), planes.data_ptr(), m["blocks"],
                                     t["subseq"].data_ptr(), t["subseq"].numel(), 2, ws.data_ptr(), 16, None, st) == _lib.PM_EINVAL


def test_prefetcher_fused_decode_yields_the_unfused_images(tmp_path, files):
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher
    from ssl4polyp_amd.folder import ImageFolderFrames, jpeg_collate
    d = tmp_path / "unlabelled"
    d.mkdir()
    for name, data in make_files():
        (d / name).write_bytes(data)
    ds = ImageFolderFrames(str(tmp_path), decode="device")
    ld = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, collate_fn=jpeg_collate)
    for transform in ("mae", "train", "eval"):
        runs = []
        for fused in (True, False):
            pf = DevicePrefetcher(ld, DEV, augment=DeviceAugmenter(DEV, size=S), transform=transform, fused_decode=fused,
                                  generator=torch.Generator().manual_seed(5))
            runs.append([x.clone() for x, _ in pf])
            assert ("out" in pf._decoder._scratch.bufs) == (not fused)   # the fused run never allocates the full-size RGB output
        assert [tuple(x.shape) for x in runs[0]] == [(4, 3, S, S), (4, 3, S, S), (2, 3, S, S)]
        assert all(torch.equal(a, b) for a, b in zip(*runs)), transform
    # "eval" is the plain transform: Pillow's resize of every file, ToTensor, Normalize
    from oracle.input_ref import to_tensor_normalize
    want = to_tensor_normalize(torch.from_numpy(np.stack([pil_resized(f, S) for f in files])))
    assert torch.equal(torch.cat(runs[0]).cpu(), want)
