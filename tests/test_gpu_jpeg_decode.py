"""Baseline JPEG decoding on the device (pm_jpeg_decode, data.DeviceJpegDecoder, the JpegBatch path of DevicePrefetcher,
main_pretrain --decode device): every frame against Pillow decoding the same bytes on this machine, BYTE FOR BYTE."""
import io
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
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 5), (7, 13), (8, 8), (16, 16), (17, 31), (33, 17), (150, 333), (224, 224), (576, 720),
         (1080, 1920)]


def _content(h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    kind = seed % 4
    if kind == 0:   # smooth gradients
        return np.stack([(xx * 255 // max(w - 1, 1) + 40 * c) % 256 for c in range(3)], -1).astype(np.uint8)
    if kind == 1:   # noise
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 2:   # flat areas: long zero runs, ZRL, EOB
        out = np.full((h, w, 3), (40, 120, 200), dtype=np.uint8)
        out[h // 2:, w // 3:] = (250, 10, 128)
        return out
    sat = np.zeros((h, w, 3), dtype=np.uint8)   # saturated colours: the range limit
    sat[..., 0] = np.where((xx // 3 + yy // 5) % 2, 255, 0)
    sat[..., 1] = np.where((xx // 4) % 2, 0, 255)
    sat[..., 2] = np.where((yy // 2) % 2, 255, 0)
    return sat


def _jpeg(arr, sampling, quality, optimize, restart, progressive=False) -> bytes:
    from PIL import Image
    im = Image.fromarray(arr)
    kw = {"quality": quality, "optimize": optimize, "progressive": progressive}
    if sampling == "L":
        im = im.convert("L")
    else:
        kw["subsampling"] = sampling
    if restart == "block":
        kw["restart_marker_blocks"] = 1
    elif restart == "row":
        kw["restart_marker_rows"] = 1
    b = io.BytesIO()
    try:
        im.save(b, format="JPEG", **kw)
    except OSError:   # Pillow's optimize buffer holds 2 bytes per pixel at q >= 95: saturated / noisy 4:4:4 frames overflow it
        if not optimize:
            raise
        return _jpeg(arr, sampling, quality, False, restart, progressive)
    return b.getvalue()


def _pil(data) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _decode(files, decoder=None):
    from ssl4polyp_amd.data import DeviceJpegDecoder
    from ssl4polyp_amd.jpeg import JpegBatch
    jb = JpegBatch.from_bytes(files)
    dec = decoder or DeviceJpegDecoder(DEV)
    rf = dec(jb.to(DEV))
    torch.cuda.synchronize()
    return rf, jb


def _assert_equal_to_pillow(files, rf):
    from ssl4polyp_amd.data import RaggedFrames
    want = RaggedFrames.from_frames([_pil(f) for f in files])
    assert torch.equal(rf.offset.cpu(), want.offset) and torch.equal(rf.hw.cpu(), want.hw)
    if not torch.equal(rf.data.cpu(), want.data):
        bad = [b for b in range(len(files)) if not torch.equal(rf.frame(b).cpu(), want.frame(b))]
        raise AssertionError(f"frames {bad} differ from Pillow")


@pytest.mark.parametrize("rot", range(4))
def test_decode_matrix_equals_pillow(rot):
    """Mixed ragged batches over sizes 1x1 .. 1080x1920 x subsampling 0 / 1 / 2 / grey x quality 1 / 50 / 90 / 100 x optimize
    x restart markers none / every block / every row x gradient / noise / flat / saturated content."""
    files = []
    for i, (h, w) in enumerate(SIZES):
        for j, sampling in enumerate((0, 1, 2, "L")):
            k = i + j + rot
            if (h, w) == (1080, 1920) and k % 2:
                continue   # (keeps the test short; every option still meets a 1080p frame across the four batches)
            files.append(_jpeg(_content(h, w, k // 4 + j + i), sampling, (1, 50, 90, 100)[k % 4], bool((k // 2) % 2),
                               (None, "block", "row")[k % 3]))
    rf, jb = _decode(files)
    assert jb.meta["fallback"] == []
    _assert_equal_to_pillow(files, rf)


def test_fancy_upsampling_widths_one_to_five():
    files = [_jpeg(_content(h, w, h * 7 + w), s, 90, False, None) for s in (1, 2) for h in range(1, 6) for w in range(1, 6)]
    rf, _ = _decode(files)
    _assert_equal_to_pillow(files, rf)


def test_fallback_frames_in_a_mixed_batch():
    """A progressive JPEG, a CMYK JPEG and a PNG among device frames: decoded on the host, copied into their slots."""
    from PIL import Image
    rgb = _content(45, 61, 0)
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, format="JPEG")
    png = io.BytesIO()
    Image.fromarray(_content(20, 30, 1)).save(png, format="PNG")
    files = [_jpeg(rgb, 2, 90, False, None), _jpeg(rgb, 0, 75, False, None, progressive=True), b.getvalue(),
             _jpeg(_content(77, 19, 2), "L", 90, True, "row"), png.getvalue(), _jpeg(_content(64, 64, 3), 1, 95, False, "block")]
    rf, jb = _decode(files)
    assert jb.meta["fallback"] == [1, 2, 4]
    _assert_equal_to_pillow(files, rf)


def test_corrupt_entropy_data_is_contained_and_deterministic():
    """Bytes flipped inside one file's entropy data (structure intact): the call succeeds, every other frame is exact, and two
    calls give the same bytes."""
    from ssl4polyp_amd.data import DeviceJpegDecoder
    from ssl4polyp_amd.jpeg import parse_jpeg
    good = [_jpeg(_content(96, 128, s), 2, 90, False, None) for s in range(3)]
    bad = bytearray(_jpeg(_content(96, 128, 7), 2, 90, False, "row"))
    sos = bytes(bad).index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(bad[sos + 2:sos + 4], "big")
    rng = np.random.Generator(np.random.PCG64(11))
    for p in rng.integers(start + 4, len(bad) - 8, 40):
        if bad[p] != 0xFF and bad[p - 1] != 0xFF and bad[p + 1] != 0xFF:
            bad[p] = (bad[p] ^ 0x5A) if (bad[p] ^ 0x5A) != 0xFF else 0x11
    bad = bytes(bad)
    parse_jpeg(bad)   # still routed to the device
    files = good[:2] + [bad] + good[2:]
    dec = DeviceJpegDecoder(DEV)
    rf1, jb = _decode(files, dec)
    first = rf1.data.clone()
    rf2, _ = _decode(files, dec)
    assert torch.equal(first, rf2.data)
    # a fresh decoder whose workspace and output hold garbage: nothing unwritten is read
    fresh = DeviceJpegDecoder(DEV)
    for name, n, dt in (("coef", jb.meta["blocks"] * 64, torch.int16), ("planes", jb.meta["blocks"] * 64, torch.uint8),
                        ("out", jb.meta["nbytes"], torch.uint8)):
        fresh._scratch.bufs[name] = torch.randint(0, 100, (n,), device=DEV).to(dt)
    rf3, _ = _decode(files, fresh)
    assert torch.equal(first, rf3.data)
    for b in (0, 1, 3):
        assert torch.equal(rf2.frame(b).cpu(), torch.from_numpy(_pil(files[b]).copy()))


def test_interval_that_runs_out_of_data_and_rewritten_headers_equal_pillow():
    """libjpeg's insufficient-data rule (half of one restart interval's bytes removed: the rest of that interval is grey, the next
    interval decodes normally), 16-bit DQT, Adobe APP14 transform 1 without JFIF, 'R','G','B' ids under JFIF -- and more
    Huffman tables than fit in LDS (optimized tables of 40 frames: the global-memory table path)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_jpeg_host_cpu import _cut_interval, _rebuild
    from ssl4polyp_amd.jpeg import parse_jpeg
    files = []
    for k, s in enumerate((2, 0, 1, "L")):
        base = _jpeg(_content(64, 80, k), s, 90, False, "row")
        files += [_cut_interval(base, 1), _rebuild(base, dqt16=True)]
        if s != "L":
            files += [_rebuild(base, drop_app0=True, adobe=1), _rebuild(base, ids=[82, 71, 66])]
    for f in files:
        parse_jpeg(f)   # all on the device
    rf, jb = _decode(files)
    assert jb.meta["fallback"] == []
    _assert_equal_to_pillow(files, rf)
    many = [_jpeg(_content(40 + k, 56, 4 * k + 1), (0, 1, 2)[k % 3], 50 + k, True, None) for k in range(40)]
    rf, jb = _decode(many)
    assert jb.huff.shape[0] > 31   # more tables than the LDS copy holds
    _assert_equal_to_pillow(many, rf)


def test_c_entry_refuses_bad_arguments():
    from ssl4polyp_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    p = buf.data_ptr()
    args = lambda **kw: [p, kw.get("eb", 64), p, 1, p, kw.get("nf", 1), p, 1, p, 1, None, 0, None, kw.get("nfb", 0), p, p, 0, 0, p,
                         64, st]
    assert lib.pm_jpeg_decode(*args(eb=60)) == _lib.PM_EALIGN
    assert lib.pm_jpeg_decode(*args(nf=-1)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode(*args(nfb=1)) == _lib.PM_EINVAL   # a fallback row without its table
    assert lib.pm_jpeg_decode(*args(nf=0)) == 0


def _folder(root):
    """About 40 JPEGs at three sizes (mixed samplings, qualities, restart markers) + one progressive JPEG + one PNG."""
    from PIL import Image
    d = os.path.join(root, "unlabelled")
    os.makedirs(d)
    k = 0
    for H, W in ((120, 160), (200, 90), (64, 64)):
        for i in range(13):
            data = _jpeg(_content(H, W, k), (0, 1, 2, "L")[k % 4], (60, 90, 95)[k % 3], bool(k % 2), (None, "row", "block")[k % 3])
            with open(os.path.join(d, f"{k:03d}.jpg"), "wb") as f:
                f.write(data)
            k += 1
    with open(os.path.join(d, "prog.jpg"), "wb") as f:
        f.write(_jpeg(_content(100, 140, 50), 2, 85, False, None, progressive=True))
    Image.fromarray(_content(70, 50, 51)).save(os.path.join(d, "still.png"))
    return root


@pytest.mark.parametrize("transform", ["mae", "train"])
def test_prefetcher_device_decode_equals_host_decode(tmp_path, transform):
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher
    from ssl4polyp_amd.folder import folder_loader
    root = _folder(str(tmp_path))

    def run(decode):
        ld = folder_loader(root, batch_size=8, world=1, rank=0, seed=0, num_workers=2, pin_memory=True, decode=decode)
        ld.sampler.set_epoch(0)
        pf = DevicePrefetcher(ld, DEV, augment=DeviceAugmenter(DEV), transform=transform, generator=torch.Generator().manual_seed(3))
        return [(x.clone(), y.clone()) for x, y in pf]
    host, dev = run("host"), run("device")
    assert len(host) == len(dev) == 41 // 8
    for (a, la), (b, lb) in zip(host, dev):
        assert torch.equal(la, lb) and torch.equal(a, b)


def test_main_pretrain_with_device_decoding(tmp_path):
    """python -m ssl4polyp_amd.main_pretrain --data_path <folder> --no_train_dir --decode device: one epoch, a finite loss, a
    loadable checkpoint."""
    root = _folder(str(tmp_path / "data"))
    out = tmp_path / "out"
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    p = subprocess.run([sys.executable, "-m", "ssl4polyp_amd.main_pretrain", "--data_path", root, "--no_train_dir", "--epochs", "1",
                        "--batch_size", "8", "--num_workers", "2", "--output_dir", str(out), "--log_every", "1", "--decode", "device"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    rec = [json.loads(ln) for ln in open(out / "log.txt")]
    assert len(rec) == 1 and math.isfinite(rec[0]["train_loss"]) and rec[0]["epoch"] == 0
    import ssl4polyp_amd as A
    from ssl4polyp_amd.train import load_mae_checkpoint
    m = A.mae_vit_base_patch16()
    assert load_mae_checkpoint(out / "ckpts" / "checkpoint-0.pth", m) == 0
