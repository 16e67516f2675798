"""Decoding in parallel inside a restart interval (pm_jpeg_decode_parallel, data.DeviceJpegDecoder(mode="parallel")): byte for byte
Pillow's on intact files, byte for byte the one-lane-per-interval decoder's on damaged ones, and the counters say which path ran."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_jpeg_decode import DEV, _assert_equal_to_pillow, _content, _jpeg, _pil   # noqa: E402
from test_jpeg_subseq_cpu import _endo_like, _sin_noise   # noqa: E402

pytestmark = pytest.mark.gpu


def _decode(files, decoder=None, **kw):
    from ssl4polyp_amd.data import DeviceJpegDecoder
    from ssl4polyp_amd.jpeg import JpegBatch
    jb = JpegBatch.from_bytes(files)
    dec = decoder or DeviceJpegDecoder(DEV, **kw)
    rf = dec(jb.to(DEV))
    torch.cuda.synchronize()
    return rf, jb, dec


def _realistic():
    """The kinds of the first three rows of the design's table: sinusoids + noise (standard and optimized tables), endoscopy-like;
    q90 4:2:0, no restart markers, every frame many workgroups long."""
    return [_jpeg(_sin_noise(576, 720, 1), 2, 90, False, None), _jpeg(_sin_noise(576, 720, 2), 2, 90, True, None),
            _jpeg(_endo_like(576, 720, 3), 2, 90, False, None), _jpeg(_sin_noise(1080, 1920, 4), 2, 90, False, None),
            _jpeg(_endo_like(1080, 1920, 5), 2, 90, True, None)]


def test_default_mode_is_parallel():
    from ssl4polyp_amd.data import DeviceJpegDecoder
    d = DeviceJpegDecoder(DEV)
    assert d.mode == "parallel" and d.sync_rounds == 2
    with pytest.raises(ValueError):
        DeviceJpegDecoder(DEV, mode="frame")


@pytest.mark.parametrize("size", [(576, 720), (1080, 1920)])
def test_frames_that_span_many_workgroups_equal_pillow(size):
    h, w = size
    files = []
    for j, sampling in enumerate((2, 0, "L")):
        for q in (50, 90, 100):
            for opt in (False, True):
                files.append(_jpeg(_sin_noise(h, w, 10 * j + q), sampling, q, opt, None))
    rf, jb, dec = _decode(files, mode="parallel")
    assert jb.meta["fallback"] == [] and jb.meta["n_subseq"] > 256 * len(files)
    _assert_equal_to_pillow(files, rf)
    st = dec.stats()
    print("stats", size, st)
    assert st["subsequences"] == jb.meta["n_subseq"] and st["intervals"] == len(files)


def test_slow_contents_tiny_frames_and_restart_markers_equal_pillow():
    """Uniform noise, saturated stripes and the flat frame in grey (slow to synchronise), frames of 1x1 .. 17x31 in the same batch
    (intervals shorter than one subsequence), and restart markers per block / per row (thousands of one-subsequence intervals)."""
    files = [_jpeg(_content(576, 720, 1), 2, 90, False, None), _jpeg(_content(576, 720, 3), "L", 90, False, None),
             _jpeg(_content(576, 720, 2), "L", 90, False, None), _jpeg(_content(576, 720, 3), 0, 90, False, None)]
    files += [_jpeg(_content(h, w, h + w), s, 90, False, None) for (h, w), s in
              zip(((1, 1), (2, 2), (3, 5), (7, 13), (8, 8), (16, 16), (17, 31)), (0, 1, 2, "L", 2, 1, 0))]
    files += [_jpeg(_sin_noise(576, 720, 6), 2, 90, False, "block"), _jpeg(_sin_noise(576, 720, 7), 2, 90, True, "row"),
              _jpeg(_content(150, 333, 1), "L", 100, False, "block"), _jpeg(_sin_noise(576, 720, 8), 0, 100, False, "row")]
    rf, jb, dec = _decode(files, mode="parallel")
    assert jb.meta["fallback"] == [] and jb.intervals.shape[0] > 2000
    _assert_equal_to_pillow(files, rf)
    print("stats", dec.stats())


def test_counters_say_which_path_ran():
    """Default sync_rounds: no interval of the realistic frames takes the sequential way out.  sync_rounds=0: every workgroup after
    an interval's first starts from its guess, the acceptance rule refuses the interval, the sequential decoder takes it -- and the
    bytes are still Pillow's."""
    files = _realistic()
    rf, jb, dec = _decode(files)
    st = dec.stats()
    print("stats", st)
    _assert_equal_to_pillow(files, rf)
    assert st["intervals"] == len(files) and st["subsequences"] == jb.meta["n_subseq"]
    assert st["sequential_intervals"] == 0 and st["rounds_changed"] >= 1 and 1 <= st["max_workgroup_steps"] <= 257
    rf0, _, dec0 = _decode(files, sync_rounds=0)
    st0 = dec0.stats()
    print("stats sync_rounds=0", st0)
    _assert_equal_to_pillow(files, rf0)
    assert st0["sequential_intervals"] > 0 and st0["rounds_changed"] == 0
    rf1, _, dec1 = _decode(files, sync_rounds=1)
    print("stats sync_rounds=1", dec1.stats())
    _assert_equal_to_pillow(files, rf1)


def _flip(data, n, seed):
    bad = bytearray(data)
    sos = bytes(bad).index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(bad[sos + 2:sos + 4], "big")
    rng = np.random.Generator(np.random.PCG64(seed))
    for p in rng.integers(start + 4, len(bad) - 8, n):
        if bad[p] != 0xFF and bad[p - 1] != 0xFF and bad[p + 1] != 0xFF:
            bad[p] = (bad[p] ^ 0x5A) if (bad[p] ^ 0x5A) != 0xFF else 0x11
    return bytes(bad)


def _truncate_scan(data, keep):
    """Drop the tail of the entropy bytes of a file without restart markers (EOI stays): its one interval runs out of data."""
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    end = data.rindex(b"\xff\xd9")
    cut = start + int((end - start) * keep)
    while data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + data[end:]


def _damaged_files():
    from test_jpeg_host_cpu import _cut_interval
    good = [_jpeg(_sin_noise(576, 720, s), 2, 90, False, None) for s in range(2)] + [_jpeg(_content(96, 128, 2), 1, 90, False, None)]
    return [good[0], _flip(_jpeg(_sin_noise(576, 720, 7), 2, 90, False, None), 40, 11), good[1],
            _flip(_jpeg(_endo_like(576, 720, 8), 0, 90, True, None), 5, 12),
            _truncate_scan(_jpeg(_sin_noise(576, 720, 9), 2, 90, False, None), 0.6),
            _cut_interval(_jpeg(_sin_noise(576, 720, 10), 2, 90, False, "row"), 1), good[2],
            _cut_interval(_jpeg(_content(64, 80, 1), 2, 90, False, "row"), 1),
            _cut_interval(_jpeg(_sin_noise(300, 400, 3), "L", 90, False, "row"), 2, keep=0.9),
            _truncate_scan(_jpeg(_endo_like(576, 720, 11), "L", 90, False, None), 0.97)]


def test_damaged_streams_equal_the_interval_decoder():
    """Where Pillow is no oracle (test_gpu_jpeg_decode explains why) the one-lane-per-interval decoder is: bytes flipped inside the
    entropy data of multi-workgroup frames without restart markers, intervals cut short (of one workgroup and of many).  Two calls
    give the same bytes, a fresh decoder whose every buffer holds random bytes gives the same bytes, and the undamaged frames are
    exact."""
    from ssl4polyp_amd.data import DeviceJpegDecoder
    from ssl4polyp_amd.jpeg import parse_jpeg
    files = _damaged_files()
    for f in files:
        parse_jpeg(f)   # all on the device
    ref, jb, _ = _decode(files, mode="interval")
    want = ref.data.clone()
    dec = DeviceJpegDecoder(DEV, mode="parallel")
    rf1, _, _ = _decode(files, dec)
    assert torch.equal(rf1.data, want)
    print("stats", dec.stats())
    rf2, _, _ = _decode(files, dec)
    assert torch.equal(rf2.data, want)
    lib_need = ctypes.c_size_t(0)
    from ssl4polyp_amd import _lib
    assert _lib.load().pm_jpeg_decode_workspace(jb.intervals.shape[0], jb.meta["n_subseq"], ctypes.byref(lib_need)) == 0
    fresh = DeviceJpegDecoder(DEV, mode="parallel")
    for name, n, dt in (("coef", jb.meta["blocks"] * 64, torch.int16), ("planes", jb.meta["blocks"] * 64, torch.uint8),
                        ("out", jb.meta["nbytes"], torch.uint8), ("workspace", lib_need.value, torch.uint8)):
        fresh._scratch.bufs[name] = torch.randint(0, 256, (n,), device=DEV).to(dt)
    rf3, _, _ = _decode(files, fresh)
    assert torch.equal(rf3.data, want)
    for b in (0, 2, 6):
        assert torch.equal(rf3.frame(b).cpu(), torch.from_numpy(_pil(files[b]).copy()))
    # sync_rounds=0 sends the long intervals down the sequential way out: the same bytes again
    rf4, _, dec0 = _decode(files, sync_rounds=0)
    assert torch.equal(rf4.data, want) and dec0.stats()["sequential_intervals"] > 0


def test_c_entry_refuses_bad_arguments():
    from ssl4polyp_amd import _lib
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    assert lib.pm_jpeg_decode_workspace(1, 300, ctypes.byref(need)) == 0 and need.value > 300 * 24
    assert lib.pm_jpeg_decode_workspace(-1, 0, ctypes.byref(need)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode_workspace(1, 1, None) == _lib.PM_EINVAL
    assert lib.pm_jpeg_decode_workspace(1, 1, ctypes.byref(need)) == 0
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(need.value + 16, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    p = buf.data_ptr()

    def args(**kw):
        return [p, kw.get("eb", 64), p, 1, p, kw.get("nf", 1), p, 1, p, 1, None, 0, None, kw.get("nfb", 0), p, p, 0, 0, p, 64,
                kw.get("sub", p), kw.get("ns", 1), kw.get("rounds", 2), kw.get("ws", ws.data_ptr()), kw.get("wsb", need.value), None, st]
    assert lib.pm_jpeg_decode_parallel(*args(eb=60)) == _lib.PM_EALIGN
    assert lib.pm_jpeg_decode_parallel(*args(ws=ws.data_ptr() + 4)) == _lib.PM_EALIGN
    assert lib.pm_jpeg_decode_parallel(*args(nf=-1)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode_parallel(*args(ns=-1)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode_parallel(*args(rounds=-1)) == _lib.PM_ESHAPE
    assert lib.pm_jpeg_decode_parallel(*args(nfb=1)) == _lib.PM_EINVAL   # a fallback row without its table
    assert lib.pm_jpeg_decode_parallel(*args(sub=None)) == _lib.PM_EINVAL   # subsequences without their table
    assert lib.pm_jpeg_decode_parallel(*args(ws=None)) == _lib.PM_EINVAL
    assert lib.pm_jpeg_decode_parallel(*args(wsb=need.value - 1)) == _lib.PM_EINVAL   # smaller than the query
    assert lib.pm_jpeg_decode_parallel(*args(nf=0)) == 0
    torch.cuda.synchronize()


def test_no_subsequences_with_frames_present():
    """A batch whose frames are all decoded on the host: n_subseq = 0, the call copies them into their slots."""
    import io
    from PIL import Image
    png = io.BytesIO()
    Image.fromarray(_content(20, 30, 1)).save(png, format="PNG")
    files = [png.getvalue(), _jpeg(_content(45, 61, 0), 0, 75, False, None, progressive=True)]
    rf, jb, dec = _decode(files, mode="parallel")
    assert jb.meta["n_subseq"] == 0 and jb.meta["fallback"] == [0, 1]
    _assert_equal_to_pillow(files, rf)
    assert dec.stats()["subsequences"] == 0 and dec.stats()["sequential_intervals"] == 0


def _folder(root):
    """Files large enough to span workgroups, two sizes, without restart markers and with; one progressive file."""
    d = os.path.join(root, "unlabelled")
    os.makedirs(d)
    for k in range(12):
        H, W = ((576, 720), (480, 640))[k % 2]
        img = _endo_like(H, W, k) if k % 3 == 0 else _sin_noise(H, W, k)
        data = _jpeg(img, (2, 0, "L")[k % 3], (90, 75)[k % 2], bool(k % 2), (None, None, "row")[k % 3])
        with open(os.path.join(d, f"{k:03d}.jpg"), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "prog.jpg"), "wb") as f:
        f.write(_jpeg(_content(100, 140, 50), 2, 85, False, None, progressive=True))
    return root


@pytest.mark.parametrize("transform", ["mae", "train"])
def test_prefetcher_device_decode_equals_host_decode(tmp_path, transform):
    from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher
    from ssl4polyp_amd.folder import folder_loader
    root = _folder(str(tmp_path))

    def run(decode):
        ld = folder_loader(root, batch_size=4, world=1, rank=0, seed=0, num_workers=2, pin_memory=True, decode=decode)
        ld.sampler.set_epoch(0)
        pf = DevicePrefetcher(ld, DEV, augment=DeviceAugmenter(DEV), transform=transform, generator=torch.Generator().manual_seed(3))
        out = [(x.clone(), y.clone()) for x, y in pf]
        return out, pf
    (host, _), (dev, pf) = run("host"), run("device")
    assert len(host) == len(dev) == 13 // 4
    for (a, la), (b, lb) in zip(host, dev):
        assert torch.equal(la, lb) and torch.equal(a, b)
    st = pf._decoder.stats()
    assert pf._decoder.mode == "parallel" and st["subsequences"] > 256
