"""Baseline JPEG decoding, host half (ssl4polyp_amd.jpeg), without a GPU: the marker parser against Pillow's own reading of the same
files, the routing between the device decoder and the host fallback, the unstuffed restart intervals, the packed JpegBatch (pickle,
pin_memory, a spawned worker), and a NumPy restatement of the device stages (entropy decode through the derived tables, islow
IDCT, fancy upsampling, colour) held to Pillow byte for byte, so that a kernel failure can be located to a stage."""
import io
import os
import pickle

import numpy as np
import pytest
import torch


def _img(h, w, seed, kind="mixed"):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([(xx * 7 + yy * 3 + 60 * c) % 256 for c in range(3)], -1).astype(np.float64)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (30, 200, 90), dtype=np.uint8)
    return np.clip(grad + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def _jpeg(arr, mode=None, **kw) -> bytes:
    from PIL import Image
    im = Image.fromarray(arr)
    if mode is not None:
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, format="JPEG", **kw)
    return b.getvalue()


def _png(arr) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _pil(data) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


CASES = [{}, {"subsampling": 0}, {"subsampling": 1}, {"subsampling": 2, "quality": 100}, {"quality": 1}, {"optimize": True},
         {"restart_marker_blocks": 1}, {"restart_marker_rows": 1, "subsampling": 1}, {"mode": "L", "restart_marker_blocks": 2}]


@pytest.mark.parametrize("kw", CASES)
def test_parser_reports_what_pillow_reads(kw):
    from PIL import Image, JpegImagePlugin
    from ssl4polyp_amd.jpeg import parse_jpeg
    for h, w in ((1, 1), (7, 13), (17, 31), (40, 24)):
        data = _jpeg(_img(h, w, 1), **kw)
        hd = parse_jpeg(data)
        im = Image.open(io.BytesIO(data))
        assert (hd.width, hd.height) == im.size and hd.mode == im.mode
        assert hd.sampling == JpegImagePlugin.get_sampling(im)
        assert {k: list(v) for k, v in hd.quant.items()} == {k: list(v) for k, v in im.quantization.items()}
        mcu_w = 8 * hd.hs
        if "restart_marker_blocks" in kw:
            assert hd.restart_interval == kw["restart_marker_blocks"]
        elif "restart_marker_rows" in kw:
            assert hd.restart_interval == kw["restart_marker_rows"] * -(-w // mcu_w)
        else:
            assert hd.restart_interval == 0
        assert hd.n_intervals == (-(-hd.n_mcus // hd.restart_interval) if hd.restart_interval else 1)


def test_routing_between_device_and_host():
    from PIL import Image
    from ssl4polyp_amd.jpeg import JpegFallback, parse_jpeg
    rgb = _img(40, 56, 2)
    device = [_jpeg(rgb), _jpeg(rgb, subsampling=0), _jpeg(rgb, subsampling=1), _jpeg(rgb, subsampling=2), _jpeg(rgb, mode="L"),
              _jpeg(rgb, optimize=True), _jpeg(rgb, restart_marker_blocks=1), _jpeg(rgb, restart_marker_rows=1)]
    for d in device:
        parse_jpeg(d)
    good = _jpeg(rgb)
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, format="JPEG")
    host = {"progressive": _jpeg(rgb, progressive=True), "cmyk": b.getvalue(), "png": _png(rgb), "truncated": good[:len(good) // 2],
            "no EOI": good[:-2], "empty": b"", "text": b"not an image at all"}
    for name, d in host.items():
        with pytest.raises(JpegFallback):
            parse_jpeg(d)
        if name in ("progressive", "cmyk", "png"):
            assert _pil(d).shape == (40, 56, 3)


@pytest.mark.parametrize("kw", [{"restart_marker_blocks": 3}, {"restart_marker_rows": 1}, {}])
def test_unstuffed_intervals_restuff_to_the_scan(kw):
    from ssl4polyp_amd.jpeg import parse_jpeg
    data = _jpeg(_img(48, 72, 3, "noise"), quality=100, subsampling=2, **kw)   # noise at q100: many 0xFF bytes to stuff
    hd = parse_jpeg(data)
    sos = data.index(b"\xff\xda")
    scan = data[sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"):len(data) - 2]
    assert data[-2:] == b"\xff\xd9" and b"\xff\x00" in scan
    parts = []
    for k in range(hd.n_intervals):
        parts.append(bytes(hd.data[hd.starts[k]:hd.starts[k] + hd.lengths[k]]).replace(b"\xff", b"\xff\x00"))
        if k < hd.n_intervals - 1:
            parts.append(bytes([0xFF, 0xD0 + k % 8]))
    assert b"".join(parts) == scan
    ri = hd.restart_interval or hd.n_mcus
    assert hd.n_intervals == -(-hd.n_mcus // ri)


def _files():
    rgb = _img(30, 44, 4)
    return [_jpeg(rgb, subsampling=2), _jpeg(_img(9, 17, 5), mode="L"), _png(_img(12, 10, 6)), _jpeg(rgb, progressive=True),
            _jpeg(_img(33, 17, 7), subsampling=1, restart_marker_blocks=1), _jpeg(rgb, subsampling=2, quality=60)]


def test_jpeg_batch_packing_pickle_and_pin():
    from ssl4polyp_amd.data import RaggedFrames
    from ssl4polyp_amd.jpeg import INTERVAL_WORDS, JpegBatch, parse_jpeg
    files = _files()
    jb = JpegBatch.from_bytes(files)
    want = RaggedFrames.from_frames([_pil(f) for f in files])
    assert len(jb) == 6 and not jb.is_cuda
    assert torch.equal(jb.offset, want.offset) and torch.equal(jb.hw, want.hw)
    assert jb.meta["fallback"] == [2, 3] and jb.meta["nbytes"] == want.data.numel()
    for k, b in enumerate(jb.meta["fallback"]):
        s, o, n = jb.fallback_table[k].tolist()
        assert o == want.offsets[b] and np.array_equal(jb.fallback[s:s + n].numpy(), want.frame(b).numpy().reshape(-1))
    # intervals: longest first, word-aligned, every MCU of every device frame exactly once
    iv = jb.intervals.numpy()
    assert iv.shape[1] == INTERVAL_WORDS and (np.diff(iv[:, 2]) <= 0).all()
    assert jb.entropy.numel() % 16 == 0 and (iv[:, 1] % 4 == 0).all() and (iv[:, 1] * 4 + iv[:, 2] <= jb.entropy.numel()).all()
    heads = [parse_jpeg(files[b]) for b in (0, 1, 4, 5)]
    for f, hd in enumerate(heads):
        mine = iv[iv[:, 0] == f]
        mine = mine[np.argsort(mine[:, 3])]
        assert mine[:, 4].sum() == hd.n_mcus and (mine[1:, 3] == mine[:-1, 3] + mine[:-1, 4]).all()
        for row in mine:
            k = int(np.flatnonzero(hd.starts == hd.starts[row[3] // (hd.restart_interval or hd.n_mcus)])[0])
            got = jb.entropy[row[1] * 4:row[1] * 4 + row[2]].numpy()
            assert np.array_equal(got, hd.data[hd.starts[k]:hd.starts[k] + hd.lengths[k]])
    # frames 0 and 5 come from one encoder and quality -> shared Huffman tables; 0 / 5 have different quantisation tables
    fr = jb.frames.numpy()
    assert (fr[0, 8:14] == fr[3, 8:14]).all() and not (fr[0, 14:17] == fr[3, 14:17]).all()
    assert jb.huff.shape[1] == 1024 and jb.huff.shape[0] <= 8 and jb.quant.shape[1] == 64
    assert fr[:, 17].tolist() == sorted(fr[:, 17].tolist()) and fr[1, 2] == 1
    back = pickle.loads(pickle.dumps(jb))
    assert all(torch.equal(back.t[k], jb.t[k]) for k in JpegBatch.TENSORS) and back.meta["fallback"] == [2, 3]
    if torch.cuda.is_available():
        pinned = jb.pin_memory()
        assert pinned.is_pinned() and all(torch.equal(pinned.t[k], jb.t[k]) for k in JpegBatch.TENSORS)


def test_jpeg_collate_in_a_spawned_worker(tmp_path):
    from ssl4polyp_amd.folder import ImageFolderFrames, folder_loader
    from ssl4polyp_amd.jpeg import JpegBatch
    d = tmp_path / "root" / "cls"
    d.mkdir(parents=True)
    for i, f in enumerate(_files()):
        (d / f"{i:02d}.jpg").write_bytes(f)
    with pytest.raises(ValueError):
        ImageFolderFrames(str(tmp_path / "root"), decode="gpu")
    ld = folder_loader(str(tmp_path / "root"), batch_size=3, num_workers=1, pin_memory=False, decode="device")
    ld.sampler.set_epoch(0)
    order = list(iter(ld.sampler))
    batches = list(ld)
    assert len(batches) == 2
    for i, (jb, labels) in enumerate(batches):
        assert isinstance(jb, JpegBatch) and labels.tolist() == [0, 0, 0]
        ref = JpegBatch.from_bytes([ld.dataset[j][0] for j in order[3 * i:3 * i + 3]])
        assert all(torch.equal(jb.t[k], ref.t[k]) for k in JpegBatch.TENSORS)


# ---------------------------------------------------------------------------------------------------------------------------
# the device stages restated in NumPy (the kernels' integer arithmetic, one stage per function)
# ---------------------------------------------------------------------------------------------------------------------------
def _entropy_decode(hd):
    """pm_jpeg.hip jpeg_huff_kernel through the derived records: coefficient planes [component] -> int64 [bh, bw, 64]."""
    from ssl4polyp_amd.jpeg import NATURAL_ORDER, derive_huffman
    tabs = {}
    for (kind, t), (bits, vals) in hd.tables.items():
        r = derive_huffman(bits, vals, kind == "dc")
        tabs[(kind, t)] = (r[0:512].view(np.uint16), r[512:584].view(np.int32), r[584:656].view(np.int32), r[656:912])
    samp = [(hd.hs, hd.vs)] + [(1, 1)] * (hd.ncomp - 1)
    coef = [np.zeros((hd.mcuy * v, hd.mcux * h, 64), dtype=np.int64) for h, v in samp]
    ri = hd.restart_interval or hd.n_mcus
    for k in range(hd.n_intervals):
        seg = bytes(hd.data[hd.starts[k]:hd.starts[k] + hd.lengths[k]]) + bytes(64)
        val, total = int.from_bytes(seg, "big"), 8 * len(seg)
        pos = [0]

        def peek(n):
            return (val >> (total - pos[0] - n)) & ((1 << n) - 1)

        def decode(t):
            look, maxcode, valoffset, huffval = t
            e = int(look[peek(8)])
            nb, sym = e >> 8, e & 0xFF
            if nb > 8:
                nb = 9
                while nb <= 16 and peek(nb) > maxcode[nb]:
                    nb += 1
                sym = 0 if nb > 16 else int(huffval[(peek(nb) + valoffset[nb]) & 0xFF])
            pos[0] += nb
            return sym

        def extend(s):
            r = peek(s)
            pos[0] += s
            return r - (1 << s) + 1 if r < (1 << (s - 1)) else r

        pred = [0] * hd.ncomp
        for m in range(k * ri, min((k + 1) * ri, hd.n_mcus)):
            my, mx = divmod(m, hd.mcux)
            for c, (h, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(h):
                        blk = coef[c][my * v + by, mx * h + bx]
                        s = decode(tabs[("dc", hd.dc_ids[c])])
                        pred[c] += extend(s) if s else 0
                        blk[0] = pred[c]
                        kk = 1
                        while kk < 64:
                            sym = decode(tabs[("ac", hd.ac_ids[c])])
                            r, s = sym >> 4, sym & 15
                            if s:
                                kk += r
                                blk[NATURAL_ORDER[kk]] = extend(s)
                            elif r != 15:
                                break
                            else:
                                kk += 15
                            kk += 1
            if pos[0] > 8 * hd.lengths[k]:   # read past the data: the interval's later MCUs stay zero (insufficient_data)
                break
    return coef


def _jidct8(c, first):
    """jidctint.c one pass along the last axis (int64, as the kernel's int32 never overflows on valid data)."""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * 4433
    e2, e3 = z1 + z3 * -15137, z1 + z2 * 6270
    e0, e1 = (c[..., 0] + c[..., 4]) << 13, (c[..., 0] - c[..., 4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 * 2446 + z1 + z3, o1 * 16819 + z2 + z4, o2 * 25172 + z2 + z3, o3 * 12299 + z1 + z4
    sh = 11 if first else 18
    d = lambda x: (x + (1 << (sh - 1))) >> sh
    return np.stack([d(t10 + o3), d(t11 + o2), d(t12 + o1), d(t13 + o0), d(t13 - o0), d(t12 - o1), d(t11 - o2), d(t10 - o3)], -1)


def _idct_planes(hd, coef):
    """jpeg_idct_kernel: dequantise, islow IDCT, range limit -> uint8 planes [bh * 8, bw * 8]."""
    planes = []
    for c, q in enumerate(coef):
        bh, bw, _ = q.shape
        qt = hd.quant[hd.qt_ids[c]].astype(np.uint16).view(np.int16).astype(np.int64)
        v = (q * qt).reshape(bh, bw, 8, 8)
        v = _jidct8(v.swapaxes(-1, -2), True).swapaxes(-1, -2)
        v = _jidct8(v, False)
        v = np.clip(v + 128, 0, 255)
        planes.append(v.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes


def _colour(hd, planes):
    """jpeg_color_kernel: fancy upsampling (jdsample.c) + jdcolor.c -> uint8 [H, W, 3]."""
    H, W = hd.height, hd.width
    Y = planes[0][:H, :W]
    if hd.ncomp == 1:
        return np.repeat(Y[..., None], 3, -1).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    dw, dh = -(-W // hd.hs), -(-H // hd.vs)

    def up(p):
        if hd.hs == 1:
            return p[y, x]
        i, odd = x >> 1, (x & 1).astype(bool)
        if dw <= 2:
            return p[y >> (hd.vs - 1), i]
        i2 = np.where(odd, np.minimum(i + 1, dw - 1), np.maximum(i - 1, 0))
        if hd.vs == 1:
            return (3 * p[y, i] + p[y, i2] + np.where(odd, 2, 1)) >> 2
        r = y >> 1
        r2 = np.where(y & 1, np.minimum(r + 1, dh - 1), np.maximum(r - 1, 0))
        s1, s2 = 3 * p[r, i] + p[r2, i], 3 * p[r, i2] + p[r2, i2]
        return (3 * s1 + s2 + np.where(odd, 7, 8)) >> 4

    cb, cr = up(planes[1]) - 128, up(planes[2]) - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("mode", [0, 1, 2, "L"])
def test_numpy_restatement_of_the_device_stages_equals_pillow(mode):
    """The three device stages, restated, on tiny frames of every supported layout: widths 1-5 (fancy upsampling only where the
    downsampled width exceeds 2), odd sizes, restart intervals, optimized tables, flat blocks (long zero runs / EOB) and
    saturated colours -- equal to Pillow byte for byte."""
    from ssl4polyp_amd.jpeg import parse_jpeg
    kw = {"mode": "L"} if mode == "L" else {"subsampling": mode}
    sizes = [(h, w) for h in (1, 2, 3, 5) for w in (1, 2, 3, 4, 5)] + [(7, 13), (17, 31), (33, 17)]
    for n, (h, w) in enumerate(sizes):
        for q, extra, kind in ((90, {}, "mixed"), (100, {"restart_marker_blocks": 1}, "noise"), (50, {"optimize": True}, "flat"),
                               (1, {"restart_marker_rows": 1}, "mixed")):
            data = _jpeg(_img(h, w, n, kind), quality=q, **kw, **extra)
            hd = parse_jpeg(data)
            got = _colour(hd, _idct_planes(hd, _entropy_decode(hd)))
            assert np.array_equal(got, _pil(data)), (h, w, q, extra, kind)


def _rebuild(data, drop_app0=False, app0_trunc=False, adobe=None, dqt16=False, ids=None):
    """Rewrite the header segments of a Pillow JPEG: drop or truncate the JFIF APP0, add an Adobe APP14 with a transform, re-store
    the quantisation tables with 16-bit precision, change the component ids."""
    out = bytearray(data[:2])
    if adobe is not None:
        out += b"\xff\xee" + (14).to_bytes(2, "big") + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, adobe])
    p = 2
    while True:
        m, ln = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        seg = bytearray(data[p + 4:p + 2 + ln])
        p += 2 + ln
        if m == 0xE0 and drop_app0:
            continue
        if m == 0xE0 and app0_trunc:
            seg = seg[:12]   # (libjpeg needs 14 bytes to see JFIF; Pillow reads 12)
        if m == 0xDB and dqt16:
            new, q = bytearray(), 0
            while q < len(seg):
                new += bytes([0x10 | (seg[q] & 15)]) + b"".join(int(v).to_bytes(2, "big") for v in seg[q + 1:q + 65])
                q += 65
            seg = new
        if m in (0xC0, 0xC1) and ids:
            for i in range(seg[5]):
                seg[6 + 3 * i] = ids[i]
        if m == 0xDA and ids:
            for i in range(seg[0]):
                seg[1 + 2 * i] = ids[i]
        out += bytes([0xFF, m]) + (len(seg) + 2).to_bytes(2, "big") + bytes(seg)
        if m == 0xDA:
            return bytes(out + data[p:])


def _cut_interval(data, k, keep=0.5):
    """Drop the second half of restart interval k's entropy bytes (structure intact: the RST markers stay in sequence)."""
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    marks = [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    a, b = marks[k - 1] + 2, marks[k]
    cut = a + int((b - a) * keep)
    cut -= data[cut - 1] == 0xFF   # (never split a stuffed 0xFF 0x00)
    return data[:cut] + data[b:]


def test_parser_branches_follow_libjpeg():
    """16-bit DQT, Adobe APP14 transform 1 / 0, 'R','G','B' component ids, a JFIF APP0 too short for libjpeg (examine_app0 needs
    14 bytes): routed as libjpeg reads the colour space, and what the device decodes restates Pillow byte for byte."""
    from PIL import Image
    from ssl4polyp_amd.jpeg import JpegFallback, parse_jpeg
    base = _jpeg(_img(19, 27, 8), subsampling=2)
    dev = {"dqt16": _rebuild(base, dqt16=True), "adobe1": _rebuild(base, drop_app0=True, adobe=1),
           "jfif+rgb ids": _rebuild(base, ids=[82, 71, 66]), "adobe1+rgb ids": _rebuild(base, drop_app0=True, adobe=1, ids=[82, 71, 66])}
    for name, d in dev.items():
        hd = parse_jpeg(d)
        im = Image.open(io.BytesIO(d))
        assert {k: list(v) for k, v in hd.quant.items()} == {k: list(v) for k, v in im.quantization.items()}, name
        assert np.array_equal(_colour(hd, _idct_planes(hd, _entropy_decode(hd))), _pil(d)), name
    host = {"adobe0": _rebuild(base, drop_app0=True, adobe=0), "rgb ids": _rebuild(base, drop_app0=True, ids=[82, 71, 66]),
            "short JFIF + adobe0": _rebuild(base, app0_trunc=True, adobe=0)}
    for name, d in host.items():
        with pytest.raises(JpegFallback):
            parse_jpeg(d)
        assert _pil(d).shape == (19, 27, 3), name


def test_long_code_search_equals_jpeg_huff_decode():
    """The device's one-step search for codes over 8 bits (limits of lengths 9..16) against jpeg_huff_decode's bit-by-bit loop,
    for every 16-bit prefix the lookahead table misses, on standard and optimized tables."""
    from ssl4polyp_amd.jpeg import derive_huffman, parse_jpeg
    tables = set()
    for kw in ({}, {"optimize": True}, {"optimize": True, "quality": 100}):
        tables |= {(k[0], *v) for k, v in parse_jpeg(_jpeg(_img(64, 64, 9, "noise"), **kw)).tables.items()}
    p16 = np.arange(1 << 16, dtype=np.int64)
    for kind, bits, vals in tables:
        r = derive_huffman(bits, vals, kind == "dc")
        look, maxcode, valoffset, huffval = r[0:512].view(np.uint16), r[512:584].view(np.int32), r[584:656].view(np.int32), r[656:912]
        limit, voff = r[912:944].view(np.uint32).astype(np.int64), r[944:976].view(np.int32)
        miss = p16[(look[p16 >> 8] >> 8) > 8]
        l_loop = np.full(len(miss), 17)
        for l in range(16, 8, -1):   # the first l with code_l <= maxcode[l]
            l_loop = np.where((miss >> (16 - l)) <= maxcode[l], l, l_loop)
        l_dev = 9 + (miss[:, None] >= limit[None, :]).sum(1)
        assert np.array_equal(l_loop, l_dev)
        ok = l_dev <= 16
        l = l_dev[ok]
        sym_loop = huffval[((miss[ok] >> (16 - l)) + valoffset[l]) & 0xFF]
        sym_dev = huffval[((miss[ok] >> (16 - l)) + voff[l - 9]) & 0xFF]
        assert np.array_equal(sym_loop, sym_dev)


def test_interval_that_runs_out_of_data_stays_grey_as_in_libjpeg():
    """Half of one restart interval's bytes removed: libjpeg reads zero bits to the end of the MCU that ran out, leaves the
    interval's later MCUs zero and resumes at the next RST marker; the restatement (and the kernel's rule) give Pillow's pixels."""
    from ssl4polyp_amd.jpeg import parse_jpeg
    for kw in ({"subsampling": 2}, {"subsampling": 0}, {"mode": "L"}):
        d = _cut_interval(_jpeg(_img(64, 80, 10), restart_marker_rows=1, **kw), 1)
        hd = parse_jpeg(d)
        assert np.array_equal(_colour(hd, _idct_planes(hd, _entropy_decode(hd))), _pil(d)), kw
