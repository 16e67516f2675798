"""Baseline JPEG for the device decoder: the host half (csrc/pm_jpeg.hip is the device half).

DataLoader workers read the files and pack them; nothing here touches the GPU.  `parse_jpeg` walks the markers of one file (SOI,
APPn / COM skipped, DQT, SOF0 / SOF1, DHT, DRI, SOS, EOI) and decides whether the device can decode it bit for bit as Pillow's
libjpeg-turbo does: 8-bit Huffman-coded sequential, one scan with Ss=0 / Se=63 / Ah=Al=0, one component (grey) or three YCbCr
components with luma sampling (1,1), (2,1) or (2,2) and chroma (1,1), any restart interval.  Everything else -- progressive,
arithmetic, 12-bit, CMYK / YCCK / RGB, multi-scan, other samplings, a missing EOI, any structural error, files that are not JPEG --
raises `JpegFallback`, and the packer decodes that file here exactly as folder.pil_loader does.

`JpegBatch.from_bytes` packs a batch: the entropy data of every device frame with its byte stuffing removed, split at its RSTn
markers into restart intervals that each start on a 16-byte boundary (one row per interval: frame, word offset, byte length, first
MCU, MCU count; sorted by length so that the lanes of a wave finish together), one row per device frame, the Huffman tables of the
batch (deduplicated, derived as jdhuff.c jpeg_make_d_derived_tbl does), its quantisation tables (deduplicated, natural order), the
predecoded RGB bytes of the fallback frames, and the offset / size tables of the decoded `RaggedFrames` (packed back to back
exactly as `RaggedFrames.from_frames` packs them).  For the decoding in parallel inside an interval (pm_jpeg_decode_parallel) every
interval is cut from its start into ceil(length / SUBSEQ_BYTES) subsequences, numbered through the sorted rows: word 5 of a row is
its first subsequence, and `subseq` names the row of every subsequence.
"""
from __future__ import annotations

import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# jutils.c jpeg_natural_order: zigzag index -> natural index, 16 extra entries of 63 so that a corrupt run stays inside its block
NATURAL_ORDER = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
                          53, 60, 61, 54, 47, 55, 62, 63] + [63] * 16, dtype=np.int32)

HUFF_RECORD = 1024   # bytes per derived Huffman table (pm_jpeg.hip HuffTable)
FRAME_WORDS = 32     # int32 words per frame row (pm_jpeg.hip kFrameWords)
INTERVAL_WORDS = 8   # int32 words per interval row (pm_jpeg.hip kIntervalWords)
SUBSEQ_BYTES = 128   # bytes per subsequence of an interval, one lane each in the parallel entropy stage (pm_jpeg.hip kSubBytes)


class JpegFallback(Exception):
    """The file is decoded on the host (the message says why)."""


class JpegHeader:
    """What parse_jpeg found in a file the device decodes: size, components, sampling, tables, restart interval, and the scan's
    unstuffed bytes `data` with its restart intervals (`starts`, `lengths`, byte positions in `data`)."""
    __slots__ = ("height", "width", "ncomp", "comp_ids", "hs", "vs", "quant", "qt_ids", "dc_ids", "ac_ids", "tables",
                 "restart_interval", "mcux", "mcuy", "data", "starts", "lengths")

    @property
    def mode(self) -> str:
        return "L" if self.ncomp == 1 else "RGB"

    @property
    def sampling(self) -> int:
        """JpegImagePlugin.get_sampling: 0 / 1 / 2 for 4:4:4 / 4:2:2 / 4:2:0, -1 for greyscale."""
        return -1 if self.ncomp == 1 else {(1, 1): 0, (2, 1): 1, (2, 2): 2}[(self.hs, self.vs)]

    @property
    def n_mcus(self) -> int:
        return self.mcux * self.mcuy

    @property
    def n_intervals(self) -> int:
        return len(self.starts)


def _u16(d, p: int) -> int:
    return (int(d[p]) << 8) | int(d[p + 1])


_DERIVED: Dict[Tuple[bool, bytes, bytes], np.ndarray] = {}


def derive_huffman(bits: bytes, vals: bytes, is_dc: bool) -> np.ndarray:
    """jdhuff.c jpeg_make_d_derived_tbl for one table -> its 1024-byte device record: uint16 lookup[256] (code length << 8 | symbol
    for the codes of at most 8 bits, 9 << 8 where the code is longer), int32 maxcode[18], int32 valoffset[18], uint8 huffval[256],
    then for lengths 9..16 uint32 limit[8] and int32 valoffset[8] (the kernel's one-step search for a long code's length).
    bits[l - 1] = number of codes of length l.  Raises JpegFallback where libjpeg raises JERR_BAD_HUFF_TABLE."""
    key = (bool(is_dc), bytes(bits), bytes(vals))
    rec = _DERIVED.get(key)
    if rec is not None:
        return rec
    counts = list(key[1])
    nsym = sum(counts)
    if len(counts) != 16 or nsym > 256 or len(key[2]) < nsym:
        raise JpegFallback("bad Huffman table")
    huffval = np.zeros(256, dtype=np.uint8)
    huffval[:nsym] = np.frombuffer(key[2][:nsym], dtype=np.uint8)
    huffsize = [l + 1 for l in range(16) for _ in range(counts[l])]
    huffcode: List[int] = []
    code, p = 0, 0
    si = huffsize[0] if huffsize else 0
    while p < nsym:   # Figure C.2
        while p < nsym and huffsize[p] == si:
            huffcode.append(code)
            code += 1
            p += 1
        if code >= (1 << si):
            raise JpegFallback("bad Huffman table")
        code <<= 1
        si += 1
    maxcode = np.full(18, -1, dtype=np.int32)
    valoffset = np.zeros(18, dtype=np.int32)
    p = 0
    for l in range(1, 17):   # Figure F.15
        if counts[l - 1]:
            valoffset[l] = p - huffcode[p]
            p += counts[l - 1]
            maxcode[l] = huffcode[p - 1]
    maxcode[17] = 0xFFFFF
    lookup = np.full(256, 9 << 8, dtype=np.uint16)
    p = 0
    for l in range(1, 9):
        for _ in range(counts[l - 1]):
            lb = huffcode[p] << (8 - l)
            lookup[lb:lb + (1 << (8 - l))] = (l << 8) | int(huffval[p])
            p += 1
    if is_dc and (huffval[:nsym] > 15).any():
        raise JpegFallback("bad DC Huffman table")
    # codes over 8 bits: per length 9..16 the left-justified limit (maxcode + 1) << (16 - l), carried over lengths without codes
    # so that the limits never decrease (the first l with peek16 < limit[l] is where jpeg_huff_decode stops)
    limit = np.zeros(8, dtype=np.uint32)
    lim = 0
    for l in range(1, 17):
        if counts[l - 1]:
            lim = (int(maxcode[l]) + 1) << (16 - l)
        if l >= 9:
            limit[l - 9] = lim
    rec = np.zeros(HUFF_RECORD, dtype=np.uint8)
    rec[0:512] = lookup.view(np.uint8)
    rec[512:584] = maxcode.view(np.uint8)
    rec[584:656] = valoffset.view(np.uint8)
    rec[656:912] = huffval
    rec[912:944] = limit.view(np.uint8)
    rec[944:976] = valoffset[9:17].view(np.uint8)
    if len(_DERIVED) > 4096:
        _DERIVED.clear()
    _DERIVED[key] = rec
    return rec


def _unstuff_scan(d: np.ndarray, pos: int, restart_interval: int, n_mcus: int):
    """The entropy-coded segment that starts at `pos` -> (unstuffed bytes, interval starts, interval lengths, position of the
    marker that ends the scan).  0xFF 0x00 -> 0xFF; the scan is split at its RSTn markers, which must come in sequence, one
    between every two restart intervals."""
    s = d[pos:]
    ff = np.flatnonzero(s[:-1] == 0xFF)
    nxt = s[ff + 1]
    term = np.flatnonzero((nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)))
    if len(term) == 0:
        raise JpegFallback("no marker after the scan")
    end = int(ff[term[0]])
    ff, nxt = ff[:term[0]], nxt[:term[0]]
    is_rst = nxt != 0
    rst = ff[is_rst]
    n_iv = -(-n_mcus // restart_interval) if restart_interval > 0 else 1
    if len(rst) != n_iv - 1:
        raise JpegFallback("restart markers do not match the restart interval")
    if len(rst) and not np.array_equal(nxt[is_rst].astype(np.int64) - 0xD0, np.arange(len(rst)) % 8):
        raise JpegFallback("restart markers out of sequence")
    keep = np.ones(end, dtype=bool)
    keep[ff[~is_rst] + 1] = False
    keep[rst] = False
    keep[rst + 1] = False
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    bounds = np.concatenate([[0], kept_before[rst], [kept_before[end]]]).astype(np.int64)
    return s[:end][keep], bounds[:-1], np.diff(bounds), pos + end


def parse_jpeg(data) -> JpegHeader:
    """Walk the markers of one file.  Returns the header of a file the device decodes; raises JpegFallback otherwise."""
    d = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegFallback("not a JPEG file")
    qt: Dict[int, np.ndarray] = {}
    ht: Dict[Tuple[int, int], Tuple[bytes, bytes]] = {}
    h = JpegHeader()
    h.restart_interval = 0
    sof = None
    jfif, adobe_transform = False, None
    scanned = False
    p = 2
    try:
        while True:
            if p >= n or d[p] != 0xFF:
                raise JpegFallback("marker expected")
            while p < n and d[p] == 0xFF:   # fill bytes
                p += 1
            if p >= n:
                raise JpegFallback("truncated")
            m = int(d[p])
            p += 1
            if m == 0xD9:   # EOI
                break
            if m in (0x00, 0x01) or 0xD0 <= m <= 0xD8:
                raise JpegFallback(f"unexpected marker 0x{m:02X}")
            if p + 2 > n:
                raise JpegFallback("truncated")
            ln = _u16(d, p)
            if ln < 2 or p + ln > n:
                raise JpegFallback("truncated segment")
            seg = d[p + 2:p + ln]
            p += ln
            if 0xE0 <= m <= 0xEF or m == 0xFE:   # APPn, COM
                if m == 0xE0 and len(seg) >= 14 and bytes(seg[:5]) == b"JFIF\0":   # (jdmarker.c examine_app0)
                    jfif = True
                if m == 0xEE and len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
                    adobe_transform = int(seg[11])
                continue
            if m == 0xDB:   # DQT
                q = 0
                while q < len(seg):
                    pq, tq = int(seg[q]) >> 4, int(seg[q]) & 15
                    if pq > 1 or tq > 3 or q + 1 + 64 * (pq + 1) > len(seg):
                        raise JpegFallback("bad DQT")
                    raw = seg[q + 1:q + 1 + 64 * (pq + 1)]
                    vals = raw.astype(np.int64) if pq == 0 else (raw[0::2].astype(np.int64) << 8) | raw[1::2]
                    nat = np.zeros(64, dtype=np.int64)
                    nat[NATURAL_ORDER[:64]] = vals
                    qt[tq] = nat
                    q += 1 + 64 * (pq + 1)
                continue
            if m == 0xC4:   # DHT
                q = 0
                while q < len(seg):
                    tc, th = int(seg[q]) >> 4, int(seg[q]) & 15
                    if tc > 1 or th > 3 or q + 17 > len(seg):
                        raise JpegFallback("bad DHT")
                    bits = bytes(seg[q + 1:q + 17])
                    cnt = sum(bits)
                    if cnt > 256 or q + 17 + cnt > len(seg):
                        raise JpegFallback("bad DHT")
                    ht[(tc, th)] = (bits, bytes(seg[q + 17:q + 17 + cnt]))
                    q += 17 + cnt
                continue
            if m == 0xDD:   # DRI
                if len(seg) != 2:
                    raise JpegFallback("bad DRI")
                h.restart_interval = _u16(seg, 0)
                continue
            if m in (0xC0, 0xC1):   # SOF0, SOF1
                if sof is not None or len(seg) < 6:
                    raise JpegFallback("bad SOF")
                prec, H, W, nf = int(seg[0]), _u16(seg, 1), _u16(seg, 3), int(seg[5])
                if prec != 8:
                    raise JpegFallback(f"{prec}-bit samples")
                if H == 0 or W == 0 or nf not in (1, 3) or len(seg) != 6 + 3 * nf:
                    raise JpegFallback("unsupported frame header")
                comps = [(int(seg[6 + 3 * i]), int(seg[7 + 3 * i]) >> 4, int(seg[7 + 3 * i]) & 15, int(seg[8 + 3 * i]))
                         for i in range(nf)]
                if len({c[0] for c in comps}) != nf or any(c[3] > 3 or not 1 <= c[1] <= 4 or not 1 <= c[2] <= 4 for c in comps):
                    raise JpegFallback("bad component")
                sof = (H, W, comps)
                continue
            if m == 0xCC:
                raise JpegFallback("arithmetic coding")
            if 0xC2 <= m <= 0xCF and m != 0xC8:
                raise JpegFallback(f"SOF 0x{m:02X}: not sequential Huffman")
            if m == 0xDA:   # SOS
                if sof is None or scanned:
                    raise JpegFallback("multi-scan file" if scanned else "SOS before SOF")
                H, W, comps = sof
                ns = int(seg[0]) if len(seg) else 0
                if len(seg) != 4 + 2 * ns or ns != len(comps):
                    raise JpegFallback("not one interleaved scan of every component")
                ids = [int(seg[1 + 2 * i]) for i in range(ns)]
                if ids != [c[0] for c in comps]:
                    raise JpegFallback("scan component order")
                if int(seg[1 + 2 * ns]) != 0 or int(seg[2 + 2 * ns]) != 63 or int(seg[3 + 2 * ns]) != 0:
                    raise JpegFallback("not a sequential scan")
                h.dc_ids = [int(seg[2 + 2 * i]) >> 4 for i in range(ns)]
                h.ac_ids = [int(seg[2 + 2 * i]) & 15 for i in range(ns)]
                h.height, h.width, h.ncomp, h.comp_ids = H, W, ns, ids
                if ns == 3:   # jdapimin.c default_decompress_parms: which 3-component files are YCbCr
                    if not jfif and (adobe_transform == 0 or (adobe_transform is None and ids == [82, 71, 66])):
                        raise JpegFallback("RGB colour space")
                    if [c[1:3] for c in comps[1:]] != [(1, 1), (1, 1)] or (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)):
                        raise JpegFallback("sampling factors")
                    h.hs, h.vs = comps[0][1], comps[0][2]
                else:         # one component: one block per MCU whatever its factors say
                    h.hs, h.vs = 1, 1
                h.mcux = -(-W // (8 * h.hs))
                h.mcuy = -(-H // (8 * h.vs))
                h.qt_ids = [c[3] for c in comps]
                if any(t not in qt for t in h.qt_ids):
                    raise JpegFallback("missing quantisation table")
                h.quant = {t: qt[t].copy() for t in set(h.qt_ids)}
                if any((0, t) not in ht for t in h.dc_ids) or any((1, t) not in ht for t in h.ac_ids):
                    raise JpegFallback("missing Huffman table")
                h.tables = {("dc", t): ht[(0, t)] for t in set(h.dc_ids)}
                h.tables.update({("ac", t): ht[(1, t)] for t in set(h.ac_ids)})
                for (kind, _), (bits, vals) in h.tables.items():
                    derive_huffman(bits, vals, kind == "dc")
                h.data, h.starts, h.lengths, p = _unstuff_scan(d, p, h.restart_interval, h.n_mcus)
                scanned = True
                continue
            raise JpegFallback(f"marker 0x{m:02X}")
    except (IndexError, ValueError) as e:
        raise JpegFallback(f"structural error: {e}") from None
    if not scanned:
        raise JpegFallback("no scan")
    return h


def host_decode(data: bytes) -> np.ndarray:
    """folder.pil_loader on the bytes of a file: Pillow's decode, converted to RGB, uint8 [H, W, 3]."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


class JpegBatch:
    """A batch of compressed frames for data.DeviceJpegDecoder (see the module docstring).  Tensors, contiguous: entropy uint8
    [16 k], intervals int32 [N, 8], frames int32 [F, 32], huff uint8 [T, 1024], quant int32 [Q, 64], fallback uint8 (the fallback
    frames' RGB bytes), fallback_table int64 [K, 3] (source offset, output offset, bytes), offset int64 [B], hw int32 [B, 2].
    `meta` is the host side: the RaggedFrames tables as numpy (`offset`, `hw`), the coefficient `blocks` and device `pixels` the
    workspace follows, the decoded `nbytes`, the indices of the `fallback` frames and `n_subseq`.  intervals[:, 5] is the row's first
    subsequence (the exclusive scan of ceil(byte length / SUBSEQ_BYTES) over the rows); subseq int32 [n_subseq] is the interval row
    of every subsequence."""
    TENSORS = ("entropy", "intervals", "frames", "huff", "quant", "fallback", "fallback_table", "offset", "hw", "subseq")

    def __init__(self, tensors: Dict[str, torch.Tensor], meta: dict):
        self.t = tensors
        self.meta = meta

    def __getattr__(self, name):
        t = self.__dict__.get("t")
        if t is not None and name in t:
            return t[name]
        raise AttributeError(name)

    def __len__(self) -> int:
        return len(self.meta["offset"])

    @property
    def is_cuda(self) -> bool:
        return self.t["entropy"].is_cuda

    def is_pinned(self) -> bool:
        return all(v.is_pinned() for v in self.t.values())

    def pin_memory(self, device=None) -> "JpegBatch":
        """(called by DataLoader(pin_memory=True) in its pin thread)"""
        return JpegBatch({k: v.pin_memory() for k, v in self.t.items()}, self.meta)

    def to(self, device, non_blocking: bool = False) -> "JpegBatch":
        return JpegBatch({k: v.to(device, non_blocking=non_blocking) for k, v in self.t.items()}, self.meta)

    @classmethod
    def from_bytes(cls, files: Sequence[bytes]) -> "JpegBatch":
        """Pack the contents of B files of any format (what the device cannot decode is decoded here)."""
        if not len(files):
            raise ValueError("JpegBatch.from_bytes takes a non-empty sequence of files")
        heads: List[Optional[JpegHeader]] = []
        fb_frames: Dict[int, np.ndarray] = {}
        for b, data in enumerate(files):
            try:
                heads.append(parse_jpeg(data))
            except JpegFallback:
                heads.append(None)
                fb_frames[b] = host_decode(bytes(data))
        hw = np.array([(h.height, h.width) if h is not None else fb_frames[b].shape[:2] for b, h in enumerate(heads)],
                      dtype=np.int64)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offset = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)   # as RaggedFrames.from_frames
        huff_index: Dict[Tuple, int] = {}
        huff_recs: List[np.ndarray] = []
        quant_index: Dict[bytes, int] = {}
        quant_rows: List[np.ndarray] = []

        def huff_id(kind, bits, vals):
            key = (kind, bits, vals)
            if key not in huff_index:
                huff_index[key] = len(huff_recs)
                huff_recs.append(derive_huffman(bits, vals, kind == "dc"))
            return huff_index[key]

        def quant_id(tab):
            row = tab.astype(np.uint16).view(np.int16).astype(np.int32)   # libjpeg-turbo's 16-bit islow multipliers
            key = row.tobytes()
            if key not in quant_index:
                quant_index[key] = len(quant_rows)
                quant_rows.append(row)
            return quant_index[key]

        frames, iv_rows, chunks = [], [], []
        pos, blocks, pixels = 0, 0, 0
        for b, h in enumerate(heads):
            if h is None:
                continue
            f = len(frames)
            row = np.zeros(FRAME_WORDS, dtype=np.int64)
            row[0:8] = (h.height, h.width, h.ncomp, h.hs, h.vs, h.mcux, h.mcuy, h.restart_interval)
            for c in range(h.ncomp):
                row[8 + c] = huff_id("dc", *h.tables[("dc", h.dc_ids[c])])
                row[11 + c] = huff_id("ac", *h.tables[("ac", h.ac_ids[c])])
                row[14 + c] = quant_id(h.quant[h.qt_ids[c]])
                row[17 + c] = blocks
                blocks += h.n_mcus * (h.hs * h.vs if c == 0 else 1)
            row[20], row[21] = offset[b] & 0xFFFFFFFF, offset[b] >> 32
            row[22], row[23] = pixels & 0xFFFFFFFF, pixels >> 32
            pixels += h.height * h.width
            frames.append(row)
            # the restart intervals, each on a 16-byte boundary of the packed buffer, zero-padded
            lens = h.lengths
            padded = (lens + 15) & ~15
            dst = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
            buf = np.zeros(int(padded.sum()), dtype=np.uint8)
            if len(h.data):
                buf[np.arange(len(h.data)) + np.repeat(dst - h.starts, lens)] = h.data
            chunks.append(buf)
            ri = h.restart_interval if h.restart_interval > 0 else h.n_mcus
            first = np.arange(h.n_intervals, dtype=np.int64) * ri
            r = np.zeros((h.n_intervals, INTERVAL_WORDS), dtype=np.int64)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = f, (pos + dst) // 4, lens, first, np.minimum(ri, h.n_mcus - first)
            iv_rows.append(r)
            pos += len(buf)
        if blocks >= 2 ** 31 or pos >= 2 ** 33:
            raise ValueError("JpegBatch: the batch is too large for the device tables")
        entropy = np.concatenate(chunks + [np.zeros(16, dtype=np.uint8)])
        iv = np.concatenate(iv_rows) if iv_rows else np.zeros((0, INTERVAL_WORDS), dtype=np.int64)
        iv = iv[np.argsort(-iv[:, 2], kind="stable")]   # longest first: the 64 lanes of a wave decode similar lengths
        n_sub = (iv[:, 2] + SUBSEQ_BYTES - 1) // SUBSEQ_BYTES   # (an empty interval has none)
        iv[:, 5] = np.cumsum(n_sub) - n_sub
        total_sub = int(n_sub.sum())
        if total_sub >= 2 ** 31:
            raise ValueError("JpegBatch: the batch is too large for the device tables")
        subseq = np.repeat(np.arange(len(iv), dtype=np.int32), n_sub)
        fb_ids = sorted(fb_frames)
        fb_sizes = np.array([fb_frames[b].size for b in fb_ids], dtype=np.int64)
        fb_table = np.zeros((len(fb_ids), 3), dtype=np.int64)
        if fb_ids:
            fb_table[:, 0] = np.concatenate([[0], np.cumsum(fb_sizes)[:-1]])
            fb_table[:, 1] = offset[fb_ids]
            fb_table[:, 2] = fb_sizes
        fallback = np.concatenate([fb_frames[b].reshape(-1) for b in fb_ids]) if fb_ids else np.zeros(0, dtype=np.uint8)
        t = {"entropy": torch.from_numpy(entropy),
             "intervals": torch.from_numpy(iv.astype(np.int32)),
             "frames": torch.from_numpy(np.stack(frames).astype(np.uint32).view(np.int32) if frames
                                        else np.zeros((0, FRAME_WORDS), dtype=np.int32)),
             "huff": torch.from_numpy(np.stack(huff_recs) if huff_recs else np.zeros((0, HUFF_RECORD), dtype=np.uint8)),
             "quant": torch.from_numpy(np.stack(quant_rows) if quant_rows else np.zeros((0, 64), dtype=np.int32)),
             "fallback": torch.from_numpy(fallback),
             "fallback_table": torch.from_numpy(fb_table),
             "offset": torch.from_numpy(offset.copy()),
             "hw": torch.from_numpy(hw.astype(np.int32)),
             "subseq": torch.from_numpy(subseq)}
        meta = {"offset": offset, "hw": hw, "blocks": int(blocks), "pixels": int(pixels), "nbytes": int(nbytes.sum()),
                "fallback": fb_ids, "n_subseq": total_sub}
        return cls(t, meta)
