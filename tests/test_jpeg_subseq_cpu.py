"""The host half of decoding in parallel inside a restart interval (no GPU): the subsequence table JpegBatch packs for
pm_jpeg_decode_parallel, and a pure-Python model of the device scheme -- one lane per subsequence that starts from a guessed decoder
state, hand-over inside a workgroup to a fixed point, rounds across workgroups through double-buffered states, the acceptance rule
E[i] == X[i - 1] -- compared with the sequential decoder's states at every subsequence boundary."""
import io
import pickle

import numpy as np
import pytest
import torch

from test_jpeg_host_cpu import _img, _jpeg, _png


def _mixed_files():
    rgb = _img(70, 90, 4)
    return [_jpeg(rgb, subsampling=2, quality=95), _jpeg(_img(40, 56, 5), mode="L", restart_marker_rows=1), _png(_img(12, 10, 6)),
            _jpeg(_img(33, 17, 7), subsampling=1, restart_marker_blocks=1), _jpeg(rgb, subsampling=0, quality=60),
            _jpeg(_img(64, 64, 8), mode="L", quality=100), _jpeg(_img(48, 48, 9), subsampling=2, restart_marker_rows=1)]


def test_subsequence_table_of_a_mixed_batch():
    from ssl4polyp_amd.jpeg import INTERVAL_WORDS, SUBSEQ_BYTES, JpegBatch
    assert SUBSEQ_BYTES % 16 == 0
    files = _mixed_files()
    jb = JpegBatch.from_bytes(files)
    assert "subseq" in JpegBatch.TENSORS and jb.meta["fallback"] == [2]
    iv, sub = jb.intervals.numpy(), jb.subseq.numpy()
    assert iv.shape[1] == INTERVAL_WORDS == 8 and sub.dtype == np.int32
    counts = -(-iv[:, 2] // SUBSEQ_BYTES)
    assert (counts > 1).any() and (counts == 1).any()   # intervals of several subsequences and of one
    # first-subsequence numbers: the exclusive scan of the counts in row order, so non-decreasing; meta["n_subseq"] their sum
    assert np.array_equal(iv[:, 5], np.cumsum(counts) - counts) and (np.diff(iv[:, 5]) >= 0).all()
    assert jb.meta["n_subseq"] == int(counts.sum()) == len(sub)
    assert (iv[:, 6:] == 0).all()
    # every byte of every interval lies in exactly one subsequence of its row
    for r, row in enumerate(iv):
        mine = np.flatnonzero(sub == r)
        assert np.array_equal(mine, row[5] + np.arange(counts[r]))
        covered = np.zeros(row[2], dtype=np.int64)
        for k in range(counts[r]):
            covered[k * SUBSEQ_BYTES:(k + 1) * SUBSEQ_BYTES] += 1
        assert (covered == 1).all() and counts[r] * SUBSEQ_BYTES >= row[2] > (counts[r] - 1) * SUBSEQ_BYTES
    # a lane finds its row by binary search over the first-subsequence numbers (rows without subsequences never match)
    for i in (0, len(sub) // 2, len(sub) - 1):
        r = int(np.searchsorted(iv[:, 5], i, side="right")) - 1
        while counts[r] == 0:
            r -= 1
        assert r == sub[i]
    # the old fields are what they were without the table: rows longest first, words 0..4 as the per-file parse gives them
    assert (np.diff(iv[:, 2]) <= 0).all() and jb.entropy.numel() % 16 == 0 and (iv[:, 1] % 4 == 0).all()
    back = pickle.loads(pickle.dumps(jb))
    assert all(torch.equal(back.t[k], jb.t[k]) for k in JpegBatch.TENSORS) and back.meta["n_subseq"] == jb.meta["n_subseq"]
    if torch.cuda.is_available():
        pinned = jb.pin_memory()
        assert pinned.is_pinned() and torch.equal(pinned.subseq, jb.subseq)
    # a batch without device frames has an empty table
    empty = JpegBatch.from_bytes([_png(_img(5, 6, 1))])
    assert empty.meta["n_subseq"] == 0 and empty.subseq.numel() == 0 and empty.subseq.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------------------
# the state machine of pm_jpeg.hip sub_decode<false> (decode_block's symbol rules without the coefficients), in Python
# ---------------------------------------------------------------------------------------------------------------------------
def _code_table(bits, vals):
    """16-bit window -> (code length, symbol); 17 bits / symbol 0 where no code of at most 16 bits matches (jpeg_huff_decode)"""
    ln, sy = [17] * 65536, [0] * 65536
    code, p = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo, n = code << (16 - l), 1 << (16 - l)
            ln[lo:lo + n] = [l] * n
            sy[lo:lo + n] = [vals[p]] * n
            code += 1
            p += 1
        code <<= 1
    return ln, sy


class _Machine:
    """One interval of a parsed file: step() decodes one symbol from the state (bit position p, block in MCU c, zigzag index z)."""

    def __init__(self, hd):
        assert hd.n_intervals == 1
        d = np.concatenate([np.asarray(hd.data, np.uint8), np.zeros(16, np.uint8)]).astype(np.uint64)
        self.w = ((d[:-2] << 16) | (d[1:-1] << 8) | d[2:]).tolist()   # 24 bits from every byte position
        self.nbits = int(hd.lengths[0]) * 8
        lum = hd.hs * hd.vs if hd.ncomp == 3 else 1
        comp = [0] * lum + [1, 2] if hd.ncomp == 3 else [0]
        self.bpm = len(comp)
        cache = {}

        def tab(kind, t):
            if (kind, t) not in cache:
                cache[(kind, t)] = _code_table(*[list(x) for x in hd.tables[(kind, t)]])
            return cache[(kind, t)]
        self.dc = [tab("dc", hd.dc_ids[c]) for c in comp]
        self.ac = [tab("ac", hd.ac_ids[c]) for c in comp]

    def step(self, p, c, z):
        win = (self.w[p >> 3] >> (8 - (p & 7))) & 0xFFFF if p < self.nbits else 0   # zero bits past the interval
        if z == 0:
            ln, sy = self.dc[c]
            return p + ln[win] + min(sy[win], 15), c, 1
        ln, sy = self.ac[c]
        r, s = sy[win] >> 4, sy[win] & 15
        p += ln[win] + s
        z = z + r + 1 if s else (z + 16 if r == 15 else 64)   # k += r, ++k; ZRL; EOB
        return (p, (c + 1) % self.bpm, 0) if z >= 64 else (p, c, z)

    def lane(self, i, entry, S):
        """from `entry` to the first symbol boundary at or past the end of subsequence i"""
        p, c, z = entry
        while p < (i + 1) * S:
            p, c, z = self.step(p, c, z)
        return p, c, z


def _scheme(M, S, wg, rounds):
    """The device scheme (jpeg_sync_kernel launched 1 + rounds times, then jpeg_verify_kernel's rule) -> (converged, E, busiest
    workgroup's steps in the first launch)."""
    n = -(-M.nbits // S)
    E = [(i * S, 0, 0) for i in range(n)]
    X = [None] * n
    first_steps = 0
    for r in range(rounds + 1):
        prev = list(X)   # what the last lanes held after the previous launch
        for w0 in range(0, n, wg):
            w1 = min(w0 + wg, n)
            if r == 0:
                dirty = set(range(w0, w1))
            elif w0 > 0 and prev[w0 - 1] != E[w0]:
                E[w0] = prev[w0 - 1]
                dirty = {w0}
            else:
                continue
            steps = 0
            while dirty:
                steps += 1
                assert steps <= wg + 1
                for i in dirty:
                    X[i] = M.lane(i, E[i], S)
                nxt = set()
                for i in dirty:
                    if i + 1 < w1 and E[i + 1] != X[i]:
                        E[i + 1] = X[i]
                        nxt.add(i + 1)
                dirty = nxt
            if r == 0:
                first_steps = max(first_steps, steps)
    return all(E[i] == X[i - 1] for i in range(1, n)), E, first_steps


def _sin_noise(h, w, seed, sigma=6.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.stack([127 + 90 * np.sin(xx / (17 + 5 * c) + yy / (23 - 3 * c) + c) for c in range(3)], -1)
    return np.clip(out + rng.normal(0, sigma, out.shape), 0, 255).astype(np.uint8)


def _endo_like(h, w, seed):
    """a textured disc on a black frame with a flat box, as endoscopy frames look"""
    img = _sin_noise(h, w, seed, 4.0)
    yy, xx = np.mgrid[0:h, 0:w]
    img[((yy - h / 2) ** 2 / (h * 0.48) ** 2 + (xx - w * 0.55) ** 2 / (w * 0.42) ** 2) > 1] = 0
    img[int(h * .7):int(h * .95), int(w * .02):int(w * .18)] = (0, 140, 60)
    return img


FRAMES = {"sinusoids + noise": lambda: _jpeg(_sin_noise(384, 480, 1), subsampling=2, quality=90),
          "optimized tables": lambda: _jpeg(_sin_noise(384, 480, 1), subsampling=2, quality=90, optimize=True),
          "endoscopy-like": lambda: _jpeg(_endo_like(384, 480, 2), subsampling=2, quality=90)}


@pytest.mark.parametrize("kind", list(FRAMES))
def test_model_of_the_device_scheme_synchronises_and_verifies(kind):
    """(i) a lane that starts from the guess meets the sequential decoder's trajectory long before a whole workgroup of
    subsequences has passed; (ii) with workgroups of 16 lanes (the frame then spans more than ten of them, as a 1080p frame spans the
    device's 256-lane workgroups) the scheme ends converged after one round with every entry state equal to the sequential
    decoder's, and not converged without a round -- the condition under which sync_rounds=2 converges on the device."""
    from ssl4polyp_amd.jpeg import SUBSEQ_BYTES, parse_jpeg
    S, wg = SUBSEQ_BYTES * 8, 16
    M = _Machine(parse_jpeg(FRAMES[kind]()))
    n = -(-M.nbits // S)
    assert n > 10 * wg
    # the sequential decoder: every symbol boundary, and its state at the first boundary at or past every subsequence start
    true, T = {}, [(0, 0, 0)]
    st = (0, 0, 0)
    while st[0] < M.nbits:
        true[st[0]] = st[1:]
        if st[0] >= len(T) * S:
            T.append(st)
        st = M.step(*st)
    T = T[:n]
    dist = []
    for i in range(1, n):
        p, c, z = i * S, 0, 0
        while p < M.nbits and true.get(p) != (c, z):
            p, c, z = M.step(p, c, z)
        dist.append(p - i * S)
    never = sum(1 for i, d in enumerate(dist, 1) if i * S + d >= M.nbits)
    assert never <= 8 and max(dist) < 256 * S // 8, (never, max(dist))   # a wrong entry never survives a workgroup (by 8x)
    ok, E, steps = _scheme(M, S, wg, rounds=1)
    assert ok and E == T and steps <= wg
    ok0, E0, _ = _scheme(M, S, wg, rounds=0)
    assert not ok0 and E0 != T
    ok2, E2, _ = _scheme(M, S, wg, rounds=2)
    assert ok2 and E2 == T
