"""Host side of the one-call AdamW update (pm_adamw_segments / pm_adamw_grid): the grid arithmetic and the argument refusals.
Both return before any stream call, so they run without a device (as the plan functions of test_host_cpu.py do)."""
import ctypes
import os

import pytest

from ssl4polyp_amd import _lib

SIZES = (4, 1028, 262148, 1048580)  # the sizes tests/test_gpu_adamw_footprint.py updates
CHUNK = 4 * 256                      # vectors per workgroup and loop trip of adamw_dev_kernel (kAdamwChunk)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    return _lib.load()


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("n", SIZES)
def test_grid(lib, n):
    nvec = n // 4
    # no bound: the grid pm_adamw_dev has always used, one workgroup per 256 vectors up to 4096
    assert lib.pm_adamw_grid(n, 0) == min(max(_ceil(nvec, 256), 1), 4096)
    # a bound: one workgroup per chunk of the unrolled loop, never more than the bound, never an idle workgroup
    assert lib.pm_adamw_grid(n, 1) == 1
    assert lib.pm_adamw_grid(n, 256) == min(_ceil(nvec, CHUNK), 256)
    for bound in (1, 3, 256):
        g = lib.pm_adamw_grid(n, bound)
        assert 1 <= g <= bound and (g - 1) * CHUNK < nvec


def test_grid_of_a_vit_b_block_and_refusals(lib):
    assert lib.pm_adamw_grid(7077888, 0) == 4096     # a ViT-B block's matrices: capped
    assert lib.pm_adamw_grid(7077888, 256) == 256
    assert lib.pm_adamw_grid(7077888, 4096) == 1728  # fewer chunks than the bound
    assert lib.pm_adamw_grid(0, 0) == _lib.PM_ESHAPE
    assert lib.pm_adamw_grid(6, 0) == _lib.PM_ESHAPE
    assert lib.pm_adamw_grid(1024, -1) == _lib.PM_ESHAPE


def _segment(**over):
    """A well-formed segment over made-up addresses (a refusal never dereferences or enqueues anything)."""
    f = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, shadow=0x5000, shadow_dtype=_lib.PM_BF16, n=1028, hyper=0x6000, done_event=None)
    f.update(over)
    return _lib.AdamwSegment(**f)


def _call(lib, segs, n_segs=None, hyper=0x6000, n_groups=1, max_blocks=0):
    arr = (_lib.AdamwSegment * max(len(segs), 1))(*segs)
    return lib.pm_adamw_segments(arr if segs is not None else None, len(segs) if n_segs is None else n_segs, hyper, n_groups,
                                 None, None, max_blocks)


def test_segments_refusals(lib):
    assert ctypes.sizeof(_lib.AdamwSegment) == 72  # the layout of pm_adamw_segment on an LP64 host
    assert lib.pm_adamw_segments(None, 1, 0x6000, 1, None, None, 0) == _lib.PM_EINVAL
    assert _call(lib, [_segment()], hyper=None) == _lib.PM_EINVAL
    for field in ("p", "g", "m", "v", "hyper"):
        assert _call(lib, [_segment(), _segment(**{field: None})]) == _lib.PM_EINVAL, field
    assert _call(lib, [_segment(shadow_dtype=7)]) == _lib.PM_EINVAL            # an unknown shadow type ...
    assert _call(lib, [_segment(n=1030)]) == _lib.PM_ESHAPE                    # n % 4 != 0
    assert _call(lib, [_segment(), _segment(n=0)]) == _lib.PM_ESHAPE
    assert _call(lib, [], n_segs=0) == _lib.PM_ESHAPE                          # zero segments
    assert _call(lib, [_segment()], n_groups=0) == _lib.PM_ESHAPE
    assert _call(lib, [_segment()], max_blocks=-1) == _lib.PM_ESHAPE


def test_alignment_refusals(lib):
    """p, g, m, v and an f32 shadow are moved as 16-byte vectors, a 16-bit shadow as 8-byte ones: anything else is PM_EALIGN, from
    pm_adamw_segments (any segment), pm_adamw_dev and pm_adamw alike -- after the NULL / shape / type refusals, before any launch."""
    for field, base in (("p", 0x1000), ("g", 0x2000), ("m", 0x3000), ("v", 0x4000)):
        for off in (4, 8, 12):
            assert _call(lib, [_segment(), _segment(**{field: base + off})]) == _lib.PM_EALIGN, (field, off)
    for dt in (_lib.PM_BF16, _lib.PM_F16):
        for off in (2, 4, 6):
            assert _call(lib, [_segment(shadow=0x5000 + off, shadow_dtype=dt)]) == _lib.PM_EALIGN, (dt, off)
    for off in (4, 8, 12):
        assert _call(lib, [_segment(shadow=0x5000 + off, shadow_dtype=_lib.PM_F32)]) == _lib.PM_EALIGN, off
    # the earlier refusals keep their status on a misaligned segment
    assert _call(lib, [_segment(p=0x1004, n=1030)]) == _lib.PM_ESHAPE
    assert _call(lib, [_segment(p=0x1004, shadow_dtype=7)]) == _lib.PM_EINVAL
    assert _call(lib, [_segment(p=0x1004, g=None)]) == _lib.PM_EINVAL
    # pm_adamw_dev and pm_adamw (made-up addresses: every call here returns before a launch)
    well = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, s=0x5000, dt=_lib.PM_BF16)
    args = lambda o: [{**well, **o}[k] for k in ("p", "g", "m", "v", "s", "dt")]
    dev = lambda **o: lib.pm_adamw_dev(*args(o), 1028, 0x6000, None)
    host = lambda **o: lib.pm_adamw(*args(o), 1028, 1e-3, 0.9, 0.95, 1e-8, 0.05, 1, 1.0, None)
    for call in (dev, host):
        for k, base in (("p", 0x1000), ("g", 0x2000), ("m", 0x3000), ("v", 0x4000)):
            assert call(**{k: base + 8}) == _lib.PM_EALIGN, k
        assert call(s=0x5004) == _lib.PM_EALIGN
        assert call(s=0x5008, dt=_lib.PM_F32) == _lib.PM_EALIGN
        assert call(p=0x1008, s=0x5000, dt=7) == _lib.PM_EINVAL
    assert host(p=None) == _lib.PM_EINVAL
