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
