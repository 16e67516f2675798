"""The two-stage column sums keep their bits: pm_colsum_ws, the mask-token gradient of pm_mae_unshuffle_bwd and the three sums of
pm_layernorm_bwd (first-stage kernel + reduce_partial_rows) against tests/golden/partial_sums.npz, by equality.  The fixture was
written by tests/golden/make_partial_sums.py with the library as it stood before the three reduce kernels became one; the cases
and what each of them reaches are in tests/partial_sums_cases.py."""
import functools

import numpy as np
import pytest
import torch

import partial_sums_cases as cases

pytestmark = pytest.mark.gpu

DEV = cases.DEV


@functools.lru_cache(maxsize=None)
def _k(prec):
    from ssl4polyp_amd.engine import Kernels
    return Kernels(prec)


@pytest.fixture(scope="module")
def outs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return cases.outputs(_k)


def test_every_case_matches_the_fixture(outs, golden):
    want = golden("partial_sums.npz")
    got = cases.freeze(outs)
    assert sorted(got) == sorted(want)
    bad = [name for name in sorted(want) if not np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8))]
    assert not bad, bad


def test_cases_reach_the_branches_they_name():
    """The shapes are what the case table says they are: 128 splits, 115 and 1024 partial rows (the libraries' own grid rules)."""
    lib = _k("bf16").lib
    from ssl4polyp_amd import _lib
    M, N = cases.COLSUM_SHAPES[2]
    assert lib.pm_workspace_bytes(_lib.WS_COLSUM, M, N) == 128 * N * 4 and lib.pm_workspace_bytes(_lib.WS_COLSUM, 5, 4) == 4 * 4
    B, L, keep, D = cases.UNSHUFFLE_SHAPES[1]
    assert -(-B * (L - keep) // 64) == 115
    M, D = cases.LAYERNORM_SHAPES[1]
    assert lib.pm_workspace_bytes(_lib.WS_LAYERNORM_BWD, M, D) == 1024 * 3 * D * 4


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_unshuffle_bwd_gathers_the_kept_rows(outs, prec):
    for B, L, keep, D in cases.UNSHUFFLE_SHAPES:
        dx, ids = cases.unshuffle_input(B, L, keep, D)
        src = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=DEV), 1 + ids[:, :keep].long()], dim=1)   # [B, keep + 1]
        want = dx.view(B, L + 1, D).gather(1, src[:, :, None].expand(B, keep + 1, D)).reshape(B * (keep + 1), D)
        got = outs[f"unshuffle/{prec}/{B}x{L}x{keep}x{D}/demb"]
        assert torch.equal(got, want.to(got.dtype))


def test_column_sums_on_two_streams_at_once(outs):
    """Kernels.colsum on two non-default streams at once and once alone: the same bits three times, and each stream was given a
    scratch buffer of its own."""
    k = _k("bf16")
    M, N = 1031, 260
    x = cases.colsum_input(M, N, "f32")
    alone = outs[f"colsum/f32/{M}x{N}/zero"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = [torch.zeros(N, device=DEV) for _ in streams]
    torch.cuda.synchronize()
    for st, o in zip(streams, res):
        with torch.cuda.stream(st):
            k.colsum(x, o, M, N)
    torch.cuda.synchronize()
    assert torch.equal(res[0], alone) and torch.equal(res[1], alone)
    bufs = [k._scratch(0, x.device, st) for st in streams] + [k._scratch(0, x.device)]
    assert len({b.data_ptr() for b in bufs}) == 3
