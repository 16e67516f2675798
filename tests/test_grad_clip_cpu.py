"""Host side of gradient clipping and per-group norms (pm_grad_norms_workspace / pm_grad_norms / pm_grad_clip): the float64
reference the GPU tests use is pinned against torch, the symbols exist under the unchanged ABI version, the workspace query
answers and every refusal returns before any stream call, so all of it runs without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from ssl4polyp_amd import _lib


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    return _lib.load()


def test_reference_matches_torch_clip_grad_norm_and_adamw_in_float64():
    """Two groups, 5 steps, gradients whose norm lies above max_norm on some steps and below it on others."""
    rng = np.random.default_rng(3)
    shapes = [[(7, 5), (5,)], [(11, 3), (3,), (2, 2)]]
    init = [[rng.standard_normal(s) for s in grp] for grp in shapes]
    hyper = [dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05), dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)]
    tp = [[torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in grp] for grp in init]
    topt = torch.optim.AdamW([dict(params=ps, **h) for ps, h in zip(tp, hyper)])
    ref = R.ClippedAdamW([dict(params=[a.copy() for a in grp], **h) for grp, h in zip(init, hyper)])
    max_norm, active = 1.5, []
    for step, mag in enumerate((0.05, 3.0, 0.1, 0.6, 0.02)):
        grads = [[rng.standard_normal(s) * mag for s in grp] for grp in shapes]
        for ps, gs in zip(tp, grads):
            for p, g in zip(ps, gs):
                p.grad = torch.tensor(g, dtype=torch.float64)
        t_groups = [float(torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in ps]))) for ps in tp]
        t_total = float(torch.nn.utils.clip_grad_norm_([p for ps in tp for p in ps], max_norm))
        topt.step()
        gn, total, coef = ref.step(grads, max_norm)
        active.append(coef < 1.0)
        assert abs(total - t_total) <= 1e-14 * t_total and np.allclose(gn, t_groups, rtol=1e-14, atol=0)
        assert coef == R.clip_coef(t_total, max_norm) or abs(coef - R.clip_coef(t_total, max_norm)) < 1e-15
        for ps, rs in zip(tp, ref.groups):
            for p, r in zip(ps, rs["params"]):
                assert np.allclose(p.detach().numpy(), r, rtol=1e-12, atol=1e-15), step
    assert any(active) and not all(active), active
    # the moments follow the clipped gradient (Adam's parameters alone hardly show a scale): against an unclipped run they differ
    plain = R.ClippedAdamW([dict(params=[a.copy() for a in grp], **h) for grp, h in zip(init, hyper)])
    g = [[np.full(s, 2.0) for s in grp] for grp in shapes]
    _, total, coef = plain.step(g, None)
    assert coef == 1.0 and total == pytest.approx(2.0 * np.sqrt(sum(int(np.prod(s)) for grp in shapes for s in grp)))
    assert R.clip_coef(0.5, 1.0) == 1.0 and R.clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)
    gn, total = R.norms([9.0, 16.0, 0.0], [0.5, 0.5, 0.5])
    assert list(gn) == [1.5, 2.0, 0.0] and total == 2.5


def test_symbols_present_under_the_unchanged_abi(lib):
    assert lib.pm_abi_version() == _lib.ABI_VERSION == 16
    for name in ("pm_grad_norms_workspace", "pm_grad_norms", "pm_grad_clip"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.GradSegment) == 24  # the layout of pm_grad_segment on an LP64 host


def _ws(lib, n_segs, n_groups):
    size = ctypes.c_size_t(0)
    st = lib.pm_grad_norms_workspace(n_segs, n_groups, ctypes.byref(size))
    return st, size.value


def test_workspace_query_answers_without_a_device(lib):
    st, one = _ws(lib, 1, 2)
    assert st == 0 and one > 0 and one % 8 == 0
    # one [sum, #NaN, #Inf] f64 row per group and workgroup; it grows with the groups, and with the segments only per launch batch
    assert _ws(lib, 1, 4) == (0, 2 * one) and _ws(lib, 17, 2) == (0, one) and _ws(lib, 1000, 2)[1] > one
    assert lib.pm_grad_norms_workspace(1, 2, None) == _lib.PM_EINVAL
    assert _ws(lib, 0, 2)[0] == _lib.PM_ESHAPE and _ws(lib, 1, 0)[0] == _lib.PM_ESHAPE


def _seg(**over):
    """A well-formed segment over a made-up address (a refusal never dereferences or enqueues anything)."""
    f = dict(g=0x10000, n=1028, group=1)
    f.update(over)
    return _lib.GradSegment(**f)


def _norms(lib, segs, n_segs=None, n_groups=2, ws=0x20000, ws_bytes=None, sumsq=0x30000, stats=0x40000):
    arr = (_lib.GradSegment * max(len(segs), 1))(*segs)
    n = len(segs) if n_segs is None else n_segs
    if ws_bytes is None:
        ws_bytes = _ws(lib, max(n, 1), max(n_groups, 1))[1]
    return lib.pm_grad_norms(arr, n, n_groups, ws, ws_bytes, sumsq, stats, None)


def test_grad_norms_refusals(lib):
    assert lib.pm_grad_norms(None, 1, 2, 0x20000, 1 << 20, 0x30000, 0x40000, None) == _lib.PM_EINVAL
    for field in ("ws", "sumsq", "stats"):
        assert _norms(lib, [_seg()], **{field: None}) == _lib.PM_EINVAL, field
    assert _norms(lib, [_seg(), _seg(g=None)]) == _lib.PM_EINVAL
    assert _norms(lib, [_seg(n=0)]) == _lib.PM_ESHAPE
    assert _norms(lib, [_seg(), _seg(n=-4)]) == _lib.PM_ESHAPE
    assert _norms(lib, [_seg(n=1030)]) == _lib.PM_ESHAPE                      # n % 4 != 0
    assert _norms(lib, [_seg(group=2)]) == _lib.PM_EINVAL                     # a group index out of range ...
    assert _norms(lib, [_seg(), _seg(group=-1)]) == _lib.PM_EINVAL
    assert _norms(lib, [_seg()], ws_bytes=_ws(lib, 1, 2)[1] - 1) == _lib.PM_EINVAL   # a short workspace
    assert _norms(lib, [], n_segs=0) == _lib.PM_ESHAPE
    assert _norms(lib, [_seg(group=0)], n_groups=0) == _lib.PM_ESHAPE
    assert _norms(lib, [_seg(g=0x10004)]) == _lib.PM_EALIGN                   # 16-byte loads


def test_grad_clip_refusals(lib):
    ok = dict(sumsq=0x30000, hyper=0x50000, n_groups=2, max_norm=1.0, clip=1, scaled=0, record=0x60000)

    def call(**over):
        a = dict(ok)
        a.update(over)
        return lib.pm_grad_clip(a["sumsq"], a["hyper"], a["n_groups"], a["max_norm"], a["clip"], a["scaled"], a["record"], None)

    for field in ("sumsq", "hyper", "record"):
        assert call(**{field: None}) == _lib.PM_EINVAL, field
    assert call(n_groups=0) == _lib.PM_ESHAPE
    for bad in (0.0, -1.0, float("nan")):
        assert call(max_norm=bad) == _lib.PM_EINVAL, bad                      # max_norm <= 0
