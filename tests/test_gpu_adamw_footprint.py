"""The one-call AdamW update (pm_adamw_segments) and its bounded grid.  adamw_dev_kernel has no cross-element sums, so the
thread-to-element map is free: whatever the grid bound, every output -- P, M, V and the bf16 / fp16 shadow -- must equal
pm_adamw_dev's at its own grid BIT FOR BIT (torch.equal, no tolerance), after one and after three consecutive steps.

Sizes (elements; a vector is 4, a workgroup's trip of the unrolled loop 4 x 256 vectors = 4096 elements):
  4          one vector
  1 028      257 vectors: fewer than one workgroup's unrolled stride, a ragged trip
  262 148    64 whole trips + one ragged vector
  1 048 580  more than bound x stride for the bounds 1 and 3 and 256 (256 x 4096 = 1 048 576): every workgroup loops
"""
import functools

import pytest
import torch

from ssl4polyp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (4, 1028, 262148, 1048580)
BOUNDS = (1, 3, 256, 0)
SHADOWS = (None, torch.bfloat16, torch.float16)
GUARD = 64  # guard elements in front of and behind every buffer
HYPER = (1e-2, 0.9, 0.95, 1e-8, 0.05, 0.5)  # lr, beta1, beta2, eps, weight decay, gradient scale


class Bufs:
    """p / g / m / v (/ shadow) of n elements, each inside its own guarded allocation, from one seed."""

    def __init__(self, n, shadow, seed=0):
        gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
        self.n, self.full, self.guard = n, {}, {}
        for name in ("p", "g", "m", "v"):
            t = torch.randn(n + 2 * GUARD, device=DEV, generator=gen) * (1e-3 if name == "g" else 0.05)
            if name == "v":
                t = t.square()
            self.full[name] = t
        if shadow is not None:
            self.full["s"] = torch.randn(n + 2 * GUARD, device=DEV, generator=gen).to(shadow)
        for name, t in self.full.items():
            self.guard[name] = (t[:GUARD].clone(), t[GUARD + n:].clone())
        self.hyper = torch.zeros(2, 16, device=DEV)
        self.hyper[:, :6] = torch.tensor(HYPER, device=DEV)

    def view(self, name):
        t = self.full.get(name)
        return None if t is None else t[GUARD:GUARD + self.n]

    def ptr(self, name):
        t = self.view(name)
        return None if t is None else t.data_ptr()

    def dtype(self):
        return _lib.dtype_code(self.full["s"].dtype) if "s" in self.full else 0

    def guards_intact(self):
        return all(torch.equal(t[:GUARD], self.guard[k][0]) and torch.equal(t[GUARD + self.n:], self.guard[k][1])
                   for k, t in self.full.items())

    def snapshot(self):
        return {k: self.view(k).clone() for k in self.full}

    def segment(self, group=1, event=None):
        return _lib.AdamwSegment(self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.ptr("s"), self.dtype(), self.n,
                                 self.hyper[group].data_ptr(), event)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _segments(lib, bufs, bound):
    """One pm_adamw_segments call (tick + one launch per buffer set) on the current stream."""
    arr = (_lib.AdamwSegment * len(bufs))(*[b.segment() for b in bufs])
    _lib.check(lib.pm_adamw_segments(arr, len(bufs), bufs[0].hyper.data_ptr(), 2, None, _stream(), bound), "pm_adamw_segments")


@functools.lru_cache(maxsize=None)
def _reference(n, shadow):
    """pm_adamw_tick + pm_adamw_dev (its own full grid) on the seeded buffers: the state after one and after three steps."""
    lib = _lib.load()
    b = Bufs(n, shadow)
    snaps = {}
    for step in (1, 2, 3):
        _lib.check(lib.pm_adamw_tick(b.hyper.data_ptr(), 2, _stream()), "pm_adamw_tick")
        _lib.check(lib.pm_adamw_dev(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), b.ptr("s"), b.dtype(), n, b.hyper[1].data_ptr(),
                                    _stream()), "pm_adamw_dev")
        if step in (1, 3):
            snaps[step] = (b.snapshot(), b.hyper.clone())
    assert b.guards_intact()
    assert not torch.equal(snaps[1][0]["p"], snaps[3][0]["p"])  # (the update does move the parameters)
    return snaps


@pytest.mark.parametrize("shadow", SHADOWS, ids=["noshadow", "bf16", "fp16"])
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("n", SIZES)
def test_bits_equal_pm_adamw_dev_at_every_bound(n, bound, shadow):
    lib = _lib.load()
    ref = _reference(n, shadow)
    b = Bufs(n, shadow)
    for step in (1, 2, 3):
        _segments(lib, [b], bound)
        if step in (1, 3):
            want, hyper = ref[step]
            assert torch.equal(b.hyper, hyper)
            for k, t in b.snapshot().items():
                assert torch.equal(t, want[k]), (k, step)
    assert b.guards_intact()


@pytest.mark.parametrize("bound", (0, 3))
def test_skip_flag_leaves_everything_untouched(bound):
    lib = _lib.load()
    b = Bufs(262148, torch.bfloat16)
    _segments(lib, [b], bound)          # one ordinary step: the counter stands at 1
    b.hyper[:, 9] = 1.0                 # pm_loss_scale_update found a non-finite gradient
    before, hyper = b.snapshot(), b.hyper.clone()
    _segments(lib, [b], bound)
    assert torch.equal(b.hyper, hyper) and float(b.hyper[1, 6]) == 1.0  # pm_adamw_tick did not advance the step
    for k, t in b.snapshot().items():
        assert torch.equal(t, before[k]), k
    assert b.guards_intact()


def test_done_events_order_a_consumer_on_another_stream():
    """Three segments, three done events on a side stream; a consumer stream waits for event 1 ONLY and then reads segment 1's
    parameters: it must see the updated values (the segments run in order, so segment 0's as well)."""
    lib = _lib.load()
    n = 1048580
    want = _reference(n, torch.bfloat16)[1][0]
    bufs = [Bufs(n, torch.bfloat16) for _ in range(3)]
    for b in bufs[1:]:
        b.hyper = bufs[0].hyper  # one hyper-parameter array for the call
    side, consumer = torch.cuda.Stream(), torch.cuda.Stream()
    events = [torch.cuda.Event() for _ in range(3)]
    for e in events:
        e.record(side)  # (materialises the handles)
    fork = torch.cuda.Event()
    fork.record(torch.cuda.current_stream())  # the buffers were filled on the current stream
    segs = [b.segment(event=e.cuda_event) for b, e in zip(bufs, events)]
    arr = (_lib.AdamwSegment * 3)(*segs)
    _lib.check(lib.pm_adamw_segments(arr, 3, bufs[0].hyper.data_ptr(), 2, fork.cuda_event, side.cuda_stream, 3), "pm_adamw_segments")
    consumer.wait_event(events[1])
    with torch.cuda.stream(consumer):
        got_p, got_s, got_p0 = bufs[1].view("p").clone(), bufs[1].view("s").clone(), bufs[0].view("p").clone()
    consumer.synchronize()
    assert torch.equal(got_p, want["p"]) and torch.equal(got_s, want["s"]) and torch.equal(got_p0, want["p"])
    torch.cuda.synchronize()
    for b in bufs:
        assert b.guards_intact()
        assert torch.equal(b.view("p"), want["p"])


def test_whole_step_overlapped_equals_inline():
    """A two-block, D = 64 classifier: three steps with the overlapped FusedAdamW (pm_adamw_segments on the side stream, the next
    forward gated per block) against three steps inline -- parameters and losses bit for bit, twice over (the same bits every run)."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd.optim import FusedAdamW
    g = torch.Generator(device=DEV).manual_seed(11)
    imgs = torch.randn(4, 3, 224, 224, device=DEV, generator=g)
    labels = torch.tensor([1.0, 0.0, 0.0, 1.0], device=DEV)

    def run(overlap):
        torch.manual_seed(3)
        m = A.ViT_from_MAE(None, True, 2, False, None, embed_dim=64, depth=2, num_heads=2, out_token="cls").to(DEV)
        head = list(m.lin_head.parameters())
        hid = {id(p) for p in head}
        groups = [{"params": head, "lr": 2e-3}, {"params": [p for p in m.parameters() if id(p) not in hid and p.requires_grad]}]
        opt = FusedAdamW(m, groups, lr=1e-3, weight_decay=0.05, overlap_forward=overlap)
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            z = m(imgs)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(z[:, 1] - z[:, 0], labels)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        assert bool(m._rt.pending_updates) == overlap  # the overlapped path leaves its done events for the next forward
        opt.sync()
        torch.cuda.synchronize()
        return [float(x) for x in losses], [p.detach().clone() for p in m.parameters()]

    l0, p0 = run(False)
    for _ in range(2):
        l1, p1 = run(True)
        assert l0 == l1
        assert all(torch.equal(a, b) for a, b in zip(p0, p1))
