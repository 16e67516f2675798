"""The kernels that write the weights, on the device, against the float64 restatements and element-wise bounds of
tests/optim_ref.py at the cases of tests/optim_cases.py: pm_adamw, pm_adamw_tick + pm_adamw_dev, pm_adamw_segments (bounded grid),
the two tick kernels, pm_loss_scale_update, pm_grad_stats, pm_dgelu and pm_scale.  Every comparison is made on the operands the
kernel saw (a multi-step case feeds the reference the device's own outputs of the previous step), every buffer lies between guard
regions that are checked afterwards, and every test prints its largest err / bound per output (pytest -s)."""
import ctypes
import functools

import pytest
import torch

import optim_cases as C
import optim_ref as R
from rowops_cases import cast_table
from ssl4polyp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64          # guard elements in front of and behind every buffer (keeps the 16-byte alignment of the payload)
GUARD_VALUE = 77.0  # exact in every type used here, int32 included
SHADOWS = {"noshadow": None, "bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
ENTRIES = ("host", "dev", "segments")   # pm_adamw | pm_adamw_tick + pm_adamw_dev | pm_adamw_segments with max_blocks = 3
PEAKS = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _peak(name, value):
    PEAKS[name] = max(PEAKS.get(name, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def _report_peaks():
    yield
    print("\npeaks (largest err / bound per kernel and output):")
    for k in sorted(PEAKS):
        print(f"  {k:34s} {PEAKS[k]:.3f}")


class Bufs:
    """Named device buffers, each the payload of its own guarded allocation."""

    def __init__(self, **tensors):
        self.full, self.n = {}, {}
        for name, t in tensors.items():
            self.add(name, t)

    def add(self, name, t):
        t = t.reshape(-1)
        full = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE, dtype=t.dtype, device=DEV)
        full[GUARD:GUARD + t.numel()] = t.to(DEV)
        self.full[name], self.n[name] = full, t.numel()

    def __getitem__(self, name):
        return self.full[name][GUARD:GUARD + self.n[name]]

    def ptr(self, name):
        return self[name].data_ptr()

    def snapshot(self, *names):
        return {k: self[k].clone() for k in (names or self.full)}

    def guards_intact(self):
        return all(bool((t[:GUARD] == GUARD_VALUE).all()) and bool((t[GUARD + self.n[k]:] == GUARD_VALUE).all())
                   for k, t in self.full.items())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


# ================================================================================================ AdamW
@functools.lru_cache(maxsize=8)
def _inputs(n, regime, gscale, seed=0):
    return C.adamw_inputs(n, regime, gscale, seed)


def _adamw_bufs(n, regime, hname, shadow_dtype, seed=0):
    p, g, m, v = _inputs(n, regime, C.hyper_gscale(hname), seed)
    b = Bufs(p=p, g=g, m=m, v=v)
    # the shadow buffer exists even when the call is given NULL: nothing may write it then
    b.add("s", torch.full((n,), 3.0, dtype=shadow_dtype or torch.bfloat16))
    # record 1 is the one in use; record 0 holds another group's values that the segment must not read
    b.add("hyper", torch.stack([R.record(0.5, 0.5, 0.5, 1.0, 0.5, 3.0, 0.0, step=7), R.record(*C.HYPERS[hname])]))
    return b


def _hyper(b):
    return b["hyper"].reshape(2, R.STRIDE)


def _step(lib, entry, b, hname, step, shadow_dtype):
    """One update through `entry`; the counter stood at step - 1.  -> the record the kernel applied (CPU f32)."""
    n = b.n["p"]
    s_ptr = b.ptr("s") if shadow_dtype is not None else None
    code = _lib.dtype_code(shadow_dtype) if shadow_dtype is not None else 0
    rec_ptr = b.ptr("hyper") + 4 * R.STRIDE
    if entry == "host":
        h = C.HYPERS[hname]
        _lib.check(lib.pm_adamw(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), s_ptr, code, n, h[0], h[1], h[2], h[3], h[4], step,
                                C.hyper_gscale(hname), _stream()), "pm_adamw")
        return R.record(h[0], h[1], h[2], h[3], h[4], C.hyper_gscale(hname), 0.0, step=step)
    assert float(_hyper(b)[1, 6]) == step - 1
    if entry == "dev":
        _lib.check(lib.pm_adamw_tick(b.ptr("hyper"), 2, _stream()), "pm_adamw_tick")
        _lib.check(lib.pm_adamw_dev(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), s_ptr, code, n, rec_ptr, _stream()), "pm_adamw_dev")
    else:
        seg = _lib.AdamwSegment(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), s_ptr, code, n, rec_ptr, None)
        arr = (_lib.AdamwSegment * 1)(seg)
        _lib.check(lib.pm_adamw_segments(arr, 1, b.ptr("hyper"), 2, None, _stream(), C.SEGMENT_BOUND), "pm_adamw_segments")
    rec = _hyper(b)[1].cpu()
    assert float(rec[6]) == step
    return rec


def _check_step(b, before, rec, shadow_dtype, tag):
    """The buffers after one update against adamw_step on what they held before.  -> the ratios."""
    ref = R.adamw_step(before["p"], before["g"], before["m"], before["v"], rec)
    r = R.adamw_ratios(b["p"], b["m"], b["v"], ref)
    for k, x in r.items():
        _peak(f"adamw[{tag}] {k}", x)
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    assert same_bits(b["g"], before["g"])
    if shadow_dtype is None:
        assert same_bits(b["s"], before["s"])            # a NULL shadow writes nothing
    else:
        assert R.equal_bits(b["s"], b["p"].to(shadow_dtype))
    assert b.guards_intact()
    return r


def _set_step(b, step):
    """Put record 1 at `step` (slots 6, 7, 8 as a tick would have left them)."""
    h = _hyper(b)[1].cpu()
    rec = R.record(*[float(x) for x in h[:6]], float(h[10]), step=step)
    b["hyper"][R.STRIDE:2 * R.STRIDE] = rec.to(DEV)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shadow", SHADOWS)
@pytest.mark.parametrize("n", C.ADAMW_SIZES + (C.ADAMW_CAP,))
def test_adamw_sizes(n, shadow, entry):
    """Every size (the suite's regime; gradient x 0.5 / 1024), every shadow type and NULL, every entry point; three consecutive
    steps at 1028 and 4100."""
    lib, dt, hname = _lib.load(), SHADOWS[shadow], "half_inv1024"
    b = _adamw_bufs(n, "suite", hname, dt)
    worst = {}
    for step in ((1, 2, 3) if n in C.ADAMW_MULTI_STEP else (1,)):
        if step > 1:
            b["g"].copy_(_inputs(n, "suite", C.hyper_gscale(hname), step)[1].to(DEV))
        before = b.snapshot("p", "g", "m", "v", "s")
        rec = _step(lib, entry, b, hname, step, dt)
        for k, x in _check_step(b, before, rec, dt, entry).items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"adamw n={n} {shadow} {entry}: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))


@pytest.mark.parametrize("hname", C.HYPERS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_adamw_regimes(regime, hname):
    """Every regime x hyper set at every step count, through all three entry points (n = 4100: a whole chunk and a ragged one)."""
    lib, n, worst = _lib.load(), 4100, {}
    for entry in ENTRIES:
        for step in C.STEPS:
            if regime == "cold" and step != 1:
                continue
            b = _adamw_bufs(n, regime, hname, torch.bfloat16, seed=step % 7)
            _set_step(b, step - 1)
            before = b.snapshot("p", "g", "m", "v", "s")
            rec = _step(lib, entry, b, hname, step, torch.bfloat16)
            for k, x in _check_step(b, before, rec, torch.bfloat16, entry).items():
                worst[k] = max(worst.get(k, 0.0), x)
            if regime in ("tiny", "huge"):
                assert bool(torch.isfinite(b["p"]).all())
    print(f"adamw {regime} {hname}: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))


def test_adamw_host_and_device_records_report_bit_equality():
    """pm_adamw against pm_adamw_tick + pm_adamw_dev from the same operands: reported, not asserted (the two kernels are compiled
    separately and may contract differently; each is held to the bound above)."""
    lib = _lib.load()
    for n in (1028, 4100):
        outs = {}
        for entry in ("host", "dev"):
            b = _adamw_bufs(n, "suite", "half", torch.bfloat16)
            rec = _step(lib, entry, b, "half", 1, torch.bfloat16)
            outs[entry] = (b.snapshot("p", "m", "v", "s"), rec)
        assert torch.equal(outs["host"][1][:9], outs["dev"][1][:9])   # the device's tick stored the host's corrections
        same = {k: same_bits(outs["host"][0][k], outs["dev"][0][k]) for k in ("p", "m", "v", "s")}
        print(f"pm_adamw == pm_adamw_dev bit for bit at n={n}: {same}")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shadow", ("bf16", "fp16", "f32"))
def test_adamw_shadow_store_is_the_cast(shadow, entry):
    """lr = 0, g = m = v = 0, p = the cast table (every tie, subnormal, overflow, infinity and NaN): the update is the identity on
    p, and the shadow store is torch's round-to-nearest-even conversion of every one of the 327 680 values."""
    lib, dt = _lib.load(), SHADOWS[shadow]
    p = cast_table()
    n = p.numel()
    z = torch.zeros(n)
    b = Bufs(p=p, g=z, m=z, v=z, s=torch.full((n,), 3.0, dtype=dt),
             hyper=torch.stack([R.record(0.5, 0.5, 0.5, 1.0, 0.5, 3.0), R.record(*C.HYPERS["lr0"])]))
    _step(lib, entry, b, "lr0", 1, dt)
    assert R.equal_bits(b["p"], p.to(DEV))
    fin = ~torch.isnan(p)
    assert same_bits(b["p"][fin.to(DEV)], p[fin].to(DEV))      # finite values and infinities keep their very bits (-0.0, subnormals)
    assert not b["m"].any() and not b["v"].any()
    assert R.equal_bits(b["s"], p.to(DEV).to(dt)) and R.equal_bits(b["s"].cpu(), p.to(dt))
    assert b.guards_intact()


@pytest.mark.parametrize("entry", ENTRIES)
def test_adamw_nonfinite_gradients_stay_where_they_are(entry):
    """No scaler: a NaN / +inf / -inf gradient poisons its own element only.  Positions with a finite gradient keep the bits of a run
    in which the others were zero; the poisoned ones show the NaN / Inf pattern of the f32 emulation."""
    lib, n, hname = _lib.load(), 4100, "b95_wd"
    at = torch.tensor(C.NONFINITE_AT)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")]).repeat(2)
    outs = {}
    for run in ("zeroed", "planted"):     # (the planted run last: `before` and `rec` are its own)
        b = _adamw_bufs(n, "suite", hname, torch.float16)
        b["g"][at.to(DEV)] = bad.to(DEV) if run == "planted" else 0.0
        before = b.snapshot("p", "g", "m", "v")
        _set_step(b, 1)
        rec = _step(lib, entry, b, hname, 2, torch.float16)
        outs[run] = b.snapshot("p", "m", "v", "s")
        assert b.guards_intact()
    clean = torch.ones(n, dtype=torch.bool)
    clean[at] = False
    for k in ("p", "m", "v", "s"):
        assert same_bits(outs["planted"][k][clean.to(DEV)], outs["zeroed"][k][clean.to(DEV)]), k
    emu = R.adamw_f32(before["p"], before["g"], before["m"], before["v"], rec, torch.float16)
    assert bool(torch.isnan(emu["p"][at]).all()) and bool(torch.isinf(emu["v"][at[1:3]]).all())   # (the pattern is not trivial)
    for k, ek in (("p", "p"), ("m", "m"), ("v", "v"), ("s", "shadow")):
        got, want = outs["planted"][k][at.to(DEV)].float().cpu(), emu[ek][at].float()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), k
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)]), k


@pytest.mark.parametrize("entry", ("dev", "segments"))
@pytest.mark.parametrize("n", (4, 4100))
def test_adamw_skip_flag_leaves_every_byte(n, entry):
    lib = _lib.load()
    b = _adamw_bufs(n, "suite", "half_inv1024", torch.bfloat16)
    _set_step(b, 5)
    b["hyper"][R.STRIDE + 9] = 1.0
    before = b.snapshot()
    rec_ptr, st = b.ptr("hyper") + 4 * R.STRIDE, _stream()
    if entry == "dev":
        _lib.check(lib.pm_adamw_tick(b.ptr("hyper"), 2, st), "pm_adamw_tick")
        _lib.check(lib.pm_adamw_dev(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), b.ptr("s"), 1, n, rec_ptr, st), "pm_adamw_dev")
    else:
        arr = (_lib.AdamwSegment * 1)(_lib.AdamwSegment(b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"), b.ptr("s"), 1, n, rec_ptr, None))
        _lib.check(lib.pm_adamw_segments(arr, 1, b.ptr("hyper"), 2, None, st, C.SEGMENT_BOUND), "pm_adamw_segments")
    for k in ("p", "g", "m", "v", "s"):
        assert same_bits(b[k], before[k]), k
    h0, h1 = _hyper(b), before["hyper"].reshape(2, R.STRIDE)
    assert same_bits(h0[1], h1[1])                                    # the skipped record: untouched, the counter included
    assert float(h0[0, 6]) == 8.0 and same_bits(h0[0, :6], h1[0, :6]) and same_bits(h0[0, 9:], h1[0, 9:])   # its neighbour ticked
    assert b.guards_intact()


# ================================================================================================ ticks
def _check_ticked(got, before, ticked, tag):
    """got / before [n, 16] on the CPU; ticked: the record indices the kernel was asked to advance."""
    want, moved = before.clone(), torch.zeros(before.shape[0], dtype=torch.bool)
    for i in ticked:
        t = R.tick(before[i])
        if t is not None:
            want[i, 6], want[i, 7], want[i, 8] = t
            moved[i] = True
    other = [j for j in range(R.STRIDE) if j not in (7, 8)]
    assert same_bits(got[:, other], want[:, other])                   # h[6] exact; every other slot, skipped and unlisted records
    assert same_bits(got[~moved], before[~moved])
    ulps = R.ulps_apart(got[moved][:, 7:9], want[moved][:, 7:9])
    exact = int((ulps == 0).sum())
    print(f"{tag}: {int(moved.sum())} records advanced, corrections exact in {exact} of {ulps.numel()}, worst {int(ulps.max()) if ulps.numel() else 0} ulp")
    _peak(f"{tag} ulps", float(ulps.max()) if ulps.numel() else 0.0)
    assert ulps.numel() == 0 or int(ulps.max()) <= 1
    sat = moved & (before[:, 6] >= 16777215.0)
    assert bool((got[sat][:, 6] == R.SATURATED).all()) and bool((got[sat][:, 7:9] == 1.0).all())   # the counter saturates at 2^24
    return moved


@pytest.mark.parametrize("n", C.TICK_N)
def test_tick(n):
    lib = _lib.load()
    recs = C.tick_records(n)
    b = Bufs(hyper=recs)
    _lib.check(lib.pm_adamw_tick(b.ptr("hyper"), n, _stream()), "pm_adamw_tick")
    moved = _check_ticked(b["hyper"].reshape(n, R.STRIDE).cpu(), recs, range(n), f"tick n={n}")
    assert int(moved.sum()) == n - len(range(1, n, 3)) and b.guards_intact()


@pytest.mark.parametrize("n_list", C.TICK_N)
def test_tick_list(n_list):
    lib, n = _lib.load(), 200
    recs, lst = C.tick_records(n, seed=1), C.tick_list(n, n_list)
    b = Bufs(hyper=recs, list=lst)
    host = (ctypes.c_int * n_list)(*lst.tolist())
    _lib.check(lib.pm_adamw_tick_list(b.ptr("hyper"), n, b.ptr("list"), host, n_list, _stream()), "pm_adamw_tick_list")
    _check_ticked(b["hyper"].reshape(n, R.STRIDE).cpu(), recs, lst.tolist(), f"tick_list n_list={n_list}")
    assert torch.equal(b["list"].cpu(), lst) and b.guards_intact()


def test_tick_saturated_counter_stays():
    """A record at 16 777 216 = 2^24 stays there: 2^24 + 1 is not an f32.  Both corrections are 1.0."""
    lib = _lib.load()
    recs = torch.stack([R.record(1e-3, b1, b2, 1e-8, 0.05, step=C.TICK_SATURATED) for b1, b2 in C.TICK_BETAS])
    recs[:, 7:9] = 0.5
    b = Bufs(hyper=recs)
    for _ in range(2):
        _lib.check(lib.pm_adamw_tick(b.ptr("hyper"), 2, _stream()), "pm_adamw_tick")
        got = b["hyper"].reshape(2, R.STRIDE).cpu()
        assert got[:, 6].tolist() == [R.SATURATED] * 2 and bool((got[:, 7:9] == 1.0).all())
    assert b.guards_intact()


# ================================================================================================ loss scale
@pytest.mark.parametrize("n_groups", C.LS_GROUPS)
def test_loss_scale_update(n_groups):
    """Every cell of the table at this group count: state[0..5] and slots 9, 10 of every record exact, everything else untouched."""
    lib = _lib.load()
    hyper0 = torch.randn(n_groups, R.STRIDE, generator=C.gen(80 + n_groups))
    for name, state, stats, growth, backoff, interval in C.loss_scale_cells():
        b = Bufs(state=torch.tensor(state + [11.0, 13.0]), stats=torch.tensor(stats), hyper=hyper0)
        before = b.snapshot()
        _lib.check(lib.pm_loss_scale_update(b.ptr("state"), b.ptr("stats"), b.ptr("hyper"), n_groups, growth, backoff, interval,
                                            _stream()), "pm_loss_scale_update")
        new, found, inv = R.loss_scale_update(state, stats, growth, backoff, interval)
        got = b["state"].cpu()
        assert got[:6].tolist() == new, (name, got.tolist(), new)
        assert got[6:].tolist() == [11.0, 13.0]
        h = b["hyper"].reshape(n_groups, R.STRIDE).cpu()
        assert bool((h[:, 9] == found).all()) and bool((h[:, 10] == inv).all()), name
        other = [j for j in range(R.STRIDE) if j not in (9, 10)]
        assert same_bits(h[:, other], hyper0[:, other]), name
        assert same_bits(b["stats"], before["stats"]) and b.guards_intact(), name


# ================================================================================================ grad stats
def _grad_stats(lib, g, prior):
    b = Bufs(g=g, out=torch.tensor(prior))
    _lib.check(lib.pm_grad_stats(b.ptr("g"), g.numel(), b.ptr("out"), _stream()), "pm_grad_stats")
    assert same_bits(b["g"], g.to(DEV)) and b.guards_intact()
    return b["out"].cpu()


@pytest.mark.parametrize("n", C.STATS_SIZES)
def test_grad_stats(n):
    lib, g = _lib.load(), C.stats_input(n)
    for prior in ((0.0, 0.0, 0.0), C.STATS_PRIOR):                    # `out` accumulates
        got, ref = _grad_stats(lib, g, prior), R.grad_stats(g, prior)
        r = abs(got[0].double().item() - ref["ss"]) / ref["e_ss"]
        _peak("grad_stats ss", r)
        print(f"grad_stats n={n} prior={prior[0]}: ss err / bound {r:.3f}")
        assert r <= 1.0 and got[1].item() == ref["nan"] and got[2].item() == ref["inf"]
    for where, i in C.stats_plants(n).items():                        # one of each planted around position i; the sum is not looked at
        for values in ((float("nan"),), (float("inf"), -float("inf")), (float("nan"), float("inf"), -float("inf"))):
            gp = g.clone()
            idx = [j for j in (i, i - 1, i + 1) if 0 <= j < n][:len(values)]
            gp[idx] = torch.tensor(values[:len(idx)])
            got, ref = _grad_stats(lib, gp, C.STATS_PRIOR), R.grad_stats(gp, C.STATS_PRIOR)
            assert (got[1].item(), got[2].item()) == (ref["nan"], ref["inf"]), (where, values)
            assert not ref["finite"] and not torch.isfinite(got[0])


def test_grad_stats_refuses_a_misaligned_gradient():
    lib = _lib.load()
    b = Bufs(g=C.stats_input(64), out=torch.tensor(C.STATS_PRIOR))
    assert lib.pm_grad_stats(b.ptr("g") + 4, 60, b.ptr("out"), _stream()) == _lib.PM_EALIGN
    assert lib.pm_grad_stats(None, 60, b.ptr("out"), _stream()) == _lib.PM_EINVAL
    assert lib.pm_grad_stats(b.ptr("g"), 0, b.ptr("out"), _stream()) == _lib.PM_ESHAPE
    assert b["out"].cpu().tolist() == list(C.STATS_PRIOR) and b.guards_intact()


# ================================================================================================ dgelu, scale
@pytest.mark.parametrize("n", C.DGELU_SIZES)
@pytest.mark.parametrize("prec", ("bf16", "fp16", "fp32"))
def test_dgelu(prec, n):
    lib = _lib.load()
    dy, pre = C.dgelu_inputs(n, prec)
    b = Bufs(dy=dy, pre=pre, out=torch.full((n,), 3.0, dtype=dy.dtype))
    _lib.check(lib.pm_dgelu(b.ptr("dy"), b.ptr("pre"), b.ptr("out"), _lib.dtype_code(dy.dtype), n, _stream()), "pm_dgelu")
    want, bound = R.dgelu(b["dy"], b["pre"], prec)
    r = R.ratio(b["out"], want, bound)
    _peak(f"dgelu {prec}", r)
    print(f"dgelu {prec} n={n}: err / bound {r:.3f}")
    assert r <= 1.0
    assert same_bits(b["dy"], dy.to(DEV)) and same_bits(b["pre"], pre.to(DEV)) and b.guards_intact()


def test_dgelu_refusals():
    lib = _lib.load()
    for prec, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        dy, pre = C.dgelu_inputs(64, prec)
        b = Bufs(dy=dy, pre=pre, out=torch.full((64,), 3.0, dtype=dt))
        code, off, st = _lib.dtype_code(dt), dy.element_size(), _stream()
        assert lib.pm_dgelu(b.ptr("dy"), b.ptr("pre"), b.ptr("out"), code, 62, st) == _lib.PM_ESHAPE       # n & 3
        assert lib.pm_dgelu(b.ptr("dy"), b.ptr("pre"), b.ptr("out"), code, 0, st) == _lib.PM_ESHAPE
        for k in range(3):                                                                                  # not 8-byte aligned
            ptrs = [b.ptr(x) + (off if j == k else 0) for j, x in enumerate(("dy", "pre", "out"))]
            assert lib.pm_dgelu(*ptrs, code, 60, st) == _lib.PM_EALIGN, k
            ptrs[k] = None
            assert lib.pm_dgelu(*ptrs, code, 60, st) == _lib.PM_EINVAL, k
        assert bool((b["out"] == 3.0).all()) and b.guards_intact()


@pytest.mark.parametrize("in_place", (False, True), ids=["out", "in_place"])
@pytest.mark.parametrize("n", C.SCALE_SIZES)
def test_scale(n, in_place):
    lib = _lib.load()
    x = C.stats_input(n, seed=3)
    b = Bufs(x=x, s=torch.tensor([-0.3]), out=torch.full((n,), 3.0))
    dst = "x" if in_place else "out"
    _lib.check(lib.pm_scale(b.ptr("x"), b.ptr("s"), b.ptr(dst), n, _stream()), "pm_scale")
    assert torch.equal(b[dst], x.to(DEV) * b["s"])
    assert in_place or same_bits(b["x"], x.to(DEV))
    assert float(b["s"]) == float(torch.tensor(-0.3)) and b.guards_intact()
