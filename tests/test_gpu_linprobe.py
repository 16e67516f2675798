"""The linear-probe kernels (csrc/pm_probe.hip) and what is built on them, on the device: head forward / cross-entropy / backward,
running statistics, pool + fc_norm against the float64 restatements and element-wise bounds of tests/probe_ref.py (held to f32
emulations and to wrong variants by tests/test_linprobe_cpu.py); LARS against the trajectories the reference itself recorded
(tests/golden/linprobe.npz) at the 2e-5 rel-L2 this suite applies to optimiser trajectories; the probe model against the existing
head=False classifier; main_linprobe end to end.  Every kernel is compared on the operands it saw.  Outputs lie between guard
regions that are checked afterwards.  Each test prints its largest err / bound per output (`pytest -s`)."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import probe_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32
GUARD, FILL = 64, 12345.0
TRAJ_TOL = 2e-5   # tests/test_gpu_finetune_schedule.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def fx(golden):
    return golden("linprobe.npz")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def abi(name, *args):
    from ssl4polyp_amd import _lib
    return getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream())


def _guarded(shape, dtype=f32, init=None):
    """A tensor that is a slice of a larger buffer: GUARD elements of FILL in front and behind (16-byte aligned); NaN-filled (floats)
    or -1 (integers) unless `init` is given."""
    n = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if init is not None:
        view.copy_(init)
    else:
        view.fill_(float("nan") if dtype.is_floating_point else -1)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_hold(buf, what):
    assert bool((buf[:GUARD] == FILL).all()), what + ": written in front of the buffer"
    assert bool((buf[-GUARD:] == FILL).all()), what + ": written behind the buffer"


def _report(r, what):
    for k, v in r.items():
        print(f"{what} {k}: err/bound {v:.3f}")
    for k, v in r.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of its bound"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------- head forward / CE / backward
HEAD = [(2, 64, 1), (2, 64, 2), (3, 64, 5), (3, 768, 7), (64, 64, 2), (64, 768, 1000), (65, 64, 7), (65, 768, 2), (64, 1280, 5),
        (65, 1280, 1000), (3, 1280, 2), (2, 768, 1000)]


@functools.lru_cache(maxsize=None)
def _head_case(case):
    """Operands on the device: one constant feature column (sums of 0.75 are exact: zero variance), and for C >= 2 a last class whose
    bias keeps it from ever being the arg-max although it is a target."""
    B, D, C = case
    g = _gen(B * 7 + D + C)
    feat = torch.randn(B, D, generator=g) * 1.5 + 0.3
    feat[:, 5] = 0.75
    W = torch.randn(C, D, generator=g) * (1.0 / D ** 0.5)
    bias = torch.randn(C, generator=g) * 0.1
    target = torch.randint(0, C, (B,), generator=g)
    if C >= 2:
        bias[C - 1] = -40.0
        target[0] = C - 1
    rm, rv = torch.randn(D, generator=g) * 0.2, torch.rand(D, generator=g) + 0.5
    return tuple(t.to(DEV) for t in (feat, W, bias, rm, rv, target))


def _head_forward(case, training, what, feat=None):
    B, D, C = case
    f0, W, bias, rm0, rv0, _ = _head_case(case)
    feat = f0 if feat is None else feat
    bufs = {"xhat": _guarded((B, D)), "logits": _guarded((B, C)), "rm": _guarded((D,), init=rm0), "rv": _guarded((D,), init=rv0),
            "tracked": _guarded((1,), torch.int64, init=torch.tensor([3]))}
    o = {n: v for n, (_, v) in bufs.items()}
    st = abi("pm_probe_head_fwd", feat, B, D, C, W, bias, o["rm"], o["rv"], o["tracked"], 1 if training else 0, 0.1, 1e-6, o["xhat"],
             o["logits"])
    torch.cuda.synchronize()
    for n, (buf, _) in bufs.items():
        _guards_hold(buf, f"{what} {n}")
    return st, o


@pytest.mark.parametrize("case", HEAD)
def test_head_forward_ce_backward(case):
    B, D, C = case
    feat, W, bias, rm0, rv0, target = _head_case(case)
    what = f"probe head {case}"
    st, o = _head_forward(case, True, what)
    assert st == 0
    ref = P.head_fwd_train(feat, W, bias, rm0, rv0)
    r = {"xhat": P.ratio(o["xhat"], ref["xhat"], ref["e_xhat"]), "logits": P.ratio(o["logits"], ref["logits"], ref["e_logits"]),
         "running_mean": P.ratio(o["rm"], ref["running_mean"], ref["e_running_mean"]),
         "running_var": P.ratio(o["rv"], ref["running_var"], ref["e_running_var"])}
    assert bool((o["xhat"][:, 5] == 0).all()), "the constant column has zero variance: xhat is exactly 0"
    assert int(o["tracked"]) == 4
    # cross-entropy on the logits the kernel produced
    logits = o["logits"]
    scale = torch.tensor(0.5, device=DEV)
    lb, loss = _guarded((1,))
    db, dl = _guarded((B, C))
    cb, correct = _guarded((2,), torch.int64)
    size = ctypes.c_size_t(0)
    from ssl4polyp_amd import _lib
    assert _lib.load().pm_probe_ce_workspace(B, ctypes.byref(size)) == 0 and size.value == 8 * B
    wb, ws = _guarded((2 * B,))
    assert abi("pm_probe_ce", logits, target, B, C, scale, loss, dl, correct, ws, ws.numel() * 4) == 0
    torch.cuda.synchronize()
    for buf, n in ((lb, "loss"), (db, "dlogits"), (cb, "correct"), (wb, "workspace")):
        _guards_hold(buf, f"{what} {n}")
    c = P.ce(logits, target, 0.5)
    r["loss"] = P.ratio(loss[0], c["loss"], c["e_loss"])
    r["dlogits"] = P.ratio(dl, c["dlogits"], c["e_dlogits"])
    assert correct.tolist() == [c["correct1"], c["correctk"]]
    k = min(5, C)
    srt = logits.sort(1, descending=True).values[:, :min(6, C)]
    assert bool((srt[:, :-1] != srt[:, 1:]).all()) or C == 1, "ties among the top six logits"
    top = logits.topk(k, 1).indices   # the second witness
    assert correct.tolist() == [int((top[:, 0] == target).sum()), int((top == target[:, None]).any(1).sum())]
    if C >= 2:
        assert not bool((logits.argmax(1) == C - 1).any()) and bool((target == C - 1).any())
        assert correct[0].item() < B
    # the same call without a gradient leaves dlogits alone and gives the same loss and counts
    lb2, loss2 = _guarded((1,))
    cb2, correct2 = _guarded((2,), torch.int64)
    assert abi("pm_probe_ce", logits, target, B, C, None, loss2, None, correct2, ws, ws.numel() * 4) == 0
    assert torch.equal(loss, loss2) and torch.equal(correct, correct2)
    # backward into prior contents, twice: the += of gradient accumulation
    prior_w, prior_b = (torch.randn(C, D, generator=_gen(5)) * 0.01).to(DEV), (torch.randn(C, generator=_gen(6)) * 0.01).to(DEV)
    gwb, gw = _guarded((C, D), init=prior_w)
    gbb, gb = _guarded((C,), init=prior_b)
    assert abi("pm_probe_head_bwd", dl, o["xhat"], B, D, C, gw, gb) == 0
    torch.cuda.synchronize()
    _guards_hold(gwb, what + " dW")
    _guards_hold(gbb, what + " dbias")
    b = P.head_bwd(dl, o["xhat"], prior_w, prior_b)
    r["dW"] = P.ratio(gw, b["dW"], P.sum_bound(b["n"], b["t_dW"]))
    r["dbias"] = P.ratio(gb, b["dbias"], P.sum_bound(b["n"], b["t_dbias"]))
    once_w, once_b = gw.clone(), gb.clone()
    assert abi("pm_probe_head_bwd", dl, o["xhat"], B, D, C, gw, gb) == 0
    b2 = P.head_bwd(dl, o["xhat"], once_w, once_b)
    r["dW twice"] = P.ratio(gw, b2["dW"], P.sum_bound(b2["n"], b2["t_dW"]))
    r["dbias twice"] = P.ratio(gb, b2["dbias"], P.sum_bound(b2["n"], b2["t_dbias"]))
    _report(r, what)


@pytest.mark.parametrize("case", [(1, 64, 2), (3, 768, 7), (65, 1280, 1000)])
def test_head_eval_mode(case):
    B, D, C = case
    feat, W, bias, rm0, rv0, _ = _head_case(case)
    st, o = _head_forward(case, False, f"probe head eval {case}")
    assert st == 0
    assert torch.equal(o["rm"], rm0) and torch.equal(o["rv"], rv0) and int(o["tracked"]) == 3, "eval mode updates nothing"
    ref = P.head_fwd_eval(feat, W, bias, rm0, rv0)
    _report({"xhat": P.ratio(o["xhat"], ref["xhat"], ref["e_xhat"]), "logits": P.ratio(o["logits"], ref["logits"], ref["e_logits"])},
            f"probe head eval {case}")


def test_training_mode_refuses_one_sample():
    """B = 1: torch.nn.BatchNorm1d raises in training mode; the C entry refuses before any launch, the binding raises ValueError."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.probe import ProbeHead
    st, o = _head_forward((1, 64, 2), True, "B = 1")
    assert st == _lib.PM_ESHAPE
    assert bool(torch.isnan(o["xhat"]).all()) and bool(torch.isnan(o["logits"]).all()) and int(o["tracked"]) == 3
    head = ProbeHead(torch.nn.Linear(64, 2)).to(DEV)
    x = torch.randn(1, 64, device=DEV)
    with pytest.raises(ValueError):
        head.train()(x)
    assert int(head[0].num_batches_tracked) == 0
    assert head.eval()(x).shape == (1, 2)
    with pytest.raises(ValueError):   # as torch does
        torch.nn.BatchNorm1d(64, affine=False).train()(x.cpu())
    with pytest.raises(_lib.PolypMaeError):   # no gradient with respect to the features
        head.train()(torch.randn(4, 64, device=DEV, requires_grad=True))


def test_running_statistics_over_six_steps():
    from ssl4polyp_amd.probe import ProbeHead
    B, D, C = 16, 64, 7
    g = _gen(21)
    head = ProbeHead(torch.nn.Linear(D, C)).to(DEV)
    feats = [(torch.randn(B, D, generator=g) * (1 + 0.2 * i) + 0.1 * i).to(DEV) for i in range(6)]
    rm, rv = torch.zeros(D, dtype=torch.float64, device=DEV), torch.ones(D, dtype=torch.float64, device=DEV)
    e_rm, e_rv = torch.zeros_like(rm), torch.zeros_like(rv)
    head.train()
    with torch.no_grad():
        for x in feats:
            head(x)
            s = P.bn_train(x)
            (rm, e1), (rv, e2) = P.running_update(rm, s["mean"], s["e_mean"]), P.running_update(rv, s["var_unbiased"], s["e_var_unbiased"])
            e_rm, e_rv = 0.9 * e_rm + e1, 0.9 * e_rv + e2   # the error already in the buffer shrinks by 1 - momentum
    bn = head[0]
    _report({"running_mean": P.ratio(bn.running_mean, rm, e_rm), "running_var": P.ratio(bn.running_var, rv, e_rv)}, "six steps")
    assert int(bn.num_batches_tracked) == 6 and bn.num_batches_tracked.dtype == torch.int64
    # eval-mode logits use them, and change nothing
    keep = (bn.running_mean.clone(), bn.running_var.clone())
    head.eval()
    with torch.no_grad():
        out = head(feats[0])
        ref = P.head_fwd_eval(feats[0], head[1].weight, head[1].bias, *keep)
        assert P.ratio(out, ref["logits"], ref["e_logits"]) <= 1.0
        assert torch.equal(bn.running_mean, keep[0]) and torch.equal(bn.running_var, keep[1]) and int(bn.num_batches_tracked) == 6
        # a training-mode call afterwards changes the eval results only through the documented update
        head.train()
        head(feats[1])
        s = P.bn_train(feats[1])
        want_m, e_m = P.running_update(keep[0], s["mean"], s["e_mean"])
        want_v, e_v = P.running_update(keep[1], s["var_unbiased"], s["e_var_unbiased"])
        assert P.ratio(bn.running_mean, want_m, e_m) <= 1.0 and P.ratio(bn.running_var, want_v, e_v) <= 1.0
        assert int(bn.num_batches_tracked) == 7
        head.eval()
        ref = P.head_fwd_eval(feats[0], head[1].weight, head[1].bias, bn.running_mean, bn.running_var)
        assert P.ratio(head(feats[0]), ref["logits"], ref["e_logits"]) <= 1.0
    # the module's state loads strictly into torch's own modules, whose eval output is the same map
    tref = torch.nn.Sequential(torch.nn.BatchNorm1d(D, affine=False, eps=1e-6), torch.nn.Linear(D, C))
    tref.load_state_dict({k: v.cpu() for k, v in head.state_dict().items()}, strict=True)
    with torch.no_grad():
        want = tref.double().eval()(feats[0].cpu().double())
    with torch.no_grad():
        assert P.ratio(head(feats[0]), want.to(DEV), ref["e_logits"]) <= 1.0


# ---------------------------------------------------------------------------------------------------- pool + fc_norm
@pytest.mark.parametrize("B,N,D", [(2, 197, 768), (3, 50, 768), (2, 257, 1280), (1, 2, 64)])
def test_pool_norm(B, N, D):
    from ssl4polyp_amd import _lib
    g = _gen(N + D)
    x = torch.randn(B, N, D, generator=g) * 2.0 + 0.5
    x[:, 0] = 1e4 * torch.randn(B, D, generator=g)   # the cls row: excluded from the mean
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    x, gamma, beta = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    size = ctypes.c_size_t(0)
    assert _lib.load().pm_pool_norm_workspace(B, N, D, ctypes.byref(size)) == 0
    wb, ws = _guarded((size.value // 4,))
    fb, feat = _guarded((B, D))
    assert abi("pm_pool_norm_fwd", x, B, N, D, gamma, beta, 1e-6, feat, ws, size.value) == 0
    torch.cuda.synchronize()
    _guards_hold(wb, "pool_norm workspace")
    _guards_hold(fb, "pool_norm feat")
    ref = P.pool_norm(x, gamma, beta)
    _report({"feat": P.ratio(feat, ref["feat"], ref["e_feat"])}, f"pool_norm {(B, N, D)}")
    # refusals before any launch
    fb2, feat2 = _guarded((B, D))
    assert abi("pm_pool_norm_fwd", x, B, 1, D, gamma, beta, 1e-6, feat2, ws, size.value) == _lib.PM_ESHAPE
    assert abi("pm_pool_norm_fwd", x, B, N, D, gamma, beta, 1e-6, feat2, ws, size.value - 4) == _lib.PM_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(feat2).all())


# ---------------------------------------------------------------------------------------------------- LARS
def _device_run(run, record=True):
    """The recorded schedule on the device: ProbeHead -> probe_ce -> backward -> FusedLARS over the head's two tensors and the two
    planted matrices, in f32.  -> per micro-step dict of the fixture's names."""
    from ssl4polyp_amd.optim import FusedLARS
    from ssl4polyp_amd.probe import ProbeHead, probe_ce
    from ssl4polyp_amd.train import adjust_learning_rate
    C, D = run["W0"].shape
    head = ProbeHead(torch.nn.Linear(D, C)).to(DEV)
    with torch.no_grad():
        head[1].weight.copy_(run["W0"].float())
        head[1].bias.copy_(run["b0"].float())
    zero = torch.nn.Parameter(torch.zeros(run["zero_grad"].shape, device=DEV))
    still = torch.nn.Parameter(run["still0"].float().to(DEV))
    named = [("head.1.weight", head[1].weight), ("head.1.bias", head[1].bias), ("zero", zero), ("still", still)]
    opt = FusedLARS([p for _, p in named], lr=run["lr0"], weight_decay=run["wd"])
    args = types.SimpleNamespace(lr=run["lr0"], min_lr=run["min_lr"], warmup_epochs=run["warmup"], epochs=run["epochs"])
    accum = run["accum"]
    scale = torch.full((), 1.0 / accum, device=DEV)
    feats, targets = run["feats"].float().to(DEV), run["targets"].to(DEV)
    zg = (run["zero_grad"] / accum).float().to(DEV)
    head.train()
    out = []
    for it in range(run["steps"]):
        epoch, step = divmod(it, run["per_epoch"])
        if step % accum == 0:
            adjust_learning_rate(opt, step / run["per_epoch"] + epoch, args)
        loss, correct = probe_ce(head(feats[step % len(feats)]), targets[step % len(feats)], scale)
        loss.backward()
        zero.grad = zg.clone() if zero.grad is None else zero.grad + zg
        if still.grad is None:
            still.grad = torch.zeros_like(still)
        if (step + 1) % accum == 0:
            opt.step()
            opt.zero_grad(set_to_none=True)
        rec = dict(loss=loss.detach().clone(), lr=opt.param_groups[0]["lr"], acc1=int(correct[0]), acc5=int(correct[1]),
                   running_mean=head[0].running_mean.clone(), running_var=head[0].running_var.clone(),
                   tracked=int(head[0].num_batches_tracked))
        for n, p in named:
            rec[n] = p.detach().clone()
            mu = opt.state[p].get("mu")
            rec["mu." + n] = mu.clone() if mu is not None else torch.zeros_like(p)
        out.append(rec)
    return out, opt


@pytest.mark.parametrize("name", ["c2_wd0", "c2_wd5", "c7_wd0", "c7_wd5", "vitb"])
def test_lars_follows_the_recorded_trajectories(fx, name):
    run = P.fixture_run(fx, name)
    got, opt = _device_run(run)
    worst = {}
    for it, rec in enumerate(got):
        assert rec["lr"] == float(run["lr"][it]) and rec["tracked"] == int(run["tracked"][it])
        assert (rec["acc1"], rec["acc5"]) == (int(run["acc1"][it]), int(run["acc5"][it]))
        for k in list(P.PARAMS) + ["mu." + n for n in P.PARAMS] + ["running_mean", "running_var", "loss"]:
            want = run[k][it].to(DEV)
            if float(want.abs().max()) == 0.0:   # the zero-norm branches: the reference's zeros, exactly
                assert float(rec[k].abs().max()) == 0.0, (name, it, k)
                continue
            e = rel_l2(rec[k], want)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= TRAJ_TOL, (name, it, k, e)
    for k, v in worst.items():
        print(f"{name} {k}: worst rel-L2 {v:.2e}")
    # the two zero-norm branches (lars.py:36-39) give the reference's values
    first = int(np.flatnonzero(run["updated"].numpy())[0])
    assert rel_l2(got[first]["mu.zero"], run["zero_grad"].to(DEV)) <= 1e-7   # q = 1 on the all-zero matrix: mu = g
    if run["wd"] == 0.0:
        assert torch.equal(got[-1]["still"], run["still0"].float().to(DEV)), "a zero update with q = 1 moves nothing"
    # state_dict: the reference's layout, and it round-trips
    sd = opt.state_dict()
    assert sorted(sd["param_groups"][0].keys()) == [str(k) for k in fx["optim_group_keys"]]
    assert sorted({k for st in sd["state"].values() for k in st}) == [str(k) for k in fx["optim_state_keys"]] == ["mu"]
    from ssl4polyp_amd.optim import FusedLARS
    clone = [torch.nn.Parameter(p.detach().clone()) for g in opt.param_groups for p in g["params"]]
    opt2 = FusedLARS(clone, lr=0.0)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] and opt2.param_groups[0]["weight_decay"] == run["wd"]
    for a, b in zip(clone, [p for g in opt.param_groups for p in g["params"]]):
        assert torch.equal(opt2.state[a]["mu"], opt.state[b]["mu"])


def test_schedule_twice_gives_identical_bits(fx):
    run = P.fixture_run(fx, "c7_wd5")
    a, _ = _device_run(run)
    b, _ = _device_run(run)
    for ra, rb in zip(a, b):
        for k, v in ra.items():
            assert torch.equal(v, rb[k]) if torch.is_tensor(v) else v == rb[k], k


def _lars_call(segs, hyper):
    from ssl4polyp_amd import _lib
    lib = _lib.load()
    arr = (_lib.LarsSegment * len(segs))(*[_lib.LarsSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel(), mat)
                                           for p, g, m, mat in segs])
    size = ctypes.c_size_t(0)
    assert lib.pm_lars_workspace(len(segs), ctypes.byref(size)) == 0
    wb, ws = _guarded((size.value // 8,), torch.float64)
    st = lib.pm_lars_step(arr, len(segs), hyper.data_ptr(), ws.data_ptr(), size.value, _stream())
    torch.cuda.synchronize()
    _guards_hold(wb, "lars workspace")
    return st


def test_lars_segment_table_equals_single_calls():
    """Five tensors of unequal lengths at unaligned (4-byte) addresses inside one guarded buffer, the smallest of 1 element, matrices
    and vectors mixed: one call over the table = five calls of one segment, bit for bit; against the restatement within its bound."""
    from ssl4polyp_amd import _lib
    sizes = [(1, 0), (7, 1), (130, 1), (1025, 0), (33333, 1)]   # (numel, is_matrix)
    total = sum(n + 1 for n, _ in sizes)                        # one element between neighbours: odd offsets
    g = _gen(33)
    src = {k: torch.randn(total, generator=g).to(DEV) * s for k, s in (("p", 1.0), ("g", 0.1), ("mu", 0.01))}
    hyper = torch.tensor([0.3, 0.05, 0.9, 0.001], device=DEV)

    def table():
        bufs = {k: _guarded((total,), init=v) for k, v in src.items()}
        segs, o = [], 1
        for n, mat in sizes:
            segs.append(tuple(bufs[k][1][o:o + n] for k in ("p", "g", "mu")) + (mat,))
            o += n + 1
        assert any(s[0].data_ptr() % 16 for s in segs)
        return bufs, segs

    bufs_a, segs_a = table()
    assert _lars_call(segs_a, hyper) == 0
    bufs_b, segs_b = table()
    for s in segs_b:
        assert _lars_call([s], hyper) == 0
    for k in ("p", "g", "mu"):
        _guards_hold(bufs_a[k][0], "lars table " + k)
        assert torch.equal(bufs_a[k][1], bufs_b[k][1]), k
    assert torch.equal(bufs_a["g"][1], src["g"])
    o = 1
    for (n, mat), (p, _, mu, _) in zip(sizes, segs_a):
        ref = P.lars_step(src["p"][o:o + n], src["g"][o:o + n], src["mu"][o:o + n], bool(mat), 0.3, 0.05)
        _report({"p": P.ratio(p, ref["p"], ref["e_p"]), "mu": P.ratio(mu, ref["mu"], ref["e_mu"])}, f"lars segment n = {n}")
        assert torch.equal(bufs_a["p"][1][o + n:o + n + 1], src["p"][o + n:o + n + 1]), "the element between two segments"
        o += n + 1
    # refusals before any launch
    p, gr, mu, _ = segs_a[2]
    keep = p.clone()
    arr = (_lib.LarsSegment * 1)(_lib.LarsSegment(p.data_ptr(), gr.data_ptr(), mu.data_ptr(), 0, 1))
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    assert _lib.load().pm_lars_step(arr, 1, hyper.data_ptr(), ws.data_ptr(), 512, _stream()) == _lib.PM_ESHAPE
    arr = (_lib.LarsSegment * 1)(_lib.LarsSegment(p.data_ptr(), gr.data_ptr(), mu.data_ptr(), 130, 1))
    assert _lib.load().pm_lars_step(arr, 1, hyper.data_ptr(), ws.data_ptr(), 8, _stream()) == _lib.PM_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(p, keep)


def test_lars_step_captured_follows_the_device_lr():
    """The hyper-parameters are read from the device record: a captured step replays with an lr written between replays, and
    gives the bits of the eager step."""
    from ssl4polyp_amd.optim import FusedLARS
    g = _gen(41)
    init = [torch.randn(7, 64, generator=g), torch.randn(7, generator=g)]
    grads = [torch.randn(7, 64, generator=g) * 0.1, torch.randn(7, generator=g) * 0.1]

    def make():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone().to(DEV)
        return ps, FusedLARS(ps, lr=0.1, weight_decay=0.05)

    eager, opt_e = make()
    graphed, opt_g = make()
    opt_e.step()
    opt_g.step()   # (the segment table and the device record exist before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    for lr in (0.3, 0.05):
        for opt in (opt_e, opt_g):
            opt.param_groups[0]["lr"] = lr
        opt_e.step()
        opt_g.sync_hyper()
        graph.replay()
    torch.cuda.synchronize()   # (a capture records the launches without running them: both sides took three steps)
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b) and torch.equal(opt_e.state[a]["mu"], opt_g.state[b]["mu"])
        assert not torch.equal(a.detach().cpu(), init[0] if a.ndim > 1 else init[1])


# ---------------------------------------------------------------------------------------------------- module level
@pytest.fixture(scope="module")
def vitb():
    """The ViT-B probe model (bf16 encoder, cls token, 2 classes) and the existing head=False classifier on the same weights."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd import models_vit
    torch.manual_seed(7)
    model = models_vit.vit_base_patch16(num_classes=2, global_pool=False)
    torch.nn.init.trunc_normal_(model.head.weight, std=0.01)
    models_vit.add_probe_head(model)
    model.to(DEV)
    old = A.VisionTransformer_from_Any(False, 2, True, None, 768, 12, 12, "cls")
    own = model.state_dict()
    missing, unexpected = old.load_state_dict({k: v for k, v in own.items() if not k.startswith("head.")}, strict=False)
    assert not missing and not unexpected
    old.to(DEV).eval()
    imgs = torch.randn(8, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    return model, old, imgs


def test_probe_model_equals_head_on_existing_features(vitb):
    from ssl4polyp_amd.probe import probe_head_fwd
    model, old, imgs = vitb
    assert [k for k in model.state_dict() if k.startswith("head.")] == \
        ["head.0.running_mean", "head.0.running_var", "head.0.num_batches_tracked", "head.1.weight", "head.1.bias"]
    assert sorted(n for n, p in model.named_parameters() if p.requires_grad) == ["head.1.bias", "head.1.weight"]
    model.eval()
    with torch.no_grad():
        got = model(imgs)
        feat = old(imgs)
        bn = model.head[0]
        want, _ = probe_head_fwd(feat, model.head[1].weight.detach(), model.head[1].bias.detach(), bn.running_mean, bn.running_var,
                                 bn.num_batches_tracked, False)
    assert got.shape == (8, 2) and torch.equal(got, want), "the probe model's encoder pass is the existing head=False pass"
    assert torch.equal(model.forward_features(imgs), feat)


def test_three_steps_touch_nothing_but_the_head(vitb):
    from ssl4polyp_amd.optim import FusedLARS
    from ssl4polyp_amd.probe import probe_ce
    model, _, imgs = vitb
    model.train()
    f = model._rt.flat
    inside = {r: torch.zeros(f.P[r].numel(), dtype=torch.bool, device=DEV) for r in f.P}
    for n in ("head.1.weight", "head.1.bias"):
        i = f.index[n]
        inside[f.region[i]][f.offset[i]:f.offset[i] + f.numel[i]] = True
    before = {r: (f.P[r].clone(), f.G[r].clone()) for r in f.P}
    head_before = {n: f.param_view(n).clone() for n in ("head.1.weight", "head.1.bias")}
    opt = FusedLARS(model.head.parameters(), lr=0.5)
    target = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=DEV)
    for _ in range(3):
        loss, _ = probe_ce(model(imgs), target)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
    torch.cuda.synchronize()
    for r in f.P:
        out = ~inside[r]
        assert torch.equal(f.P[r][out], before[r][0][out]), f"parameters outside head.1.* changed ({r})"
        assert torch.equal(f.G[r][out], before[r][1][out]), f"flat gradients outside head.1.* changed ({r})"
    for n, v in head_before.items():
        assert not torch.equal(f.param_view(n), v), n + " did not train"
    assert all(p.grad is None for n, p in model.named_parameters() if not n.startswith("head.1."))
    # the model's state loads strictly into torch's own head under the `head.` prefix
    D = 768
    tref = torch.nn.Sequential(torch.nn.BatchNorm1d(D, affine=False, eps=1e-6), torch.nn.Linear(D, 2))
    tref.load_state_dict({k[5:]: v.cpu() for k, v in model.state_dict().items() if k.startswith("head.")}, strict=True)
    model.eval()
    with torch.no_grad():
        feat = model.forward_features(imgs)
        got = model(imgs)
        want = tref.double().eval()(feat.cpu().double()).to(DEV)
        bn = model.head[0]
        ref = P.head_fwd_eval(feat, model.head[1].weight, model.head[1].bias, bn.running_mean, bn.running_var)
    assert P.ratio(got, want, ref["e_logits"]) <= 1.0


def test_global_pool_features():
    """A small global_pool model: fc_norm replaces norm in the state dict, and the features are pm_pool_norm_fwd of the block stack's
    output (within the bound of the restatement on the tokens the engine produced)."""
    from ssl4polyp_amd import models_vit
    torch.manual_seed(11)
    model = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=3, global_pool=True, precision="fp32")
    keys = set(model.state_dict())
    assert {"fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"} <= keys and not any(k.startswith("norm.") for k in keys)
    with torch.no_grad():
        model.fc_norm.weight.normal_(1.0, 0.2)
        model.fc_norm.bias.normal_(0.0, 0.2)
    models_vit.add_probe_head(model).to(DEV).eval()
    imgs = torch.randn(3, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    tokens = model.forward_tokens(imgs)
    assert tokens.shape == (3, 197, 64)
    feat = model.forward_features(imgs)
    ref = P.pool_norm(tokens, model.fc_norm.weight.detach(), model.fc_norm.bias.detach())
    _report({"feat": P.ratio(feat, ref["feat"], ref["e_feat"])}, "global_pool features")
    assert model(imgs).shape == (3, 3)


def test_pretrain_checkpoint_loading():
    """main_linprobe.py:216-240: the decoder's keys are unexpected, the head's are missing, head.weight is re-drawn; another grid is refused."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd import _lib, models_vit
    mae = A.MaskedAutoencoderViT(embed_dim=64, depth=2, num_heads=2, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2)
    ckpt = {k: v.clone() for k, v in mae.state_dict().items()}
    model = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=2)
    msg = models_vit.load_pretrained_for_probe(model, ckpt)
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} and all("decoder" in k or k == "mask_token" for k in msg.unexpected_keys)
    assert torch.equal(model.blocks[1].mlp.fc2.weight, mae.blocks[1].mlp.fc2.weight) and float(model.head.weight.abs().max()) > 0
    assert 0.005 < float(model.head.weight.std()) < 0.015   # trunc-normal std 0.01
    pooled = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=2, global_pool=True)
    ckpt_np = {k: v for k, v in ckpt.items() if not k.startswith("norm.")}
    with pytest.raises(AssertionError):
        models_vit.load_pretrained_for_probe(pooled, ckpt_np | {"fc_norm.weight": torch.ones(64)})
    ckpt["pos_embed"] = torch.zeros(1, 50, 64)
    with pytest.raises(_lib.PolypMaeError):
        models_vit.load_pretrained_for_probe(model, ckpt)


# ---------------------------------------------------------------------------------------------------- end to end
def _write_folder(root, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for split in ("train", "val"):
        for c in range(2):
            d = os.path.join(root, split, f"class{c}")
            os.makedirs(d)
            for i in range(8):
                h, w = int(rng.integers(260, 340)), int(rng.integers(260, 340))
                base = np.full((h, w, 3), 60 + 120 * c, dtype=np.float64) + rng.normal(0, 25, (h, w, 3))
                Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).save(os.path.join(d, f"{i}.jpg"), quality=90)


def test_main_linprobe_end_to_end(tmp_path, monkeypatch):
    """2 classes x 8 small JPEGs, 2 epochs, accum_iter 2: a checkpoint per epoch; resuming from the first continues exactly as the
    uninterrupted run; --eval on the last reports the last epoch's accuracy."""
    from ssl4polyp_amd import main_linprobe, models_vit
    monkeypatch.setattr(models_vit, "vit_test_patch16", functools.partial(models_vit.VisionTransformer, embed_dim=64, depth=2, num_heads=2),
                        raising=False)
    data = tmp_path / "data"
    _write_folder(str(data), 0)

    def args(out, **kw):
        a = main_linprobe.get_args_parser().parse_args(
            ["--model", "vit_test_patch16", "--batch_size", "4", "--epochs", "2", "--accum_iter", "2", "--warmup_epochs", "1",
             "--nb_classes", "2", "--data_path", str(data), "--output_dir", str(out), "--num_workers", "0", "--blr", "10.0",
             "--precision", "fp32", "--seed", "3"])
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    torch.manual_seed(1)
    pre = models_vit.VisionTransformer(embed_dim=64, depth=2, num_heads=2, num_classes=2)
    ckpt = tmp_path / "pretrain.pth"
    torch.save({"model": {k: v for k, v in pre.state_dict().items() if not k.startswith("head.")}}, ckpt)
    model, opt, hist = main_linprobe.run(args(tmp_path / "a", finetune=str(ckpt)))
    assert [h["epoch"] for h in hist] == [0, 1] and all(np.isfinite(h["train"]["loss"]) for h in hist)
    assert hist[0]["train"]["samples"] == 16 and hist[0]["test"]["samples"] == 16
    first, last = tmp_path / "a" / "ckpts" / "checkpoint-0.pth", tmp_path / "a" / "ckpts" / "checkpoint-1.pth"
    assert first.exists() and last.exists()
    saved = torch.load(str(last), map_location="cpu", weights_only=False)
    assert {"model", "optimizer", "epoch", "scaler", "args"} <= set(saved) and "head.0.running_var" in saved["model"]
    assert int(saved["model"]["head.0.num_batches_tracked"]) == 8
    # resume from the first epoch's checkpoint: the second epoch is the uninterrupted run's
    model_b, opt_b, hist_b = main_linprobe.run(args(tmp_path / "b", resume=str(first), finetune=str(ckpt)))
    assert [h["epoch"] for h in hist_b] == [1]
    assert hist_b[0]["train"] == {**hist[1]["train"], "seconds": hist_b[0]["train"]["seconds"]} and hist_b[0]["test"] == hist[1]["test"]
    for (k, a), b in zip(model.state_dict().items(), model_b.state_dict().values()):
        assert torch.equal(a, b), k
    # --eval reports the last epoch's accuracy
    _, _, ev = main_linprobe.run(args(tmp_path / "c", resume=str(last), eval=True))
    assert ev[0]["test"]["acc1"] == hist[1]["test"]["acc1"] and ev[0]["test"]["loss"] == hist[1]["test"]["loss"]
