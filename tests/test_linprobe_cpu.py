"""Linear probe, CPU side: the float64 restatements of tests/probe_ref.py reproduce every value the reference itself recorded
(tests/golden/linprobe.npz: its LARS, torch's BatchNorm1d + Linear + CrossEntropyLoss, its lr schedule, its crop sampler) to 1e-12
relative, the tolerance of this suite for float64 against float64; the host restatements of the package (schedule, accumulation
boundaries, box sampler, state-dict key lists) match exactly; and every element-wise bound of probe_ref holds for an f32 emulation
of the kernel's arithmetic and rejects the wrong variants a probe implementation is likely to ship."""
import numpy as np
import pytest
import torch

import probe_ref as P

f32 = torch.float32
RUNS = ("c2_wd0", "c2_wd5", "c7_wd0", "c7_wd5", "vitb")
TOL64 = 1e-12


@pytest.fixture(scope="module")
def fx(golden):
    return golden("linprobe.npz")


def _rel(got, want):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------------- the recorded reference run
@pytest.mark.parametrize("name", RUNS)
def test_restatement_reproduces_the_reference(fx, name):
    run = P.fixture_run(fx, name)
    n = 0
    for it, got in enumerate(P.replay(run)):
        for k, v in got.items():
            want = run[k][it]
            if k in ("acc1", "acc5", "tracked", "updated"):
                assert int(v) == int(want), (name, it, k)
            elif k == "lr":
                assert float(v) == float(want), (name, it, k)   # the schedule is the same host arithmetic: exact
            else:
                assert _rel(v, want) <= TOL64, (name, it, k, _rel(v, want))
        n += 1
    assert n == run["steps"]


def test_zero_norm_branches_are_taken(fx):
    """lars.py:36-39: the all-zero matrix keeps q = 1 (its mu is the plain gradient sum), the matrix without gradient and decay
    does not move; with weight decay the second one's update is wd p, so it moves."""
    run = P.fixture_run(fx, "c7_wd0")
    first = int(np.flatnonzero(run["updated"].numpy())[0])
    assert torch.equal(run["mu.zero"][first], run["zero_grad"])              # q = 1: mu = g (two halves of accum_iter 2)
    assert torch.equal(run["still"][-1], run["still0"]) and float(run["mu.still"][-1].abs().max()) == 0.0
    wd = P.fixture_run(fx, "c7_wd5")
    assert not torch.equal(wd["still"][-1], wd["still0"])
    s = P.lars_step(torch.zeros(3, 4), torch.ones(3, 4), torch.zeros(3, 4), True, 0.1, 0.0)
    assert s["q"] == 1.0
    s = P.lars_step(torch.ones(3, 4), torch.zeros(3, 4), torch.zeros(3, 4), True, 0.1, 0.0)
    assert s["q"] == 1.0 and torch.equal(s["p"], torch.ones(3, 4, dtype=torch.float64))


def test_eval_logits(fx):
    for name in RUNS:
        run = P.fixture_run(fx, name)
        e = P.head_fwd_eval(run["feats"][0], run["head.1.weight"][-1], run["head.1.bias"][-1], run["running_mean"][-1],
                            run["running_var"][-1])
        assert _rel(e["logits"], run["eval_logits"]) <= TOL64


# ---------------------------------------------------------------------------------------------------- host restatements
def test_box_sampler_matches_exactly(fx):
    from ssl4polyp_amd.data import draw_linprobe_boxes
    sizes = fx["box_sizes"]
    torch.manual_seed(int(fx["box_seed"]))
    got = [draw_linprobe_boxes(1, int(sizes[n % len(sizes)][1]), int(sizes[n % len(sizes)][0]))[0] for n in range(len(fx["boxes"]))]
    assert np.array_equal(np.stack(got), fx["boxes"])
    # one generator serves a batch in frame order
    g = torch.Generator().manual_seed(3)
    a = draw_linprobe_boxes(4, [224, 480, 500, 300], [224, 640, 333, 200], generator=g)
    g = torch.Generator().manual_seed(3)
    b = np.concatenate([draw_linprobe_boxes(1, h, w, generator=g) for h, w in ((224, 224), (480, 640), (500, 333), (300, 200))])
    assert np.array_equal(a, b)
    assert ((a[:, 2] > 0) & (a[:, 3] > 0) & (a[:, 0] + a[:, 2] <= [224, 480, 500, 300]) & (a[:, 1] + a[:, 3] <= [224, 640, 333, 200])).all()


def test_lr_table_and_accumulation_boundaries(fx):
    """train.linprobe_schedule: the lr in force at every micro-step and the steps that update, against the recorded run."""
    import types
    from ssl4polyp_amd.train import linprobe_schedule
    accum, per_epoch, steps, warmup, epochs = (int(v) for v in fx["schedule"])
    args = types.SimpleNamespace(lr=float(fx["schedule_lr"][0]), min_lr=float(fx["schedule_lr"][1]), warmup_epochs=warmup,
                                 epochs=epochs, accum_iter=accum)
    table = [row for epoch in range(steps // per_epoch) for row in linprobe_schedule(epoch, per_epoch, args)]
    assert [lr for lr, _ in table] == [float(v) for v in fx["c2_wd0.lr"]]
    assert [int(u) for _, u in table] == [int(v) for v in fx["c2_wd0.updated"]]
    assert max(lr for lr, _ in table) == args.lr and table[-1][0] < args.lr   # the run crosses the end of the warm-up


def test_key_lists(fx):
    from ssl4polyp_amd.optim import FusedLARS
    from ssl4polyp_amd.probe import ProbeHead
    head = ProbeHead(torch.nn.Linear(8, 3))
    assert ["head." + k for k in head.state_dict().keys()] == [str(k) for k in fx["model_keys"]]
    ref = torch.nn.Sequential(torch.nn.BatchNorm1d(8, affine=False, eps=1e-6), torch.nn.Linear(8, 3))
    ref.load_state_dict(head.state_dict(), strict=True)
    assert head[0].eps == ref[0].eps and head[0].momentum == ref[0].momentum
    opt = FusedLARS(head[1].parameters(), lr=0.1)
    assert sorted(opt.state_dict()["param_groups"][0].keys()) == [str(k) for k in fx["optim_group_keys"]]
    assert opt.defaults == dict(lr=0.1, weight_decay=0, momentum=0.9, trust_coefficient=0.001)
    # param groups honour lr_scale through the existing adjust_learning_rate, and that is what goes to the device record
    import types
    from ssl4polyp_amd.train import adjust_learning_rate
    opt = FusedLARS([{"params": [head[1].weight], "lr_scale": 0.5}, {"params": [head[1].bias]}], lr=0.1, weight_decay=0.05)
    lr = adjust_learning_rate(opt, 5.0, types.SimpleNamespace(lr=0.4, min_lr=0.0, warmup_epochs=10, epochs=90))
    assert lr == 0.2 and [g["lr"] for g in opt.param_groups] == [0.1, 0.2]
    assert opt._rows() == [(0.1, 0.05, 0.9, 0.001), (0.2, 0.05, 0.9, 0.001)]


# ---------------------------------------------------------------------------------------------------- f32 emulations
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _head_inputs(B, D, C, seed=0):
    g = _gen(seed)
    feat = torch.randn(B, D, generator=g) * 1.5 + 0.3
    feat[:, 3] = 0.75
    W = torch.randn(C, D, generator=g) * 0.05
    bias = torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(D, generator=g) * 0.2, torch.rand(D, generator=g) + 0.5
    target = torch.randint(0, C, (B,), generator=g)
    return feat, W, bias, rm, rv, target


def emu_bn_train(feat, rm, rv, eps=1e-6, momentum=0.1, unbiased_xhat=False, biased_running=False):
    """The kernel's arithmetic in torch f32 (the order of the sums is torch's: the bounds do not depend on it)."""
    B = feat.shape[0]
    mean = feat.sum(0) / f32_(B)
    q = ((feat - mean) ** 2).sum(0)
    rstd = torch.rsqrt(q / f32_(B - 1 if unbiased_xhat else B) + f32_(eps))
    xhat = (feat - mean) * rstd
    new_rm = f32_(1 - momentum) * rm + f32_(momentum) * mean
    new_rv = f32_(1 - momentum) * rv + f32_(momentum) * (q / f32_(B if biased_running else B - 1))
    return mean, rstd, xhat, new_rm, new_rv


def f32_(v):
    return torch.tensor(v, dtype=f32)


def emu_ce(logits, target, scale):
    B = logits.shape[0]
    m = logits.max(1, keepdim=True).values
    e = torch.exp(logits - m)
    S = e.sum(1, keepdim=True)
    row = (m + torch.log(S)) - logits.gather(1, target[:, None])
    loss = row.sum() / f32_(B)
    g = f32_(scale) / f32_(B)
    onehot = torch.zeros_like(logits).scatter_(1, target[:, None], 1.0)
    return loss, (e * (f32_(1.0) / S) - onehot) * g


def emu_lars(p, g, mu, is_matrix, lr, wd, momentum=0.9, tc=0.001, force_q=True):
    dp = g
    if is_matrix:
        dp = g + f32_(wd) * p
        pn, un = p.double().norm(), dp.double().norm()
        q = (tc * pn / un) if (not force_q or (pn > 0 and un > 0)) else torch.tensor(1.0, dtype=torch.float64)
        dp = dp * q.float()
    mu2 = f32_(momentum) * mu + dp
    return p - f32_(lr) * mu2, mu2


@pytest.mark.parametrize("B,D,C", [(2, 64, 2), (3, 64, 7), (16, 64, 7), (65, 768, 5), (64, 1280, 1000)])
def test_bounds_hold_for_f32_emulation(B, D, C):
    feat, W, bias, rm, rv, target = _head_inputs(B, D, C)
    ref = P.head_fwd_train(feat, W, bias, rm, rv)
    mean, rstd, xhat, new_rm, new_rv = emu_bn_train(feat, rm, rv)
    logits = xhat @ W.T + bias
    r = {"mean": P.ratio(mean, ref["mean"], ref["e_mean"]), "rstd": P.ratio(rstd, ref["rstd"], ref["e_rstd"]),
         "xhat": P.ratio(xhat, ref["xhat"], ref["e_xhat"]), "logits": P.ratio(logits, ref["logits"], ref["e_logits"]),
         "running_mean": P.ratio(new_rm, ref["running_mean"], ref["e_running_mean"]),
         "running_var": P.ratio(new_rv, ref["running_var"], ref["e_running_var"])}
    assert bool((xhat[:, 3] == 0).all()) and bool((ref["xhat"][:, 3] == 0).all())   # the constant column
    ev = P.head_fwd_eval(feat, W, bias, rm, rv)
    xe = (feat - rm) * torch.rsqrt(rv + f32_(1e-6))
    r["eval xhat"] = P.ratio(xe, ev["xhat"], ev["e_xhat"])
    r["eval logits"] = P.ratio(xe @ W.T + bias, ev["logits"], ev["e_logits"])
    c = P.ce(logits, target, 0.5)
    loss, dl = emu_ce(logits, target, 0.5)
    r["loss"] = P.ratio(loss, c["loss"], c["e_loss"])
    r["dlogits"] = P.ratio(dl, c["dlogits"], c["e_dlogits"])
    top = logits.topk(min(5, C), 1).indices
    assert c["correct1"] == int((top[:, 0] == target).sum()) and c["correctk"] == int((top == target[:, None]).any(1).sum())
    dW0, db0 = torch.randn(C, D, generator=_gen(5)) * 0.01, torch.randn(C, generator=_gen(6)) * 0.01
    b = P.head_bwd(dl, xhat, dW0, db0)
    r["dW"] = P.ratio(dW0 + dl.T @ xhat, b["dW"], P.sum_bound(b["n"], b["t_dW"]))
    r["dbias"] = P.ratio(db0 + dl.sum(0), b["dbias"], P.sum_bound(b["n"], b["t_dbias"]))
    for k, v in r.items():
        print(f"({B}, {D}, {C}) {k}: err/bound {v:.3f}")
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("B,N,D", [(2, 197, 768), (3, 50, 768), (2, 257, 1280), (1, 2, 64)])
def test_pool_norm_bound_holds_and_excludes_row_zero(B, N, D):
    g = _gen(7)
    x = torch.randn(B, N, D, generator=g) * 2.0 + 0.5
    x[:, 0] = 1e4 * torch.randn(B, D, generator=g)   # (a constant row would cancel in the LayerNorm)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = P.pool_norm(x, gamma, beta)
    pooled = x[:, 1:].sum(1) / f32_(N - 1)
    got = torch.nn.functional.layer_norm(pooled, (D,), gamma, beta, 1e-6)
    assert P.ratio(pooled, ref["pooled"], ref["e_pooled"]) <= 1.0
    assert P.ratio(got, ref["feat"], ref["e_feat"]) <= 1.0
    leaky = torch.nn.functional.layer_norm(x.mean(1), (D,), gamma, beta, 1e-6)   # row 0 included
    assert P.ratio(leaky, ref["feat"], ref["e_feat"]) > 1.0


@pytest.mark.parametrize("shape", [(7, 64), (1000, 768), (5,), (1,)])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_lars_bound_holds(shape, wd):
    g = _gen(9)
    p, gr, mu = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g) * 0.1, torch.randn(*shape, generator=g) * 0.01
    ref = P.lars_step(p, gr, mu, len(shape) > 1, 0.3, wd)
    p2, mu2 = emu_lars(p, gr, mu, len(shape) > 1, 0.3, wd)
    assert P.ratio(mu2, ref["mu"], ref["e_mu"]) <= 1.0 and P.ratio(p2, ref["p"], ref["e_p"]) <= 1.0


# ---------------------------------------------------------------------------------------------------- wrong variants
def test_bounds_reject_wrong_variants():
    B, D, C = 16, 64, 7
    feat, W, bias, rm, rv, target = _head_inputs(B, D, C)
    ref = P.head_fwd_train(feat, W, bias, rm, rv)
    live = [d for d in range(D) if d != 3]   # (the constant column is 0 under either variance)
    # unbiased instead of biased variance in xhat
    _, _, xhat_u, _, _ = emu_bn_train(feat, rm, rv, unbiased_xhat=True)
    assert P.ratio(xhat_u[:, live], ref["xhat"][:, live], ref["e_xhat"][:, live]) > 1.0
    # biased variance in the running update
    _, _, xhat, _, rv_b = emu_bn_train(feat, rm, rv, biased_running=True)
    assert P.ratio(rv_b[live], ref["running_var"][live], ref["e_running_var"][live]) > 1.0
    # the loss not divided by accum_iter
    logits = xhat @ W.T + bias
    c = P.ce(logits, target, 0.5)
    _, dl_full = emu_ce(logits, target, 1.0)
    assert P.ratio(dl_full, c["dlogits"], c["e_dlogits"]) > 1.0
    # a trust ratio / decay applied to the bias
    g = _gen(11)
    b, gb, mub = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.1, torch.zeros(C)
    want = P.lars_step(b, gb, mub, False, 0.3, 0.05)
    with_ratio = emu_lars(b, gb, mub, True, 0.3, 0.0)       # treated like a matrix
    mu_decay = gb + f32_(0.05) * b                          # decay, no trust ratio
    for wrong in (with_ratio, (b - f32_(0.3) * mu_decay, mu_decay)):
        assert P.ratio(wrong[0], want["p"], want["e_p"]) > 1.0 and P.ratio(wrong[1], want["mu"], want["e_mu"]) > 1.0
    # q not forced to 1 at a zero norm: a zero parameter stops moving (q = 0), a zero update divides by zero
    z, gz = torch.zeros(3, 7), torch.randn(3, 7, generator=g)
    want = P.lars_step(z, gz, torch.zeros(3, 7), True, 0.3, 0.0)
    p2, mu2 = emu_lars(z, gz, torch.zeros(3, 7), True, 0.3, 0.0, force_q=False)
    assert P.ratio(p2, want["p"], want["e_p"]) > 1.0 and P.ratio(mu2, want["mu"], want["e_mu"]) > 1.0
    s = torch.randn(5, 6, generator=g)
    want = P.lars_step(s, torch.zeros(5, 6), torch.zeros(5, 6), True, 0.3, 0.0)
    p2, mu2 = emu_lars(s, torch.zeros(5, 6), torch.zeros(5, 6), True, 0.3, 0.0, force_q=False)
    assert P.ratio(p2, want["p"], want["e_p"]) > 1.0   # NaN: not finite counts as outside every bound
