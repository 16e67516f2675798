"""Float64 restatements of the linear-probe kernels (csrc/pm_probe.hip) and the element-wise bounds of their outputs (not a test
module).  Built like tests/rowops_ref.py, which it imports and does not edit: every reference takes the operands as the kernel sees
them (f32 tensors, whatever device) and runs in plain torch float64; every bound is counted from the rounding points of the kernel's
arithmetic, u = 2^-24, no fitted factor.  tests/test_linprobe_cpu.py holds the restatements to the recorded reference run
(tests/golden/linprobe.npz) and the bounds to f32 emulations and to wrong variants; tests/test_gpu_linprobe.py holds the kernels to them.

BatchNorm (training): the LayerNorm-shaped chain of rowops_ref.row_stats with the roles of B and D exchanged -- per COLUMN d the
  mean over B, the biased variance, r = (var + eps)^-1/2, xhat = (x - mean) r, and e_mean, e_rstd, e_xhat as derived there.
  running' = (1 - m) running + m new: four roundings (1 - m, the two products, the sum) of the two terms' sizes, plus m times the
  error of `new`; the unbiased variance sum / (B - 1) carries (B + 3) u relative (subtract, square, B - 1 additions of positive
  terms, the division) and the mean's error squared, times B / (B - 1) (the deviations from the true mean sum to zero).
BatchNorm (eval): r = (running_var + eps)^-1/2 carries 2.5 u (the addition halves under the root, rsqrtf 2 u); xhat the subtraction
  and the product: 5 u |xhat| in all (the subtraction's rounding is relative to |x - mean| itself).
Linear: rowops_ref._dot_bound -- the error of xhat through |W| plus (D + 2) u of the absolute terms.
Cross-entropy, per row with a_c = z_c - max z <= 0, S = sum_c exp(a_c):
  every term of S carries (|a_c| + 2) u (the subtraction's rounding through exp, expf itself), the sum (C + 1) u more:
      r_S = (max |a| + C + 3) u
  lse = max + log S: r_S + 2 u |log S| + u |lse|;  the row's loss lse - z_t: + u |loss_b|;  the mean: sum_bound(B + 1, mean |loss_b|).
  p_c = exp(a_c) / S: (|a_c| + 2) u + r_S + 4 u (the reciprocal, the product);  dlogits = (p - onehot) g with g = s / B:
      e = g p ((|a_c| + 6) u + r_S) + 5 u |dlogits|     (the subtraction, g's own two roundings, the product, one spare)
  The counts are integers: equal or wrong.
Head backward: sums of B products into a prior value, sum_bound(B + 1, T) as for rowops_ref.head_bwd's dW / dbias.
Pool + fc_norm: pooled = mean over the N - 1 patch rows: N u of the mean absolute term (N - 2 additions, the division).  The
  LayerNorm behind it sees operands off by d_k <= e_pool: the mean moves by mean_k d_k, the variance by at most
  (2 / D) sum_k |x_k - mean| (d_k + mean d) + (max d + mean d)^2, half of that relative to var + eps in rstd; then row_stats' chain.
LARS, one step from f32 operands: dp = g + wd p (2 u of the two terms); q from f64 norms of f32 values, rounded to f32 once (the
  norms of the rounded dp carry its 2 u): 4 u; dp q: u.  mu' = m mu + dp: e_dp + 2 u |m mu| + u |mu'|;  p' = p - lr mu':
  lr e_mu + u |lr mu'| + u |p'|."""
import torch

import rowops_ref as R
from rowops_ref import U32, ratio, sum_bound  # noqa: F401

BN_EPS = 1e-6
MOMENTUM = 0.1


# ------------------------------------------------------------------------------------------------ BatchNorm1d(affine=False)
def bn_train(feat, eps=BN_EPS):
    """feat [B, D] -> float64 mean / var (biased) / var_unbiased / rstd [D], xhat [B, D] and e_mean, e_rstd, e_xhat, e_var_unbiased."""
    B = feat.shape[0]
    s = R.row_stats(feat.double().T.contiguous(), eps)  # columns as rows: the chain with B and D exchanged
    col = lambda k: s[k][:, 0]
    var_u = col("var") * B / (B - 1)
    return dict(mean=col("mean"), var=col("var"), var_unbiased=var_u, rstd=col("rstd"), xhat=s["xhat"].T, e_mean=col("e_mean"),
                e_rstd=col("e_rstd"), e_xhat=s["e_xhat"].T, e_var_unbiased=var_u * (B + 3) * U32 + col("e_mean") ** 2 * B / (B - 1))


def running_update(old, new, e_new, momentum=MOMENTUM):
    """(1 - momentum) old + momentum new -> (float64 value, bound)."""
    old, new = old.double(), new.double()
    val = (1 - momentum) * old + momentum * new
    return val, momentum * e_new + 4 * U32 * (((1 - momentum) * old).abs() + (momentum * new).abs())


def bn_eval(feat, running_mean, running_var, eps=BN_EPS):
    x = feat.double()
    xhat = (x - running_mean.double()) * (running_var.double() + eps) ** -0.5
    return dict(xhat=xhat, e_xhat=5 * U32 * xhat.abs())


def linear(xhat, e_xhat, W, bias):
    """-> (float64 logits, bound)."""
    return R._dot_bound(xhat, e_xhat, W.double(), bias.double())


def head_fwd_train(feat, W, bias, running_mean, running_var, eps=BN_EPS, momentum=MOMENTUM):
    s = bn_train(feat, eps)
    s["logits"], s["e_logits"] = linear(s["xhat"], s["e_xhat"], W, bias)
    s["running_mean"], s["e_running_mean"] = running_update(running_mean, s["mean"], s["e_mean"], momentum)
    s["running_var"], s["e_running_var"] = running_update(running_var, s["var_unbiased"], s["e_var_unbiased"], momentum)
    return s


def head_fwd_eval(feat, W, bias, running_mean, running_var, eps=BN_EPS):
    s = bn_eval(feat, running_mean, running_var, eps)
    s["logits"], s["e_logits"] = linear(s["xhat"], s["e_xhat"], W, bias)
    return s


# ------------------------------------------------------------------------------------------------ cross-entropy + accuracy
def ce(logits, target, scale=1.0):
    """torch.nn.CrossEntropyLoss() on logits [B, C] as given, the gradient times `scale` -> float64 loss, row_loss, dlogits, the
    counts correct1 / correctk (k = min(5, C)) and e_loss, e_dlogits."""
    z = logits.double()
    B, C = z.shape
    t = target.long()
    m = z.max(1, keepdim=True).values
    a = z - m
    S = a.exp().sum(1, keepdim=True)
    lse = m + S.log()
    zt = z.gather(1, t[:, None])
    row = (lse - zt)[:, 0]
    r_S = (a.abs().max(1, keepdim=True).values + C + 3) * U32
    e_row = (r_S + 2 * U32 * S.log().abs() + U32 * lse.abs())[:, 0] + U32 * row.abs()
    loss = row.mean()
    e_loss = e_row.mean() + sum_bound(B + 1, row.abs().mean())
    p = a.exp() / S
    onehot = torch.zeros_like(z).scatter_(1, t[:, None], 1.0)
    g = float(scale) / B
    d = (p - onehot) * g
    e_d = abs(g) * p * ((a.abs() + 6) * U32 + r_S) + 5 * U32 * d.abs()
    above = (z > zt).sum(1)
    return dict(loss=loss, row_loss=row, dlogits=d, e_loss=e_loss, e_dlogits=e_d, correct1=int((above < 1).sum()),
                correctk=int((above < min(5, C)).sum()))


# ------------------------------------------------------------------------------------------------ head backward
def head_bwd(dlogits, xhat, dW0, db0):
    """dW = dW0 + dlogits^T xhat, dbias = db0 + sum_b dlogits -> values, the sums of absolute terms t_*, n = B + 1."""
    dl, xh, w0, b0 = dlogits.double(), xhat.double(), dW0.double(), db0.double()
    return dict(dW=w0 + dl.T @ xh, t_dW=w0.abs() + dl.abs().T @ xh.abs(), dbias=b0 + dl.sum(0), t_dbias=b0.abs() + dl.abs().sum(0),
                n=dl.shape[0] + 1)


# ------------------------------------------------------------------------------------------------ pool + fc_norm
def pool_norm(x, gamma, beta, eps=R.LN_EPS):
    """x [B, N, D] -> float64 feat = LayerNorm(mean of rows 1..N-1) [B, D], pooled, and e_feat, e_pooled."""
    x = x.double()
    N, D = x.shape[1], x.shape[2]
    pooled = x[:, 1:].mean(1)
    d = N * U32 * x[:, 1:].abs().mean(1)                     # e_pooled, per element
    s = R.row_stats(pooled, eps)
    dm = d.mean(-1, keepdim=True)
    dev = (pooled - s["mean"]).abs()
    dvar = 2.0 / D * (dev * (d + dm)).sum(-1, keepdim=True) + (d.max(-1, keepdim=True).values + dm) ** 2
    rr = s["r_rstd"] + dvar / (2 * (s["var"] + eps))
    e_xhat = s["xhat"].abs() * (rr + 3 * U32) + s["rstd"] * (s["e_mean"] + dm + d)
    g, b = gamma.double(), beta.double()
    y = s["xhat"] * g + b
    return dict(feat=y, pooled=pooled, e_pooled=d, e_feat=g.abs() * e_xhat + 2 * U32 * ((s["xhat"] * g).abs() + b.abs()))


# ------------------------------------------------------------------------------------------------ LARS
def lars_step(p, g, mu, is_matrix, lr, wd, momentum=0.9, tc=0.001):
    """mae/util/lars.py:22-47 for one tensor -> float64 p', mu', q and the one-step bounds e_p, e_mu."""
    p, g, mu = p.double(), g.double(), mu.double()
    q = 1.0
    if is_matrix:
        dp = g + wd * p
        pn, un = p.norm(), dp.norm()
        if pn > 0 and un > 0:
            q = float(tc * pn / un)
        e_dp = abs(q) * (2 * U32 * (g.abs() + (wd * p).abs()) + 5 * U32 * dp.abs())
        dp = dp * q
    else:
        dp, e_dp = g, torch.zeros_like(g)
    mu2 = momentum * mu + dp
    e_mu = e_dp + 2 * U32 * (momentum * mu).abs() + U32 * mu2.abs()
    p2 = p - lr * mu2
    e_p = abs(lr) * e_mu + U32 * (lr * mu2).abs() + U32 * p2.abs()
    return dict(p=p2, mu=mu2, q=q, e_p=e_p, e_mu=e_mu)


# ------------------------------------------------------------------------------------------------ schedule + sampler
def lr_at(epoch, lr, min_lr, warmup_epochs, epochs):
    """mae/util/lr_sched.py:9-21."""
    import math
    if epoch < warmup_epochs:
        return lr * epoch / warmup_epochs
    return min_lr + (lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch - warmup_epochs) / (epochs - warmup_epochs)))


def fixture_run(golden, name):
    """The arrays of run `name` of tests/golden/linprobe.npz as float64 / int64 tensors; the wd = 0.05 runs share the inputs of
    the wd = 0 run of their shape."""
    base = name.replace("_wd5", "_wd0")
    run = {k.split(".", 1)[1]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(name + ".")}
    for k in ("feats", "targets", "W0", "b0", "still0", "zero_grad"):
        run.setdefault(k, torch.from_numpy(golden[f"{base}.{k}"]))
    accum, per_epoch, steps, warmup, epochs = (int(v) for v in golden["schedule"])
    if name == "vitb":
        accum, per_epoch, steps = 1, 2, 2
    run.update(accum=accum, per_epoch=per_epoch, steps=steps, warmup=warmup, epochs=epochs, lr0=float(golden["schedule_lr"][0]),
               min_lr=float(golden["schedule_lr"][1]), wd=float(run["weight_decay"]))
    return run


PARAMS = ("head.1.weight", "head.1.bias", "zero", "still")


def replay(run, dtype=torch.float64):
    """The recorded run restated with the functions above (engine_finetune.train_one_epoch as main_linprobe calls it), in float64.
    Yields after every micro-step a dict with the fixture's names: loss, lr, acc1, acc5, running_mean, running_var, tracked,
    updated, the four parameters and their mu."""
    p = {"head.1.weight": run["W0"].clone(), "head.1.bias": run["b0"].clone(), "zero": torch.zeros_like(run["zero_grad"]),
         "still": run["still0"].clone()}
    mu = {n: torch.zeros_like(v) for n, v in p.items()}
    grad = {n: torch.zeros_like(v) for n, v in p.items()}
    have_mu = {n: False for n in p}
    D = run["W0"].shape[1]
    rm, rv, tracked = torch.zeros(D, dtype=dtype), torch.ones(D, dtype=dtype), 0
    accum, lr = run["accum"], 0.0
    for it in range(run["steps"]):
        epoch, step = divmod(it, run["per_epoch"])
        if step % accum == 0:
            lr = lr_at(step / run["per_epoch"] + epoch, run["lr0"], run["min_lr"], run["warmup"], run["epochs"])
        x, y = run["feats"][step % run["feats"].shape[0]], run["targets"][step % run["feats"].shape[0]]
        f = head_fwd_train(x, p["head.1.weight"], p["head.1.bias"], rm, rv)
        rm, rv, tracked = f["running_mean"], f["running_var"], tracked + 1
        c = ce(f["logits"], y, 1.0 / accum)
        b = head_bwd(c["dlogits"], f["xhat"], grad["head.1.weight"], grad["head.1.bias"])
        grad["head.1.weight"], grad["head.1.bias"] = b["dW"], b["dbias"]
        grad["zero"] = grad["zero"] + run["zero_grad"] / accum
        update = (step + 1) % accum == 0
        if update:
            for n in PARAMS:
                s = lars_step(p[n], grad[n], mu[n], p[n].ndim > 1, lr, run["wd"])
                p[n], mu[n], have_mu[n] = s["p"], s["mu"], True
                grad[n] = torch.zeros_like(grad[n])
        out = dict(loss=c["loss"], lr=lr, acc1=c["correct1"], acc5=c["correctk"], running_mean=rm, running_var=rv, tracked=tracked,
                   updated=int(update))
        out.update({n: p[n] for n in PARAMS})
        out.update({"mu." + n: mu[n] for n in PARAMS})
        yield out
