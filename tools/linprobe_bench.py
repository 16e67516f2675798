"""What the linear probe adds beside the frozen forward (HIP events): ViT-B/16, bf16 encoder, B = 512 and B = 64.

    python tools/linprobe_bench.py [--batches 512 64] [--classes 1000] [--rounds 4] [--calls 200] [--out profiles/linprobe.json]
    python tools/linprobe_bench.py --forward-only [--tree OTHER_CHECKOUT]      # the evaluation forward alone, any commit

Per batch size, in ONE process: windows of the existing evaluation forward alone (a head=False classifier of models.py in eval
mode: the frozen encoder pass) and of the probe training step per micro-batch (features, BatchNorm + Linear, cross-entropy,
head backward, LARS step, zero_grad) alternate `rounds` times, each window of at least ~0.5 s timed by device events after a warm-up of
its kind (other work shares the host and the device: only alternating windows compare).  Then the added launches singly, µs per
call: pool-norm (with its achieved bytes/s: it reads B N D 4 bytes once), head forward, cross-entropy, head backward, LARS.
--forward-only times the evaluation forward alone through interfaces every commit has; --tree imports the package from another
checkout, so the same file measures the parent commit's forward beside this one's (alternate the two commands in one job)."""
import argparse
import json
import os
import statistics
import sys

HBM_PEAK_TBS = 8.0   # MI355X HBM3E specification


def events_ms(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def window(torch, fn, min_ms=500.0):
    """ms per call over a window of at least min_ms (sized by one timed probe call after the warm-up)."""
    fn()
    torch.cuda.synchronize()
    one = max(events_ms(torch, fn, 2), 1e-3)
    return events_ms(torch, fn, max(int(min_ms / one), 5))


def forward_windows(torch, A, batch, rounds, other=None):
    """[ms] of the evaluation forward alone; with `other`, its windows alternate with other()'s -> ([ms], [ms])."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    old = A.VisionTransformer_from_Any(False, 2, True, None, 768, 12, 12, "cls", precision="bf16").to(dev).eval()
    imgs = torch.randn(batch, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def fwd():
        with torch.no_grad():
            old(imgs)

    for _ in range(3):
        fwd()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(torch, fwd))
        if other is not None:
            b.append(window(torch, other))
    return (a, b) if other is not None else a


def singles(torch, batch, C, calls):
    from ssl4polyp_amd.optim import FusedLARS
    from ssl4polyp_amd.probe import ProbeHead, pool_norm, probe_ce_raw, probe_head_bwd, probe_head_fwd
    dev = torch.device("cuda", 0)
    N, D = 197, 768
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(batch, N, D, device=dev, generator=g)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    head = ProbeHead(torch.nn.Linear(D, C)).to(dev).train()
    bn, lin = head[0], head[1]
    feat = pool_norm(x, gamma, beta)
    target = torch.randint(0, C, (batch,), device=dev, generator=g)
    scale = torch.ones((), device=dev)
    logits, xhat = probe_head_fwd(feat, lin.weight.detach(), lin.bias.detach(), bn.running_mean, bn.running_var, bn.num_batches_tracked, True)
    _, dlogits, _ = probe_ce_raw(logits, target, scale, True)
    lin.weight.grad, lin.bias.grad = torch.zeros_like(lin.weight), torch.zeros_like(lin.bias)
    opt = FusedLARS(head.parameters(), lr=0.1)
    fns = {
        "pool_norm": lambda: pool_norm(x, gamma, beta),
        "head_fwd": lambda: probe_head_fwd(feat, lin.weight.detach(), lin.bias.detach(), bn.running_mean, bn.running_var,
                                           bn.num_batches_tracked, True),
        "ce": lambda: probe_ce_raw(logits, target, scale, True),
        "head_bwd": lambda: probe_head_bwd(dlogits, xhat, lin.weight.grad, lin.bias.grad),
        "lars": opt.step,
    }
    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = sorted(events_ms(torch, fn, calls) * 1e3 for _ in range(5))
        out[name] = {"us_median": us[2], "us_min": us[0], "us_max": us[4]}
        if name == "pool_norm":
            nbytes = batch * N * D * 4
            out[name].update(bytes=nbytes, TB_per_s_median=nbytes / us[2] / 1e6, share_of_hbm_peak=nbytes / us[2] / 1e6 / HBM_PEAK_TBS)
        print(f"B={batch} C={C} {name}: median {us[2]:.1f} us (min {us[0]:.1f}, max {us[4]:.1f}) of 5 x {calls} calls"
              + (f", {out[name]['TB_per_s_median']:.2f} TB/s" if name == "pool_norm" else ""))
    out["added_us_cls_token"] = sum(out[k]["us_median"] for k in ("head_fwd", "ce", "head_bwd", "lars"))
    return out


def probe_step(torch, A, batch, C, rounds):
    from ssl4polyp_amd import models_vit
    from ssl4polyp_amd.optim import FusedLARS
    from ssl4polyp_amd.probe import probe_ce
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models_vit.vit_base_patch16(num_classes=C, precision="bf16")
    torch.nn.init.trunc_normal_(model.head.weight, std=0.01)
    models_vit.add_probe_head(model).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(1)
    imgs = torch.randn(batch, 3, 224, 224, device=dev, generator=gen)
    target = torch.randint(0, C, (batch,), device=dev, generator=gen)
    opt = FusedLARS(model.head.parameters(), lr=0.1)
    scale = torch.ones((), device=dev)

    def step():
        loss, _ = probe_ce(model(imgs), target, scale)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)

    for _ in range(3):
        step()
    fwd, stp = forward_windows(torch, A, batch, rounds, other=step)
    out = {"forward_ms": fwd, "probe_step_ms": stp, "forward_median_ms": statistics.median(fwd), "probe_step_median_ms": statistics.median(stp)}
    out["added_ms"] = out["probe_step_median_ms"] - out["forward_median_ms"]
    out["added_share_of_step"] = out["added_ms"] / out["probe_step_median_ms"]
    print(f"B={batch} C={C}: evaluation forward median {out['forward_median_ms']:.3f} ms of {[round(v, 3) for v in fwd]}; probe step "
          f"median {out['probe_step_median_ms']:.3f} ms of {[round(v, 3) for v in stp]}; added {out['added_ms'] * 1e3:.0f} us = "
          f"{100 * out['added_share_of_step']:.2f} % of the step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 64])
    ap.add_argument("--classes", type=int, nargs="+", default=[1000])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linprobe_bench: no GPU (a timing taken elsewhere says nothing)")
    import ssl4polyp_amd as A
    result = {"device": torch.cuda.get_device_name(0), "host": os.uname().nodename, "model": "ViT-B/16",
              "precision": "bf16", "batches": {}}
    for batch in args.batches:
        if args.forward_only:
            ms = forward_windows(torch, A, batch, args.rounds)
            result["batches"][str(batch)] = {"forward_ms": ms, "forward_median_ms": statistics.median(ms)}
            print(f"B={batch}: evaluation forward median {statistics.median(ms):.3f} ms of {[round(v, 3) for v in ms]}")
            continue
        entry = result["batches"][str(batch)] = {}
        for C in args.classes:
            entry[f"C={C}"] = {"step": probe_step(torch, A, batch, C, args.rounds), "singles": singles(torch, batch, C, args.calls)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
