"""What the MAE fine-tune recipe costs around the block stack (HIP events): ViT-B/16, bf16, B = 64, global_pool, 1000 classes.

    python tools/finetune_mae_bench.py [--batch 64] [--classes 1000] [--rounds 4] [--calls 200] [--out profiles/finetune_mae.json]
    python tools/finetune_mae_bench.py --singles-only      # the new launches alone (the run to put under rocprofv3 --kernel-trace --stats)

In ONE process, windows of two training steps alternate `rounds` times, each window of at least ~0.5 s timed by device events after a
warm-up of its kind (other work shares the host and the device: only alternating windows compare):
  (a) recipe   mix (Mixup 0.8 / CutMix 1.0) -> forward -> soft-target CE (smoothing 0.1) -> backward -> FusedAdamW over the
               layer-decay groups of lr_decay.param_groups_lrd (26 at depth 12) with the lr adjusted every step
  (b) plain    the same model and batch without mixing or smoothing, FusedAdamW over optim.add_weight_decay's two groups
Then the new launches singly, us per call, with the bytes each must move and the rate that gives: pm_mix_batch (reads and writes
the batch once: 2 x B 3 H W 4 bytes), pm_pool_norm_bwd (writes B N D (4 + 2) bytes), pm_pool_norm_fwd_train (reads B N D 4), and
the latency-bound ones (soft CE, Linear head forward, dfeat).  And the optimiser update alone under both groupings, with the number
of pm_adamw_dev launches each makes.  The headline classifier step of bench.py is measured by bench.py itself, on this commit and on
its parent, in the same job."""
import argparse
import json
import os
import statistics
import sys
import types

HBM_PEAK_TBS = 8.0   # MI355X HBM3E specification
STREAM_TBS = 5.0     # what the project's other streaming kernels reach (README)


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


def five(torch, fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = sorted(events_ms(torch, fn, calls) * 1e3 for _ in range(5))
    return {"us_median": us[2], "us_min": us[0], "us_max": us[4]}


def build(torch, batch, C, recipe):
    import numpy as np
    from ssl4polyp_amd import models_vit
    from ssl4polyp_amd.lr_decay import param_groups_lrd
    from ssl4polyp_amd.mixup import Mixup, soft_target_ce
    from ssl4polyp_amd.optim import FusedAdamW, add_weight_decay
    from ssl4polyp_amd.train import adjust_learning_rate
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models_vit.vit_base_patch16(num_classes=C, global_pool=True, precision="bf16")
    torch.nn.init.trunc_normal_(model.head.weight, std=2e-5)
    model.to(dev).train()
    model._rt.ensure(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    imgs0 = torch.randn(batch, 3, 224, 224, device=dev, generator=gen)
    target = torch.randint(0, C, (batch,), device=dev, generator=gen)
    args = types.SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=5, epochs=50)
    if recipe:
        groups = param_groups_lrd(model, 0.05, model.no_weight_decay(), 0.75)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C, rng=np.random.RandomState(0))
    else:
        groups = add_weight_decay(model, 0.05, model.no_weight_decay())
        mix = None
    opt = FusedAdamW(model, groups, lr=args.lr)
    imgs = torch.empty_like(imgs0)
    it = [0]

    def step():
        it[0] += 1
        adjust_learning_rate(opt, 5.0 + it[0] * 1e-3, args)
        imgs.copy_(imgs0)   # (both arms: the loader's batch arrives fresh every step)
        if mix is not None:
            mix(imgs, target)
        loss = soft_target_ce(model(imgs), target, mix.state if mix is not None else None, 0.1 if recipe else 0.0)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    return model, opt, step


def steps(torch, batch, C, rounds):
    _, opt_a, step_a = build(torch, batch, C, True)
    _, opt_b, step_b = build(torch, batch, C, False)
    for fn in (step_a, step_b):
        for _ in range(3):
            fn()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(torch, step_a))
        b.append(window(torch, step_b))
    out = {"recipe_step_ms": a, "plain_step_ms": b, "recipe_median_ms": statistics.median(a), "plain_median_ms": statistics.median(b),
           "recipe_param_groups": len(opt_a.param_groups), "plain_param_groups": len(opt_b.param_groups)}
    out["added_ms"] = out["recipe_median_ms"] - out["plain_median_ms"]
    out["added_share_of_step"] = out["added_ms"] / out["recipe_median_ms"]
    print(f"B={batch} C={C}: recipe step median {out['recipe_median_ms']:.3f} ms of {[round(v, 3) for v in a]}; plain step median "
          f"{out['plain_median_ms']:.3f} ms of {[round(v, 3) for v in b]}; added {out['added_ms'] * 1e3:.0f} us = "
          f"{100 * out['added_share_of_step']:.2f} % of the step")
    return out


def optimiser(torch, batch, C, calls):
    """The update alone under both groupings (gradients left in place from one backward), and its pm_adamw_dev launches."""
    out = {}
    for name, recipe in (("layer_decay_groups", True), ("two_groups", False)):
        model, opt, _ = build(torch, batch, C, recipe)
        from ssl4polyp_amd.mixup import soft_target_ce
        imgs = torch.randn(batch, 3, 224, 224, device="cuda")
        target = torch.randint(0, C, (batch,), device="cuda")
        soft_target_ce(model(imgs), target).backward()
        f = model._rt.flat
        launches = sum(len(opt._segments(f, g)) for g in opt.param_groups)
        out[name] = {**five(torch, opt.step, calls), "param_groups": len(opt.param_groups), "pm_adamw_dev_launches": launches}
        print(f"AdamW update, {name}: {len(opt.param_groups)} groups, {launches} pm_adamw_dev launches, median "
              f"{out[name]['us_median']:.1f} us (min {out[name]['us_min']:.1f}, max {out[name]['us_max']:.1f})")
        del model, opt
    return out


def singles(torch, batch, C, calls):
    import ctypes
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    from ssl4polyp_amd.mixup import MixState, mix_batch, soft_ce_raw
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    N, D, H = 197, 768, 224
    g = torch.Generator(device=dev).manual_seed(2)
    imgs = torch.randn(batch, 3, H, H, device=dev, generator=g)
    mixup_state, cutmix_state = MixState(dev), MixState(dev)
    mixup_state.write(0.3, False, (0, 0, 0, 0))
    cutmix_state.write(0.5, True, (32, 192, 40, 200))
    x = torch.randn(batch, N, D, device=dev, generator=g)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    feat, pooled = torch.empty(batch, D, device=dev), torch.empty(batch, D, device=dev)
    mean, rstd = torch.empty(batch, device=dev), torch.empty(batch, device=dev)
    size = ctypes.c_size_t(0)
    _lib.check(lib.pm_pool_norm_workspace(batch, N, D, ctypes.byref(size)), "pm_pool_norm_workspace")
    ws = torch.empty(size.value // 4, device=dev)
    dfeat = torch.randn(batch, D, device=dev, generator=g)
    dx, dx_act = torch.empty(batch, N, D, device=dev), torch.empty(batch, N, D, device=dev, dtype=torch.bfloat16)
    dgamma, dbeta = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ws2 = torch.empty(batch * D, device=dev)
    W, bias = torch.randn(C, D, device=dev, generator=g) * 0.02, torch.zeros(C, device=dev)
    logits = torch.empty(batch, C, device=dev)
    target = torch.randint(0, C, (batch,), device=dev, generator=g)
    scale = torch.ones((), device=dev)

    def pool_fwd():
        _lib.check(lib.pm_pool_norm_fwd_train(_ptr(x), batch, N, D, _ptr(gamma), _ptr(beta), 1e-6, _ptr(feat), _ptr(pooled), _ptr(mean),
                                              _ptr(rstd), _ptr(ws), size.value, _stream()), "pm_pool_norm_fwd_train")

    def pool_bwd():
        _lib.check(lib.pm_pool_norm_bwd(_ptr(dfeat), _ptr(pooled), _ptr(mean), _ptr(rstd), _ptr(gamma), batch, N, D, _ptr(dx), _ptr(dx_act),
                                        _lib.PM_BF16, _ptr(dgamma), _ptr(dbeta), _ptr(ws2), batch * D * 4, _stream()), "pm_pool_norm_bwd")

    def head_fwd():
        _lib.check(lib.pm_linear_head_fwd(_ptr(feat), batch, D, C, _ptr(W), _ptr(bias), _ptr(logits), _stream()), "pm_linear_head_fwd")

    pool_fwd()
    head_fwd()
    _, dlogits = soft_ce_raw(logits, target, mixup_state.record, 0.1, scale, True)

    def head_dfeat():
        _lib.check(lib.pm_linear_head_dfeat(_ptr(dlogits), _ptr(W), batch, D, C, _ptr(dfeat), _stream()), "pm_linear_head_dfeat")

    img_bytes = 2 * imgs.numel() * 4
    box_bytes = 2 * batch * 3 * (192 - 32) * (200 - 40) * 4
    fns = {
        "mix_batch_mixup": (lambda: mix_batch(imgs, mixup_state, True), img_bytes),
        "mix_batch_cutmix": (lambda: mix_batch(imgs, cutmix_state, True), box_bytes),
        "pool_norm_fwd_train": (pool_fwd, x.numel() * 4),
        "pool_norm_bwd": (pool_bwd, x.numel() * 6),
        "soft_ce": (lambda: soft_ce_raw(logits, target, mixup_state.record, 0.1, scale, True), None),
        "linear_head_fwd": (head_fwd, None),
        "linear_head_dfeat": (head_dfeat, None),
    }
    out = {}
    for name, (fn, nbytes) in fns.items():
        out[name] = five(torch, fn, calls)
        line = f"B={batch} C={C} {name}: median {out[name]['us_median']:.1f} us (min {out[name]['us_min']:.1f}, max {out[name]['us_max']:.1f})"
        if nbytes is not None:
            tbs = nbytes / out[name]["us_median"] / 1e6
            out[name].update(bytes=nbytes, TB_per_s_median=tbs, share_of_hbm_peak=tbs / HBM_PEAK_TBS, share_of_streaming_rate=tbs / STREAM_TBS)
            line += f", {nbytes / 1e6:.1f} MB, {tbs:.2f} TB/s"
        print(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--singles-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("finetune_mae_bench: no GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "host": os.uname().nodename, "model": "ViT-B/16 global_pool", "precision": "bf16",
              "batch": args.batch, "classes": args.classes}
    if not args.singles_only:
        result["step"] = steps(torch, args.batch, args.classes, args.rounds)
        result["adamw_update"] = optimiser(torch, args.batch, args.classes, args.calls)
    result["singles"] = singles(torch, args.batch, args.classes, args.calls)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
