"""What FusedAdamW(per_parameter_steps=True) costs where nothing is ever unfrozen (HIP events): the optimizer step alone and the
fine-tune step (ViT-B/16, batch 64, bf16, mode "full", eager launch, overlapped AdamW -- the benchmark's headline configuration),
with the flag on against the default optimizer in the same process.

    python tools/finetune_schedule_bench.py [--calls 30] [--steps 30] [--rounds 4] [--batch 64] [--out profiles/finetune_schedule.json]

Two models from one seed, one optimizer each (flag off / flag on); windows of the two kinds alternate `rounds` times (other work
shares the host and the device: only alternating windows compare), each window timed by device events after a warm-up step of its
kind.  With a constant gradient pattern the flag runs the same update kernels over the same segments with R == G records; what
differs is one tick launch over a list instead of over the groups, and the host's planning per step.
Optimizer step alone: step() called `calls` times on the gradients of one backward (inline path, no overlap)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_ms(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def make(torch, flag, overlap, batch):
    import ssl4polyp_amd as A
    from ssl4polyp_amd.optim import FusedAdamW
    from ssl4polyp_amd.train import configure_finetune_parameters
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = A.get_MAE_backbone(None, True, 2, False, None, precision="bf16").to(dev)
    configure_finetune_parameters(model, "full")
    head = list(model.lin_head.parameters())
    hid = {id(p) for p in head}
    groups = [{"params": head, "name": "head"}, {"params": [p for p in model.parameters() if id(p) not in hid], "name": "backbone"}]
    opt = FusedAdamW(model, groups, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05, overlap_forward=overlap, per_parameter_steps=flag)
    gen = torch.Generator(device=dev).manual_seed(1234)
    imgs = [torch.randn(batch, 3, 224, 224, generator=gen, device=dev) for _ in range(4)]
    labels = (torch.rand(16, batch, generator=gen, device=dev) < 0.5).long()
    pw = torch.tensor(1.0, device=dev)
    tick = [0]

    def backward():
        i = tick[0]
        tick[0] += 1
        opt.zero_grad(set_to_none=True)
        A.supervised_loss(model(imgs[i % 4]), labels[i % 16], pos_weight=pw).backward()

    def step():
        backward()
        opt.step()
    return model, opt, backward, step


def summary(ms):
    out = {"ms": ms}
    for kind, v in ms.items():
        out[kind + "_median_ms"] = statistics.median(v)
        out[kind + "_min_ms"], out[kind + "_max_ms"] = min(v), max(v)
    out["flag_minus_default_us_median"] = (out["per_parameter_steps_median_ms"] - out["default_median_ms"]) * 1e3
    out["window_spread_us"] = max(max(v) - min(v) for v in ms.values()) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("finetune_schedule_bench: no GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch}
    kinds = (("default", False), ("per_parameter_steps", True))
    # -- the optimizer step alone (inline path)
    runs = {kind: make(torch, flag, False, args.batch) for kind, flag in kinds}
    ms = {kind: [] for kind, _ in kinds}
    for kind, _ in kinds:
        runs[kind][2]()
        for _ in range(5):
            runs[kind][1].step()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for kind, _ in kinds:
            opt = runs[kind][1]
            opt.step()
            torch.cuda.synchronize()
            ms[kind].append(events_ms(torch, opt.step, args.calls))
    result["optimizer_step"] = dict(summary(ms), calls_per_window=args.calls)
    same = all(torch.equal(a, b) for a, b in zip(runs["default"][0]._rt.flat.P.values(), runs["per_parameter_steps"][0]._rt.flat.P.values()))
    result["optimizer_step"]["same_bits"] = bool(same)
    del runs
    torch.cuda.empty_cache()
    # -- the fine-tune step (overlapped AdamW)
    runs = {kind: make(torch, flag, True, args.batch) for kind, flag in kinds}
    ms = {kind: [] for kind, _ in kinds}
    for kind, _ in kinds:
        for _ in range(10):
            runs[kind][3]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for kind, _ in kinds:
            runs[kind][3]()
            torch.cuda.synchronize()
            ms[kind].append(events_ms(torch, runs[kind][3], args.steps))
    result["cls_step"] = dict(summary(ms), steps_per_window=args.steps)
    for kind, _ in kinds:
        runs[kind][1].sync()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(runs["default"][0]._rt.flat.P.values(), runs["per_parameter_steps"][0]._rt.flat.P.values()))
    result["cls_step"]["same_bits"] = bool(same)
    result["records"] = runs["per_parameter_steps"][1]._plan_cohorts().n_records
    for name in ("optimizer_step", "cls_step"):
        r = result[name]
        print(f"{name}: default median {r['default_median_ms']:.3f} ms, per_parameter_steps median {r['per_parameter_steps_median_ms']:.3f} ms "
              f"(difference {r['flag_minus_default_us_median']:.1f} us; spread between windows of one kind up to {r['window_spread_us']:.1f} us; "
              f"same bits {r['same_bits']})")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
