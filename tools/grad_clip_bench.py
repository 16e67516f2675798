"""What gradient clipping costs (HIP events): the statistics pass alone at the ViT-B/16 flat sizes, and the fine-tune step
(ViT-B/16, batch 64, bf16, eager launch, overlapped AdamW -- the benchmark's headline configuration) with and without `max_norm`.

    python tools/grad_clip_bench.py [--calls 50] [--steps 30] [--rounds 4] [--batch 64] [--out profiles/grad_clip.json]

Statistics pass: the 17 segments of tools/adamw_bench.py (85.8 M f32 gradients, 343 MB read once), in two groups (head, backbone),
pm_grad_norms + pm_grad_clip per call; next to it the pm_grad_stats pass (f32 atomics) over the same segments, which a
loss-scaled step without clipping runs.
Step: ONE model and optimizer; windows of `steps` steps without max_norm and with it alternate `rounds` times in the same process
(other work shares the host and the device: only alternating windows compare), each window timed by device events after a
warm-up step of its kind.  max_norm = 1e30 never bites (coefficient exactly 1), so both kinds of window walk the same
trajectory and the difference is the cost of the two extra launches and the extra read of the gradients, nothing else."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [152064, 122112, 64, 589824] + [7077888] * 12 + [1536]  # tools/adamw_bench.py


def events_us(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def stats_pass(torch, _lib, calls):
    lib = _lib.load()
    tot, dev = sum(SIZES), "cuda:0"
    g = torch.randn(tot, device=dev) * 0.02
    hyper = torch.zeros(2, 16, device=dev)
    hyper[:, :6] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0])
    offs = [sum(SIZES[:i]) for i in range(len(SIZES))]
    groups = [1] * (len(SIZES) - 1) + [0]
    segs = (_lib.GradSegment * len(SIZES))(*[_lib.GradSegment(g.data_ptr() + 4 * o, n, k) for o, n, k in zip(offs, SIZES, groups)])
    size = ctypes.c_size_t(0)
    _lib.check(lib.pm_grad_norms_workspace(len(SIZES), 2, ctypes.byref(size)), "pm_grad_norms_workspace")
    ws = torch.zeros(size.value // 8, dtype=torch.float64, device=dev)
    sumsq, record = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(5, dtype=torch.float64, device=dev)
    triple = torch.zeros(3, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def norms():
        _lib.check(lib.pm_grad_norms(segs, len(SIZES), 2, ws.data_ptr(), size.value, sumsq.data_ptr(), triple.data_ptr(), st), "pm_grad_norms")
        _lib.check(lib.pm_grad_clip(sumsq.data_ptr(), hyper.data_ptr(), 2, 1.0, 1, 0, record.data_ptr(), st), "pm_grad_clip")

    def atomics():
        for o, n in zip(offs, SIZES):
            _lib.check(lib.pm_grad_stats(g.data_ptr() + 4 * o, n, triple.data_ptr(), st), "pm_grad_stats")

    out = {"elements": tot, "bytes": tot * 4}
    for name, fn in (("pm_grad_norms + pm_grad_clip", norms), ("pm_grad_stats per segment", atomics)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = sorted(events_us(torch, fn, calls) for _ in range(5))
        out[name] = {"us_median": us[2], "us_min": us[0], "us_max": us[4], "TB_per_s_median": tot * 4 / us[2] / 1e6}
        print(f"{name}: median {us[2]:.1f} us (min {us[0]:.1f}, max {us[4]:.1f}) of 5 x {calls} calls, {tot * 4 / us[2] / 1e6:.2f} TB/s")
    want = float(g.double().square().sum().sqrt())
    norms()
    print(f"total norm {float(record[2]):.12g} (torch float64 {want:.12g})")
    return out


def step_cost(torch, args):
    import ssl4polyp_amd as A
    from ssl4polyp_amd.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = A.get_MAE_backbone(None, True, 2, False, None, precision="bf16").to(dev)
    from ssl4polyp_amd.train import configure_finetune_parameters
    configure_finetune_parameters(model, "full")
    head = list(model.lin_head.parameters())
    hid = {id(p) for p in head}
    groups = [{"params": head, "name": "head"}, {"params": [p for p in model.parameters() if id(p) not in hid], "name": "backbone"}]
    opt = FusedAdamW(model, groups, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05, overlap_forward=True)
    gen = torch.Generator(device=dev).manual_seed(1234)
    imgs = [torch.randn(args.batch, 3, 224, 224, generator=gen, device=dev) for _ in range(4)]
    labels = (torch.rand(16, args.batch, generator=gen, device=dev) < 0.5).long()
    pw = torch.tensor(1.0, device=dev)
    tick = [0]

    def step(max_norm):
        i = tick[0]
        tick[0] += 1
        opt.zero_grad(set_to_none=True)
        A.supervised_loss(model(imgs[i % 4]), labels[i % 16], pos_weight=pw).backward()
        opt.step(**({} if max_norm is None else {"max_norm": max_norm}))

    for _ in range(10):
        step(None)
    torch.cuda.synchronize()
    ms = {"plain": [], "max_norm": []}
    for _ in range(args.rounds):
        for kind, mn in (("plain", None), ("max_norm", 1e30)):
            step(mn)
            torch.cuda.synchronize()
            ms[kind].append(events_us(torch, lambda: step(mn), args.steps) / 1e3)
    out = {"batch": args.batch, "steps_per_window": args.steps, "ms_per_step": ms}
    for kind, v in ms.items():
        out[kind + "_median_ms"] = statistics.median(v)
        print(f"cls bs={args.batch} step, {kind}: median {statistics.median(v):.3f} ms of {v}")
    out["extra_us_median"] = (out["max_norm_median_ms"] - out["plain_median_ms"]) * 1e3
    out["last_clip"] = opt.last_clip.tolist()
    print(f"extra per clipped step: {out['extra_us_median']:.1f} us (medians); last_clip {out['last_clip']}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ssl4polyp_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench: no GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "statistics_pass": stats_pass(torch, _lib, args.calls),
              "cls_step": step_cost(torch, args)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
