"""What timm's RandAugment and random erasing cost on the device at the ViT-B/16 fine-tune shapes (B = 64, 224 x 224): what
profiles/timm_aug.json records.

    python tools/timm_aug_bench.py [--batch 64] [--rounds 4] [--out profiles/timm_aug.json]

  launches   every new launch singly, device events, us per call: pm_randaug_stats (all samples need statistics: the worst case),
             pm_randaug_apply with the whole batch on ONE op (per op: the branches differ by two orders of magnitude in arithmetic)
             and on a drawn rand-m9-mstd0.5-inc1 layer, pm_random_erase_f32 (pixel mode, boxes drawn at probability 0.25 and 1).
  host       RandAugment.draw + RandomErasing.draw for one batch, host clock (Python; runs ahead of the device in the loop).
  tails      DeviceAugmenter.timm_tail (draws included) against mae_tail on the same cropped batch, alternating windows.
  step       the recipe step of tools/finetune_mae_bench.py behind either tail, alternating windows in one process.
The bench.py headline does not run this code; it is measured by bench.py itself on this commit and its parent."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from finetune_mae_bench import build, five, window  # noqa: E402
from ssl4polyp_amd import _lib, timm_aug as TA  # noqa: E402
from ssl4polyp_amd.data import IMAGENET_MEAN, DeviceAugmenter  # noqa: E402

DEV = torch.device("cuda", 0)
CONFIG = "rand-m9-mstd0.5-inc1"
ONE_OP = [("Identity", None), ("AutoContrast", None), ("Equalize", None), ("Invert", None), ("ColorIncreasing", 1.81),
          ("ContrastIncreasing", 1.81), ("BrightnessIncreasing", 1.81), ("SharpnessIncreasing", 1.81), ("Rotate", 27.0),
          ("ShearX", 0.27), ("TranslateXRel", 0.405), ("Rotate", 180.0)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def launches(B, S, calls):
    lib, ck = _lib.load(), _lib.check
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, 3), device=DEV, generator=g, dtype=torch.uint8)
    y = torch.empty_like(x)
    ws_bytes = _lib.workspace_bytes("pm_randaug_workspace", B)
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device=DEV)
    frame_bytes = 2 * x.numel()
    out = {"bytes_read_plus_written_per_apply": frame_bytes}

    def plan_of(records):
        p = np.stack(records).astype(TA.OP_DTYPE).reshape(B)
        return torch.from_numpy(p.view(np.uint8).reshape(B, 64).copy()).to(DEV)

    stats_plan = plan_of([TA.op_record(("AutoContrast", "Equalize", "ContrastIncreasing")[b % 3], 1.81, S, S) for b in range(B)])
    out["pm_randaug_stats_all_samples"] = five(torch, lambda: ck(lib.pm_randaug_stats(x.data_ptr(), stats_plan.data_ptr(), 1, ws.data_ptr(),
                                                                                       ws_bytes, B, S, S, stream()), "stats"), calls)
    for name, arg in ONE_OP:
        plan = plan_of([TA.op_record(name, arg, S, S)] * B)
        key = f"pm_randaug_apply_{name}" + ("_180" if arg == 180.0 else "")
        out[key] = five(torch, lambda: ck(lib.pm_randaug_apply(x.data_ptr(), y.data_ptr(), plan.data_ptr(), 1, None, ws.data_ptr(), ws_bytes,
                                                               B, S, S, 124, 116, 104, stream()), "apply"), calls)
    ra = TA.RandAugment(CONFIG, IMAGENET_MEAN)
    drawn = ra.draw(B, np.random.RandomState(0), S)
    plan = torch.from_numpy(np.ascontiguousarray(drawn).view(np.uint8).reshape(B, 128).copy()).to(DEV)
    out["pm_randaug_apply_drawn_layer"] = five(torch, lambda: ck(lib.pm_randaug_apply(
        x.data_ptr(), y.data_ptr(), plan.data_ptr(), 2, None, ws.data_ptr(), ws_bytes, B, S, S, 124, 116, 104, stream()), "apply"), calls)
    out["drawn_layer_ops"] = {int(k): int(v) for k, v in zip(*np.unique(drawn["op"][:, 0], return_counts=True))}
    f = torch.randn(B, 3, S, S, device=DEV)
    for p in (0.25, 1.0):
        boxes = TA.RandomErasing(p).draw(B, (3, S, S), np.random.RandomState(1))
        bd = torch.from_numpy(boxes).to(DEV)
        r = five(torch, lambda: ck(lib.pm_random_erase_f32(f.data_ptr(), bd.data_ptr(), 1, 2, 7, 9, B, 3, S, S, stream()), "erase"), calls)
        r["boxes"] = int((boxes[..., 2] > 0).sum())
        r["elements"] = int((boxes[..., 2] * boxes[..., 3]).sum()) * 3
        out[f"pm_random_erase_f32_pixel_p{p}"] = r
    for k, v in out.items():
        if isinstance(v, dict) and "us_median" in v:
            print(f"{k}: {v['us_median']:.1f} us (min {v['us_min']:.1f}, max {v['us_max']:.1f})")
    return out


def host_draws(B, S, n=20):
    aug = TA.TrainAugment(TA.RandAugment(CONFIG, IMAGENET_MEAN), TA.RandomErasing(0.25))
    aug.reseed(0, 0)
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        aug.rand_augment.draw(B, aug.rng, S)
        aug.random_erasing.draw(B, (3, S, S), aug.rng)
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"host draws per batch: median {statistics.median(t):.2f} ms")
    return {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}


def tails_and_steps(B, S, rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randint(0, 256, (B, S, S, 3), device=DEV, generator=g, dtype=torch.uint8)
    augm = DeviceAugmenter(DEV, size=S)
    ta = TA.TrainAugment(TA.RandAugment(CONFIG, IMAGENET_MEAN), TA.RandomErasing(0.25))
    ta.reseed(0, 0)
    gen = torch.Generator().manual_seed(0)
    out_a, out_b = torch.empty(B, 3, S, S, device=DEV), torch.empty(B, 3, S, S, device=DEV)
    tail_new = lambda: augm.timm_tail(x, ta, generator=gen, out=out_a)  # noqa: E731
    tail_old = lambda: augm.mae_tail(x, generator=gen, out=out_b)      # noqa: E731
    res = {"timm_tail_ms": [], "mae_tail_ms": [], "step_behind_timm_tail_ms": [], "step_behind_mae_tail_ms": []}
    for _ in range(rounds):
        res["timm_tail_ms"].append(window(torch, tail_new, 200.0))
        res["mae_tail_ms"].append(window(torch, tail_old, 200.0))
    _, _, step = build(torch, B, 1000, True)

    def with_new():
        tail_new()
        step()

    def with_old():
        tail_old()
        step()

    for fn in (with_new, with_old):
        for _ in range(3):
            fn()
    for _ in range(rounds):
        res["step_behind_timm_tail_ms"].append(window(torch, with_new))
        res["step_behind_mae_tail_ms"].append(window(torch, with_old))
    for k in list(res):
        res[k.replace("_ms", "_median_ms")] = statistics.median(res[k])
    res["tail_added_ms"] = res["timm_tail_median_ms"] - res["mae_tail_median_ms"]
    res["step_added_ms"] = res["step_behind_timm_tail_median_ms"] - res["step_behind_mae_tail_median_ms"]
    res["step_added_share"] = res["step_added_ms"] / res["step_behind_mae_tail_median_ms"]
    res["how"] = ("alternating windows in one process, device events around each window after a warm-up; the tails include the host "
                  "draws and the record uploads (the wall time of a window, seen by the events, is the larger of host and device work)")
    print(f"timm_tail {res['timm_tail_median_ms']:.3f} ms, mae_tail {res['mae_tail_median_ms']:.3f} ms; recipe step behind them "
          f"{res['step_behind_timm_tail_median_ms']:.3f} / {res['step_behind_mae_tail_median_ms']:.3f} ms "
          f"(+{100 * res['step_added_share']:.2f} %)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "size": a.size, "config": CONFIG, "tool": "tools/timm_aug_bench.py"}
    res["launches_us"] = launches(a.batch, a.size, a.calls)
    res["host_draws"] = host_draws(a.batch, a.size)
    res["tails_and_recipe_step"] = tails_and_steps(a.batch, a.size, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
