"""Stand-alone times of the two stochastic-depth row kernels at [64 * 197, 768] and the recipe step at drop_path_rate 0.1 against 0.0
(one build, alternating windows): what profiles/drop_path.json records.

    python tools/drop_path_bench.py --out drop_path_measure.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssl4polyp_amd import _lib, models_vit  # noqa: E402

DEV = torch.device("cuda", 0)
res = {"device": torch.cuda.get_device_name(0)}


def stream():
    return torch.cuda.current_stream().cuda_stream


def timed(fn, sets, calls=60, windows=7):
    """median / min / max microseconds per call over `windows` windows of `calls` calls, rotating over `sets` argument sets."""
    for i in range(2 * sets):
        fn(i % sets)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fn(i % sets)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return {"us_median": statistics.median(out), "us_min": min(out), "us_max": max(out)}


def kernels():
    lib = _lib.load()
    B, N, D = 64, 197, 768
    M = B * N
    s = (torch.rand(B, device=DEV) < 0.9).float() / 0.9
    SETS = 6   # 6 x (2 or 3) x 38.7 MB: past the 256 MB last-level cache
    xs = [torch.randn(M, D, device=DEV) for _ in range(SETS)]
    ys = [torch.randn(M, D, device=DEV) for _ in range(SETS)]
    outs = [torch.empty(M, D, device=DEV) for _ in range(SETS)]
    acts = [torch.empty(M, D, device=DEV, dtype=torch.bfloat16) for _ in range(SETS)]
    col = torch.zeros(D, device=DEV)
    need = _lib.workspace_bytes("pm_drop_path_workspace", M, D)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ck = _lib.check

    def add_in_place(i):
        ck(lib.pm_drop_path_add(xs[i].data_ptr(), ys[i].data_ptr(), ys[i].data_ptr(), s.data_ptr(), M, N, D, stream()), "add")

    def add_out(i):
        ck(lib.pm_drop_path_add(xs[i].data_ptr(), ys[i].data_ptr(), outs[i].data_ptr(), s.data_ptr(), M, N, D, stream()), "add")

    def cast_sum(i):
        ck(lib.pm_drop_path_scale_cast(xs[i].data_ptr(), s.data_ptr(), acts[i].data_ptr(), _lib.PM_BF16, col.data_ptr(), M, N, D,
                                       ws.data_ptr(), need, stream()), "cast")

    def cast_only(i):
        ck(lib.pm_drop_path_scale_cast(xs[i].data_ptr(), s.data_ptr(), acts[i].data_ptr(), _lib.PM_BF16, None, M, N, D, None, 0,
                                       stream()), "cast")

    # references on the same buffers: the existing column sum (reads f32) and a plain device copy
    def colsum_ref(i):
        ck(lib.pm_colsum_ws(xs[i].data_ptr(), D, _lib.PM_F32, col.data_ptr(), M, D, ws.data_ptr(), need, stream()), "colsum")

    def copy_ref(i):
        outs[i].copy_(xs[i])

    out = {}
    for name, fn, nbytes in (("drop_path_add_in_place", add_in_place, 3 * M * D * 4), ("drop_path_add", add_out, 3 * M * D * 4),
                             ("drop_path_scale_cast_bf16_colsum", cast_sum, M * D * 6 + 2 * need),
                             ("drop_path_scale_cast_bf16", cast_only, M * D * 6),
                             ("ref_pm_colsum_f32", colsum_ref, M * D * 4), ("ref_torch_copy_f32", copy_ref, 2 * M * D * 4)):
        r = timed(fn, SETS)
        r["bytes"] = nbytes
        r["TB_per_s_median"] = nbytes / r["us_median"] / 1e6
        out[name] = r
        print(name, r, flush=True)
    res["kernels_at_12608x768"] = out


def recipe():
    from ssl4polyp_amd.lr_decay import param_groups_lrd
    from ssl4polyp_amd.mixup import Mixup, soft_target_ce
    from ssl4polyp_amd.optim import FusedAdamW
    B, C = 64, 1000
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    target = torch.randint(0, C, (B,), generator=g).to(DEV)
    runs = {}
    for rate in (0.0, 0.1):
        torch.manual_seed(0)
        m = models_vit.vit_base_patch16(num_classes=C, global_pool=True, precision="bf16", drop_path_rate=rate).to(DEV)
        torch.nn.init.trunc_normal_(m.head.weight, std=2e-5)
        m.train()
        groups = param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75, with_names=True)
        opt = FusedAdamW(m, groups, lr=1e-4)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C, rng=np.random.RandomState(2))
        runs[rate] = (m, opt, mix)

    def step(rate):
        m, opt, mix = runs[rate]
        x, y = mix(imgs, target)
        opt.zero_grad(set_to_none=True)
        loss = soft_target_ce(m(x), y, mix.state, 0.1)
        loss.backward()
        opt.step()
        return loss

    series = {0.0: [], 0.1: []}
    for rate in (0.0, 0.1):
        for _ in range(10):
            step(rate)
    torch.cuda.synchronize()
    for w in range(8):
        for rate in ((0.0, 0.1) if w % 2 == 0 else (0.1, 0.0)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(25):
                loss = step(rate)
            torch.cuda.synchronize()
            series[rate].append((time.perf_counter() - t0) * 1e3 / 25)
            assert bool(torch.isfinite(loss))
    med = {r: statistics.median(v) for r, v in series.items()}
    res["recipe_step_vitb16_bf16_bs64_1000cls"] = {
        "what": "mix -> forward -> soft CE -> backward -> FusedAdamW over layer-decay groups; 8 alternating windows of 25 steps, host "
                "clock around a device synchronise",
        "rate_0.0_ms": series[0.0], "rate_0.1_ms": series[0.1], "rate_0.0_median_ms": med[0.0], "rate_0.1_median_ms": med[0.1],
        "added_ms": med[0.1] - med[0.0], "added_share_of_step": (med[0.1] - med[0.0]) / med[0.0],
        "dropped_blocks": 11, "row_kernel_launches_added_per_step": 11 * 4}
    print(res["recipe_step_vitb16_bf16_bs64_1000cls"], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="drop_path_measure.json")
    args = ap.parse_args()
    kernels()
    recipe()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
