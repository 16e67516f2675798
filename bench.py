#!/usr/bin/env python3
"""bench.py -- training-step throughput of the MI355X hot path on synthetic Hyperkvasir-shaped batches.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cls|mae] [--precision bf16|fp32] [--full]
                    [--dump-outputs DIR]
        (N > 1 without a launcher: this process starts the N ranks itself, one per GPU -- self_launch below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" = zero_grad -> forward -> loss -> backward (-> RCCL gradient all-reduce) -> fused AdamW, inputs
resident in HBM.  Headline workload = BASELINE.json configs[1]: ViT-B/16 classification
fine-tune, bf16, bs=64/GPU, 224^2.  A plain run measures the headline only: set-up, pre-heat + W warm-up steps, K timed
steps, and rank 0 prints ONE JSON line (`metric`, `value`, `unit`, `ms_per_step`, `dtype`, the step-time spread and the
roofline fraction the step time implies).  The pre-heat runs until the clocks have settled, so its step count varies; the
training state is put back to the initial weights and optimizer state after it (then a fixed RESETTLE_STEPS steps), so
that the steps from there on, warm-up and timed ones, are the same computation in every run.
--dump-outputs DIR writes what the last timed step handed its caller (loss, logits or MAE pred / mask, seeded samples of the
updated parameters and of their gradients) as float32 .npy files: two builds can be compared output for output.
--full adds everything else the line used to carry: BASELINE.json's metric names both halves ("MAE pretrain + cls finetune"),
so it also measures configs[2] (MAE pre-train, mask 0.75, bs=256/GPU) in the same process and reports it as the `mae`
sub-record, beside the fp16 / fp32 / ViT-H / C5 sub-records, the host enqueue time, and
  `roofline`      achieved algorithmic TFLOP/s vs the 2.5 PFLOP/s dense bf16 MFMA peak, plus the dominant kernel's own
                  live-measured average duration (HIP events on the stream the kernel runs on),
  `parity`        the HIP path's logits / loss / gradient errors against the CPU oracle on the benched configuration,
  `cpu_baseline`  the CPU oracle timed on this host (the reported baseline, never the target),
  `torch_baseline` stock PyTorch-ROCm (bf16 autocast, SDPA, fused AdamW) on the same synthetic step, for context.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# algorithmic GFLOP per image per training step (contractions only, step = 3 x forward)
GFLOP_PER_IMG = {"cls": 105.38, "mae": 58.16}
# C5 regimes (BASELINE.md §3 / SURVEY 8-d): forward 35.13 GFLOP/img; a trainable block adds its backward = 2 x its forward
# (1.454 GMAC = 2.908 GFLOP) -- dgrad + wgrad; linear probe is forward + head only
FWD_GFLOP_PER_IMG, BLOCK_FWD_GFLOP = 35.13, 2.908
FINETUNE_GFLOP = {"none": FWD_GFLOP_PER_IMG, "head+1": FWD_GFLOP_PER_IMG + 2 * BLOCK_FWD_GFLOP,
                  "head+2": FWD_GFLOP_PER_IMG + 4 * BLOCK_FWD_GFLOP, "full": 105.38}
PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3}  # MI355X_MICROARCH.md: dense bf16 / fp16 MFMA (same rate), f32 MFMA
PEAK_HBM_GBPS = 8000.0                         # MI355X_MICROARCH.md: HBM3E
# AdamW on the side stream beside the next forward: +0.5 % on the fine-tune step and +0.6 % on the MAE step under the final stream
# layout (scratch/archive_r3/r3_exp31.sh; with a stream set per model and the update sharing a hardware queue it cost the MAE step 1.3 %);
# PM_OVERLAP_ADAMW=0/1 forces either
OVERLAP_ADAMW = {"cls": os.environ.get("PM_OVERLAP_ADAMW", "1") != "0", "mae": os.environ.get("PM_OVERLAP_ADAMW", "1") != "0"}
MAE_IT_PER_EPOCH = 390  # ~100 k unlabelled frames / 256 per step
WORKLOAD_NAME = {"cls": "ViT-B/16 classification fine-tune", "mae": "MAE pre-train ViT-B/16 mask 0.75"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", choices=["cls", "mae"], default="cls")
    ap.add_argument("--precision", choices=["bf16", "fp16", "fp32"], default="bf16",
                    help="fp16 = the reference's AMP arithmetic (fp16 MFMA operands, f32 accumulation, device-side dynamic loss scaling)")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default 64 cls / 256 mae)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle parity block (CPU time)")
    ap.add_argument("--no-mae", action="store_true", help="cls headline only (no MAE sub-records)")
    ap.add_argument("--no-vith", action="store_true", help="no mae_vit_huge_patch14 sub-record")
    ap.add_argument("--no-fp16", action="store_true", help="skip the precision-mode fp16 sub-records (cls bs=64, MAE bs=256)")
    ap.add_argument("--no-fp32", action="store_true", help="skip the short fp32-mode (exact-f32 MFMA) cls record")
    ap.add_argument("--single-batch", action="store_true",
                    help="A/B switch: train on ONE resident batch with fixed labels, as rounds 1-3 did (the fine-tune memorises it: "
                         "loss -> 1e-5, all-zero dlogits in the linear-probe regimes); default: 8 resident image batches x 64 label "
                         "vectors, a new pairing every step, so that the loss stays O(0.7)")
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--cpu-full", action="store_true",
                    help="SURVEY 8-d protocol in full for the CPU baseline (>=3 warm-up + >=10 timed steps at bs=8 AND bs=64, "
                         "all cores and 8 threads): several minutes of CPU time")
    ap.add_argument("--lr-every-step", action="store_true",
                    help="change the learning rate before every step, as engine_pretrain.py:47-48 does (exercises the "
                         "non-blocking hyper-parameter upload)")
    ap.add_argument("--input", choices=["resident", "host"], default="resident",
                    help="resident (the contract: batch already in HBM) or host: uint8 HWC frames in pinned host memory, "
                         "copied and normalised on a side stream each step (PCIe-inclusive rate, DESIGN.md)")
    ap.add_argument("--augment", choices=["none", "device"], default="none",
                    help="with --input host: `device` feeds decoded 576x720 uint8 frames and runs the reference's whole train "
                         "transform (Resize, ColorJitter, GaussianBlur(25), flips, RandomRotation(180), ToTensor, Normalize: "
                         "classification/data/transforms.py:234-246) on the copy stream (data.DeviceAugmenter)")
    ap.add_argument("--host-busy", type=int, default=0,
                    help="also measure host enqueue time and step rate while this many spinning processes compete for the host's "
                         "cores (the 8-ranks-on-one-host picture from a one-GPU box): reported as `busy_host`")
    ap.add_argument("--preheat", type=float, default=1.0,
                    help="seconds of untimed steps before the W warm-up steps (clock / power ramp after process start; 0 = none)")
    ap.add_argument("--finetune-mode", choices=["none", "head+1", "head+2", "full"], default="full",
                    help="C5 regime of the cls workload (classification/finetune.py:49-91): linear probe / lin_head + the last 1 or "
                         "2 blocks / everything.  The default line (full) also carries the other three as `finetune_modes`")
    ap.add_argument("--force-sync", action="store_true",
                    help="N=1 only: run the bucketed RCCL gradient all-reduces at world size 1 (the multi-GPU stream schedule -- "
                         "comm stream, RCCL's own stream -- on one GPU: what the data-parallel path costs before any link is involved)")
    ap.add_argument("--no-c5", action="store_true", help="skip the `finetune_modes` sub-records (none / head+1 / head+2 + eval)")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the step as one hipGraph (auto = off: eager launch keeps up and overlaps the two streams better)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: sub-records (fp16, fp32, MAE, ViT-H, C5), per-kernel statistics, host "
                         "enqueue time, oracle parity + gates, CPU and PyTorch baselines (the --no-* options trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (float32 .npy, seeded samples of the large "
                         "arrays, < 64 MB in all) to DIR")
    return ap.parse_args()


def mae_gflop_per_img(m, mask_ratio=0.75):
    """Algorithmic GFLOP per image per MAE training step of any factory (contractions only, step = 3 x forward -- BASELINE.md section 3's
    convention; gives 58.16 for mae_vit_base_patch16): patch embedding on the kept patches, 12 D^2 + 2 N D MACs per token and block."""
    pe = m.patch_embed
    L, p = pe.num_patches, pe.patch_size[0]
    keep = int(L * (1 - mask_ratio))
    De, Dd = m.cls_token.shape[-1], m.mask_token.shape[-1]
    stack = lambda D, N, depth: depth * N * (12 * D * D + 2 * N * D)
    macs = keep * 3 * p * p * De + stack(De, keep + 1, len(m.blocks)) + (keep + 1) * De * Dd + \
        stack(Dd, L + 1, len(m.decoder_blocks)) + (L + 1) * Dd * 3 * p * p
    return 3 * 2 * macs / 1e9


def build(workload, precision, device, world, batch, finetune_mode="full", force_sync=False, factory=None):
    import ssl4polyp_amd as A
    from ssl4polyp_amd.optim import FusedAdamW, LossScaler, add_weight_decay
    from ssl4polyp_amd.parallel import DataParallel
    from ssl4polyp_amd.train import configure_finetune_parameters
    torch.manual_seed(0)  # identical init on every rank (then broadcast from rank 0 anyway)
    if workload == "cls":
        model = A.get_MAE_backbone(None, True, 2, False, None, precision=precision)
        # tc.py:5735-5740: configure_finetune_parameters(model, initial_mode) on whatever the factory returned -- "full" makes
        # EVERY parameter trainable (the sincos pos_embed too), the other modes freeze everything but lin_head (+ tail blocks)
        configure_finetune_parameters(model, finetune_mode)
    else:
        # factory: another of models_mae.py:223-250's factories (mae_vit_large_patch16, mae_vit_huge_patch14) as a sub-record
        model = getattr(A, factory or "mae_vit_base_patch16")(norm_pix_loss=False, precision=precision)
    ddp = DataParallel(model, device, force_sync=force_sync)
    if workload == "cls":
        # tc.py:5751-5768: AdamW(lr 1e-3, wd 0.05) over two groups head / backbone (config/base.yaml:1-4), built from ALL
        # parameters: frozen ones stay in the optimizer and are skipped for want of a gradient
        head = list(model.lin_head.parameters())
        hid = {id(p) for p in head}
        groups = [{"params": head, "name": "head"},
                  {"params": [p for p in model.parameters() if id(p) not in hid], "name": "backbone"}]
        opt = FusedAdamW(model, groups, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05, overlap_forward=OVERLAP_ADAMW["cls"])
    else:
        # main_pretrain.py:201-218: lr = blr * eff_batch / 256, betas (0.9, 0.95), no decay on 1-D params
        lr = 1e-3 * batch * world / 256
        opt = FusedAdamW(model, add_weight_decay(model, 0.05), lr=lr, betas=(0.9, 0.95), overlap_forward=OVERLAP_ADAMW["mae"])
    opt.grad_sync = ddp.sync
    opt.grad_scale = 1.0 / world
    # precision mode fp16: the reference's GradScaler() (tc.py:5973-5974, main_pretrain.py:219), resident on the device
    opt.loss_scaler = LossScaler() if precision == "fp16" else None
    return model, ddp, opt


N_IMG_BATCHES, N_LABEL_SETS = 8, 64


def make_batch(workload, batch, device, rank, pool=False):
    """SURVEY 8-d synthetic inputs: post-Normalize images N(0, 1), labels Bernoulli(0.5), generator seeded 1234 + rank.
    pool: 8 resident image batches and 64 label vectors ([64, B]); the step pairs image batch i % 8 with label vector i % 64, so a
    pairing repeats only every 64 steps and the labels are never learnable (rounds 1-3 trained ONE batch: the fine-tune memorised it
    within ~100 steps -- loss 1e-5, in the frozen-backbone regimes exactly 0 and with it all-zero dlogits in the timed region)."""
    g = torch.Generator(device=device).manual_seed(1234 + rank)
    if not pool:
        imgs = torch.randn(batch, 3, 224, 224, generator=g, device=device)
        labels = (torch.rand(batch, generator=g, device=device) < 0.5).long()
        return imgs, labels
    imgs = [torch.randn(batch, 3, 224, 224, generator=g, device=device) for _ in range(N_IMG_BATCHES)]
    labels = (torch.rand(N_LABEL_SETS, batch, generator=g, device=device) < 0.5).long()
    return imgs, labels


def make_step(workload, ddp, opt, imgs, labels, lr_every_step=False, noise_buf=None):
    import ssl4polyp_amd as A
    pos_weight = torch.tensor(1.0, device=(imgs[0] if isinstance(imgs, (list, tuple)) else imgs).device)
    base_lr = [g["lr"] for g in opt.param_groups]
    counter = [0]

    def touch_lr():
        if workload == "mae":
            # engine_pretrain.py:47-48: lr_sched.adjust_learning_rate(optimizer, data_iter_step / len(data_loader) + epoch)
            # before EVERY iteration -- the reference's 40 warm-up epochs (main_pretrain.py:78-79), MAE_IT_PER_EPOCH iterations
            # each.  At a constant 1e-3 from step 0 the pre-train diverges after a few hundred steps (non-finite loss at
            # --steps 400); the kernels do the same work whatever the value in the device-side hyper-parameter slot.
            from ssl4polyp_amd.train import mae_lr
            f = mae_lr(counter[0] / MAE_IT_PER_EPOCH, 1.0, 0.0, 40, 400)
            counter[0] += 1
            for g, b in zip(opt.param_groups, base_lr):
                g["lr"] = b * f
        elif lr_every_step:  # the fine-tune schedule steps per epoch (tc.py:3952-3957); this flag changes lr every step anyway
            counter[0] += 1
            f = 1.0 - 1e-4 * (counter[0] % 7)
            for g, b in zip(opt.param_groups, base_lr):
                g["lr"] = b * f

    scaler = getattr(opt, "loss_scaler", None)
    pooled = isinstance(imgs, (list, tuple))
    tick = [0]

    def pick(im, lb):
        if im is not None:          # (--input host: the prefetcher hands the batch over)
            return im, lb
        if not pooled:
            return imgs, labels
        i = tick[0]
        tick[0] = i + 1
        return imgs[i % len(imgs)], labels[i % labels.shape[0]]

    def finish(loss):
        # tc.py:4533-4546 / engine_pretrain.py:65-72: scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        return loss

    outputs = {}  # the forward's results of the latest step (detached views, no copy): --dump-outputs

    if workload == "cls":
        def step(im=None, lb=None):
            im, lb = pick(im, lb)
            touch_lr()
            opt.zero_grad(set_to_none=True)
            logits = ddp(im)
            outputs["logits"] = logits.detach()
            return finish(A.supervised_loss(logits, lb, pos_weight=pos_weight))  # tc.py:3347-3374, 6090-6102 (one HIP launch)
    else:
        def step(im=None, lb=None):
            im, lb = pick(im, lb)
            touch_lr()
            opt.zero_grad(set_to_none=True)
            # noise_buf: hipGraph replay -- the masking noise must come from a buffer the caller refills between replays (a draw
            # inside the captured region would be baked into the graph)
            loss, pred, mask = ddp(im, mask_ratio=0.75, **({"noise": noise_buf} if noise_buf is not None else {}))
            outputs.update(pred=pred.detach(), mask=mask.detach())
            return finish(loss)

    def rewind():
        """Back to the first step's batch pairing and learning-rate schedule position."""
        counter[0] = tick[0] = 0

    step.outputs, step.rewind = outputs, rewind
    return step


def kernel_stats(model, step):
    """Per-launch HIP-event timing of the GEMMs, LayerNorms and attention calls of one step (events recorded on the stream
    each kernel is launched on)."""
    k = model._rt.k
    block_calls = k.BLOCK_CALLS
    k.BLOCK_CALLS = False  # the instrumented steps issue every forward kernel as its own call (same launches), so the hooks see them
    orig = dict(gemm=k.gemm, lnf=k.layernorm_fwd, lnb=k.layernorm_bwd, af=k.attention_fwd, ab=k.attention_bwd, wg=k.wgrad_group)
    rec, hbm, att = [], [], []
    act_b = 4 if k.precision == "fp32" else 2

    def ev2():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    EPI = {0: "store", 1: "gelu", 2: "residual", 3: "dgelu", 4: "accum"}

    def gemm(A, lda, akm, B, ldb, bkm, bias, C, ldc, epi, M, N, K, **kw):
        e0, e1 = ev2()
        e0.record(); orig["gemm"](A, lda, akm, B, ldb, bkm, bias, C, ldc, epi, M, N, K, **kw); e1.record()
        # class = operand layout + epilogue: the dispatcher sends each to its own template instantiation (rocprof lists them
        # as separate kernels), so the "dominant kernel" below is a kernel symbol, not a merge of several
        lay = ("tn" if akm else "n") + ("n" if bkm else "t")
        rec.append((lay if akm else f"{lay}_{EPI.get(epi, epi)}", M, N, K, e0, e1))

    held = []  # (CUs the launch holds, flops, e0, e1) of the grouped weight-gradient launches

    def group_cus(dims, K, whole_k):
        """Workgroups (= CUs: one 128-KB LDS ring each) of a pm_wgrad_group launch over (n_out, n_in) problems: tiles of 256x256 x
        the library's k-slices."""
        import ctypes
        from ssl4polyp_amd import _lib
        arr = (_lib.WgradItem * len(dims))()
        for j, (o, i) in enumerate(dims):
            arr[j] = _lib.WgradItem(64, o, 64, i, 64, i, o, i, 0, None)
        tiles, slices = ctypes.c_int(0), ctypes.c_int(0)
        k.lib.pm_wgrad_group_plan(arr, len(dims), K, k.act, None, ctypes.byref(tiles), ctypes.byref(slices))
        work = tiles.value * (1 if whole_k else max(slices.value, 1))
        cap = k.GROUP_BLOCKS if (whole_k or slices.value <= 1) else k.GROUP_BLOCKS_SLICED
        return min(256, work if cap <= 0 else min(work, cap))

    def wgrad_group(items, K, **kw):
        e0, e1 = ev2()
        e0.record(); ok = orig["wg"](items, K, **kw); e1.record()
        if ok:
            mn = sum(it[2].shape[0] * it[2].shape[1] for it in items)
            rec.append(("wgrad_group", mn, 1, K, e0, e1))
            held.append((group_cus([tuple(it[2].shape) for it in items], K, bool(kw.get("whole_k"))), 2.0 * mn * K, e0, e1))
        return ok

    def ln_fwd(x, gamma, beta, y, mean, rstd, M, D):
        e0, e1 = ev2()
        e0.record(); orig["lnf"](x, gamma, beta, y, mean, rstd, M, D); e1.record()
        hbm.append(("layernorm_fwd", M * D * (4 + act_b), e0, e1))

    def ln_bwd(dy, x, gamma, mean, rstd, dres, dx, dx_act, dgamma, dbeta, dcolsum, M, D):
        e0, e1 = ev2()
        e0.record(); orig["lnb"](dy, x, gamma, mean, rstd, dres, dx, dx_act, dgamma, dbeta, dcolsum, M, D); e1.record()
        hbm.append(("layernorm_bwd", M * D * (act_b + 4 + 4 + 4 + act_b), e0, e1))

    def attn_fwd(qkv, out, lse, B, N, H, dh):
        e0, e1 = ev2()
        e0.record(); orig["af"](qkv, out, lse, B, N, H, dh); e1.record()
        att.append(("attention_fwd", 4.0 * B * H * N * N * dh, e0, e1))

    def attn_bwd(qkv, out, dout, lse, delta, dqkv, B, N, H, dh):
        e0, e1 = ev2()
        e0.record(); orig["ab"](qkv, out, dout, lse, delta, dqkv, B, N, H, dh); e1.record()
        att.append(("attention_bwd", 10.0 * B * H * N * N * dh, e0, e1))

    k.gemm, k.layernorm_fwd, k.layernorm_bwd, k.attention_fwd, k.attention_bwd = gemm, ln_fwd, ln_bwd, attn_fwd, attn_bwd
    k.wgrad_group = wgrad_group
    try:
        for _ in range(3):
            rec.clear(); hbm.clear(); att.clear(); held.clear()
            step()
        torch.cuda.synchronize()
    finally:
        k.gemm, k.layernorm_fwd, k.layernorm_bwd = orig["gemm"], orig["lnf"], orig["lnb"]
        k.attention_fwd, k.attention_bwd, k.wgrad_group = orig["af"], orig["ab"], orig["wg"]
        k.BLOCK_CALLS = block_calls

    def fold(items, unit):
        d = {}
        for name, work, e0, e1 in items:
            v = d.setdefault(name, [0, 0.0, 0.0])
            v[0] += 1
            v[1] += e0.elapsed_time(e1) * 1e-3
            v[2] += work
        out = {}
        for n, (c, t, w) in d.items():
            if unit == "GBps":
                out[n] = {"launches": c, "avg_us": round(t / c * 1e6, 2), "GBps": round(w / t / 1e9, 1),
                          "frac_of_hbm_peak": round(w / t / 1e9 / PEAK_HBM_GBPS, 3)}
            else:
                out[n] = {"launches": c, "avg_us": round(t / c * 1e6, 2), "tflops": round(w / t / 1e12, 1)}
        return out

    # The grouped weight-gradient launches once more, in the schedule the TIMED steps use (pm_vit_block_bwd: one C call per block,
    # which the hooks above cannot see): its fork / done events carry timestamps for three steps; fork -> done on a side stream that
    # is idle by then = the launch (+ the reduce launch behind a k-sliced group).
    if block_calls and any(r[0] == "wgrad_group" for r in rec):
        k.TIME_BLOCK_EVENTS = True
        try:
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            fast = []
            for lst in model._rt.pool.values():
                for ws in lst:
                    for key, desc, evs_done, keep in ws.__dict__.get("_bwd_descs", {}).values():
                        if not key[-3]:  # (descriptors built before the switch: not used by these steps)
                            continue
                        M, D, Hd = desc.samples * desc.N, desc.D, desc.Hd
                        dims = ((D, Hd), (Hd, D), (D, D), (3 * D, D))
                        parts = ((dims[:2], keep[0], evs_done[0], False), (dims[2:], keep[1], evs_done[1], True)) if desc.two_groups \
                            else ((dims, keep[0], evs_done[0], False),)
                        for dd, e0, e1, whole in parts:
                            fast.append((group_cus(dd, M, whole), 2.0 * M * sum(o * i for o, i in dd), e0, e1))
            if fast:
                rec[:] = [r for r in rec if r[0] != "wgrad_group"] + [("wgrad_group", f / 2.0, 1, 1, e0, e1) for _, f, e0, e1 in fast]
                held[:] = fast
        finally:
            k.TIME_BLOCK_EVENTS = False
    gem = fold([(lay, 2.0 * M * N * K, e0, e1) for lay, M, N, K, e0, e1 in rec], "tflops")
    if held and "wgrad_group" in gem:
        # The grouped launches hold a SUBSET of the CUs on purpose (72 + 36 of 256 for a ViT-B block, two launches side by side), so
        # flops / launch time against the whole chip's peak says how the chip is shared, not how well the kernel runs: also report
        # the rate on the CUs a launch holds, scaled to 256 CUs
        cu_s = sum(c / 256.0 * e0.elapsed_time(e1) * 1e-3 for c, _, e0, e1 in held)
        gem["wgrad_group"]["avg_cus_held"] = round(sum(c for c, *_ in held) / len(held), 1)
        gem["wgrad_group"]["tflops_on_held_cus_x256"] = round(sum(f for _, f, _, _ in held) / cu_s / 1e12, 1)
    tot_t = sum(v["launches"] * v["avg_us"] for v in gem.values()) * 1e-6
    return gem, fold(hbm, "GBps"), fold(att, "tflops"), tot_t


# ---------------------------------------------------------------------------------------------------------------------
# the oracle legs (CPU): baseline timing and parity
# ---------------------------------------------------------------------------------------------------------------------
def physical_cores():
    """(physical cores of the host from lscpu, CPUs this process may run on)."""
    usable = len(os.sched_getaffinity(0))
    try:
        out = subprocess.run(["lscpu", "-p=core,socket"], capture_output=True, text=True, timeout=10).stdout
        phys = len({ln for ln in out.splitlines() if ln and not ln.startswith("#")})
    except Exception:
        phys = 0
    try:  # cgroup CPU quota of the box, if any
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            usable = min(usable, max(1, int(float(q) / float(p) + 0.5)))
    except Exception:
        pass
    return phys, usable


def cpu_baseline(workload, full):
    """The CPU oracle (oracle/vit_mae_ref.py, fp32, torch CPU threads) on a bounded sample of the same workload: synthetic
    batch, reference step order (zero_grad -> fwd -> loss -> bwd -> AdamW), SURVEY 8-d protocol.  Headline figure: bs=8,
    every usable core; also the 8-thread figure (comparable with the survey container) and one bs=64 point."""
    from oracle import vit_mae_ref as O
    cfg = O.VIT_BASE
    phys, usable = physical_cores()
    sd = O.generated_state_dict(cfg, seed=1, decoder=(workload == "mae"), n_class=2 if workload == "cls" else None)
    params = {n: v.clone().requires_grad_("pos_embed" not in n) for n, v in sd.items()}
    leaves = [p for p in params.values() if p.requires_grad]
    opt = torch.optim.AdamW(leaves, lr=1e-3, weight_decay=0.05)

    def run(B, threads, warm, timed):
        torch.set_num_threads(threads)
        imgs, labels, noise = O.generated_batch(cfg, B, seed=2)

        def one():
            opt.zero_grad()
            if workload == "cls":
                loss = O.supervised_loss(O.vit_classify(params, imgs, cfg), labels, 1.0)
            else:
                loss = O.mae_forward(params, imgs, noise, cfg)[0]
            loss.backward()
            opt.step()

        for _ in range(warm):
            one()
        t0 = time.perf_counter()
        for _ in range(timed):
            one()
        dt = time.perf_counter() - t0
        print(f"[bench] cpu baseline: bs={B} threads={threads}: {B * timed / dt:.2f} img/s", file=sys.stderr, flush=True)
        return {"batch": B, "threads": threads, "warmup": warm, "timed_steps": timed, "images_per_sec": round(B * timed / dt, 3)}

    prev = torch.get_num_threads()
    try:
        if full:
            pts = [run(8, usable, 3, 10), run(8, min(8, usable), 3, 10), run(64, usable, 3, 10), run(64, min(8, usable), 3, 10)]
        else:
            pts = [run(8, usable, 3, 10), run(8, min(8, usable), 1, 3), run(64, usable, 1, 2)]
    finally:
        torch.set_num_threads(prev)
    head = pts[0]
    return {"value": head["images_per_sec"], "unit": "images/sec", "cores": usable, "kind": "port",
            "host_physical_cores": phys, "points": pts,
            "sample": f"{head['timed_steps']} timed steps (+{head['warmup']} warm-up) of the fp32 CPU oracle, {workload} ViT-B/16 "
                      f"224^2, bs=8, {usable} threads = the CPUs this box grants the job (host: {phys} physical cores); "
                      "`points` adds the 8-thread and the bs=64 figures (SURVEY 8-d); --cpu-full runs >=10 timed steps for each"}


# Hard gates of the parity block (SURVEY 8-d / the north-star tolerance): the bench exits non-zero when one fails.
#   fp32 mode (exact-f32 MFMA, same kernels' code paths) logits <= 1e-3; MAE loss <= 1e-3; MAE pred rel-L2 <= 1e-2.
# The bf16 classifier numbers are bounded by what bf16 OPERAND ROUNDING alone does to this very configuration, measured in the
# same block by the CPU emulation (oracle/vit_bf16_grad_sim.py, no kernel involved) + 25 % (+ 1e-3 absolute on the logits).
HARD_GATES = {"fp32_mode_logits_max_rel": 1e-3, "mae_loss_rel": 1e-3, "mae_pred_rel_l2": 1e-2}
# precision mode fp16: SURVEY 8-d AS WRITTEN -- loss <= 1e-3, pred and every parameter gradient <= 1e-2 rel-L2 -- and for the logits
# the floor of fp16 OPERAND rounding through 12 blocks, which no kernel can beat: the CPU emulation (oracle/vit_bf16_grad_sim.py FP16,
# no kernel involved; profiles/r4_rounding_fp16_cls_*.json) puts it at 1.30e-3 on the tests' generated weights and 1.63e-3 on this
# bench's fresh initialisation, so the logit gate is 2.0e-3 (floor + 25 %), a fixed number, not derived from what the kernels measure.
# These ARE hard gates: the process exits non-zero when the fp16 record misses one.
FP16_GATES = {"logits_max_rel": 2.0e-3, "loss_rel": 1e-3, "weight_grad_rel_l2_worst": 1e-2, "vector_grad_rel_l2_worst": 1e-2}
PARITY_LOSS_SCALE = 4096.0  # fp16 backward of the parity block: (loss x 2^12).backward(), gradients / 2^12 (exact)


_ORACLE_CACHE = {}  # (weights checksum, batch checksum) -> oracle / emulation results of the cls parity block (C5 sub-records)


def parity_block(workload, model, imgs, labels, precision, light=False):
    """The HIP path against the CPU oracle on the BENCHED configuration: the model's own weights and the benched batch go
    through oracle/vit_mae_ref.py (fp32, CPU); errors as the tests define them (max-rel for logits / loss, rel-L2 for pred
    and parameter gradients).  cls: forward + backward at the full batch, beside (i) the CPU emulation of bf16 operand
    rounding (forward AND backward) and (ii) PyTorch's own bf16 autocast of the oracle on the same tensors, and the
    fp32-mode HIP logits; MAE: forward + loss at the full batch (its backward at B = 256 is compared with a reference-made
    fixture by tests/test_gpu_parity_large.py; minutes of CPU here).  Returns the record with `gates` and `pass`."""
    import ssl4polyp_amd as A
    from oracle import vit_mae_ref as O
    cfg = O.VIT_BASE
    t0 = time.perf_counter()
    _, usable = physical_cores()
    prev = torch.get_num_threads()
    torch.set_num_threads(min(usable, 32))
    model._rt.wait_updates()
    torch.cuda.synchronize()
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}

    def rel(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))

    def rel_l2(a, b):
        a, b = a.double().cpu(), b.double().cpu()
        return float((a - b).norm() / b.norm().clamp_min(1e-30))

    out = {"config": f"{WORKLOAD_NAME[workload]}, bs={imgs.shape[0]}, {precision}", "oracle": "oracle/vit_mae_ref.py fp32 CPU"}
    gates, ok = {}, {}
    try:
        model.zero_grad(set_to_none=True)
        if workload == "cls":
            logits = model(imgs)
            logits.retain_grad()
            loss = A.supervised_loss(logits, labels, pos_weight=1.0)
            gscale = PARITY_LOSS_SCALE if precision == "fp16" else 1.0
            (loss * gscale).backward()
            imgs_c, labels_c = imgs.cpu(), labels.cpu()

            def oracle_run(fn):
                # every parameter is a leaf: mode "full" trains pos_embed too (finetune.py:52-55); decoder_pos_embed is unused
                leaves = {n: v.clone().requires_grad_(True) for n, v in sd.items()}
                z = fn(leaves)
                z.retain_grad()
                lo = O.supervised_loss(z.float(), labels_c, 1.0)
                lo.backward()
                return z.detach().float(), lo.detach(), z.grad.detach().float(), {n: v.grad for n, v in leaves.items() if v.grad is not None}

            ckey = (float(sd["lin_head.weight"].double().sum()), float(sd["blocks.5.mlp.fc1.weight"].double().sum()),
                    float(imgs_c.double().sum()), int(labels_c.sum()))
            cached = _ORACLE_CACHE.get(ckey)
            if cached is None:
                cached = _ORACLE_CACHE[ckey] = {"ref": oracle_run(lambda p: O.vit_classify(p, imgs_c, cfg))}
            lr, lo, dz_ref, g_ref = cached["ref"]

            def grad_errors(grads):
                errs = {n: rel_l2(g, g_ref[n]) for n, g in grads.items()
                        if g is not None and n in g_ref and not n.endswith("attn.qkv.bias")}
                mats = {n: e for n, e in errs.items() if g_ref[n].ndim >= 2 and g_ref[n].shape[0] > 1}
                vecs = {n: e for n, e in errs.items() if n not in mats}
                # g = sum_b dlogit_b * (d logit_b / d theta): on near-identical samples (N(0,1) images) every parameter gradient
                # is ~ (common direction) x sum_b dlogit_b, a CANCELLING sum -- a coherent shift of the logits by the bf16
                # rounding moves that scalar by percents and with it every gradient by the same factor.  alpha = the
                # projection of g on the oracle's gradient, orth = what is left beside that common factor.
                al, orth = {}, {}
                for n in mats:
                    a, b = grads[n].double().cpu().flatten(), g_ref[n].double().flatten()
                    al[n] = float((a @ b) / (b @ b).clamp_min(1e-300))
                    orth[n] = float((a - al[n] * b).norm() / b.norm().clamp_min(1e-300))
                return errs, mats, vecs, al, orth

            hip_grads = {n: p.grad / gscale for n, p in model.named_parameters() if p.grad is not None}
            errs, mats, vecs, al, orth = grad_errors(hip_grads)
            wm, wv = max(mats, key=mats.get), max(vecs, key=vecs.get)
            med = lambda d: sorted(d.values())[len(d) // 2]
            dz_hip = logits.grad.detach().float().cpu() / gscale
            out.update(logits_max_rel=rel(logits.detach(), lr), loss_rel=rel(loss.detach(), lo),
                       dlogits_rel_l2=rel_l2(dz_hip, dz_ref),
                       dlogits_batch_sum_ratio=float(dz_hip[:, 1].double().sum() / dz_ref[:, 1].double().sum()),
                       dlogits_cancellation=float(dz_ref[:, 1].double().abs().sum() / dz_ref[:, 1].double().sum().abs()),
                       weight_grad_rel_l2_worst=mats[wm], weight_grad_rel_l2_worst_name=wm, weight_grad_rel_l2_median=med(mats),
                       weight_grad_common_factor_median=med(al), weight_grad_rel_l2_worst_beside_common_factor=max(orth.values()),
                       vector_grad_rel_l2_worst=vecs[wv], vector_grad_rel_l2_worst_name=wv, vector_grad_rel_l2_median=med(vecs),
                       grads_compared=len(errs))
            if precision in ("bf16", "fp16"):
                # (i) what 16-bit operand rounding alone costs HERE, forward and backward, no kernel involved
                from oracle import vit_bf16_grad_sim as S
                ekey = "emu" if precision == "bf16" else "emu_fp16"
                if ekey not in cached:
                    rnd = S.ALL_ON if precision == "bf16" else S.FP16
                    cached[ekey] = oracle_run(lambda p: S.vit_classify(p, imgs_c, cfg, rnd))
                ze, le, dze, ge = cached[ekey]
                if light:  # a C5 regime: the emulation's errors on the parameters THIS mode trains
                    ge = {n: g for n, g in ge.items() if n in hip_grads}
                _, m_e, v_e, al_e, orth_e = grad_errors(ge)
                emu = {"logits_max_rel": rel(ze, lr), "loss_rel": rel(le, lo), "weight_grad_rel_l2_worst": max(m_e.values()),
                       "weight_grad_common_factor_median": med(al_e), "weight_grad_rel_l2_worst_beside_common_factor": max(orth_e.values()),
                       "vector_grad_rel_l2_worst": max(v_e.values()),
                       "dlogits_batch_sum_ratio": float(dze[:, 1].double().sum() / dz_ref[:, 1].double().sum())}
                out[f"{precision}_emulation"] = {k: float(f"{v:.3e}") for k, v in emu.items()}
                out[f"logits_vs_{precision}_emulation_max_rel"] = rel(logits.detach(), ze)

                if not light and precision == "bf16":
                    # (ii) PyTorch's own bf16 autocast of the oracle (the reference's AMP path with bf16 in place of fp16)
                    def autocast(p):
                        with torch.autocast("cpu", dtype=torch.bfloat16):
                            return O.vit_classify(p, imgs_c, cfg)
                    za, la, _, ga = oracle_run(autocast)
                    _, m_a, v_a, al_a, _ = grad_errors(ga)
                    out["autocast_yardstick"] = {"logits_max_rel": float(f"{rel(za, lr):.3e}"), "loss_rel": float(f"{rel(la, lo):.3e}"),
                                                 "weight_grad_rel_l2_worst": float(f"{max(m_a.values()):.3e}"),
                                                 "vector_grad_rel_l2_worst": float(f"{max(v_a.values()):.3e}"),
                                                 "weight_grad_common_factor_median": float(f"{med(al_a):.4e}")}
                    # (iii) the same kernels in fp32 mode (exact-f32 MFMA) on the same weights and batch: the north-star tolerance
                    m32 = A.get_MAE_backbone(None, True, 2, False, None, precision="fp32")
                    m32.load_state_dict({k: v for k, v in model.state_dict().items()})
                    m32.to(imgs.device)
                    with torch.no_grad():
                        l32 = m32(imgs)
                    out["fp32_mode_logits_max_rel"] = rel(l32, lr)
                    del m32
                    gates["fp32_mode_logits_max_rel"] = HARD_GATES["fp32_mode_logits_max_rel"]
                if precision == "fp16":
                    gates = dict(FP16_GATES)
                else:
                    gates = {**gates,
                             "logits_max_rel": 1.25 * emu["logits_max_rel"] + 1e-3,
                             "weight_grad_rel_l2_worst": 1.25 * emu["weight_grad_rel_l2_worst"] + 1e-3,
                             "vector_grad_rel_l2_worst": 1.25 * emu["vector_grad_rel_l2_worst"] + 1e-3,
                             "weight_grad_rel_l2_worst_beside_common_factor": 1.25 * emu["weight_grad_rel_l2_worst_beside_common_factor"] + 1e-3}
            else:
                gates = {"logits_max_rel": 1e-3, "loss_rel": 1e-3, "weight_grad_rel_l2_worst": 1e-2, "vector_grad_rel_l2_worst": 1e-2}
            if precision == "fp16":
                out["note"] = ("precision mode fp16 (the reference's AMP arithmetic): gates = SURVEY 8-d as written (loss 1e-3, every gradient "
                               "1e-2 rel-L2) + the fp16 operand-rounding floor for the logits (emulation 1.63e-3 on this init -> 2.0e-3); "
                               "`fp16_emulation` = oracle/vit_bf16_grad_sim.py FP16 on the same tensors, no kernel")
            else:
                out["note"] = ("every gradient of this step is ~ (a direction common to the 64 near-identical noise images) x sum_b dlogit_b, a "
                           "sum that cancels `dlogits_cancellation`-fold: a coherent logit shift of bf16-rounding size moves it by "
                           "(dlogits_batch_sum_ratio - 1) and every gradient with it (weight_grad_common_factor_median); "
                           "`..._beside_common_factor` is the error orthogonal to the oracle's gradient.  `bf16_emulation` = the same "
                               "quantities for oracle/vit_bf16_grad_sim.py (bf16 operand rounding on the CPU, no kernel): the gates are "
                               "1.25 x those + 1e-3; fp32 mode of the same kernels must meet 1e-3.")
        else:
            g = torch.Generator(device=imgs.device).manual_seed(4321)
            noise = torch.rand(imgs.shape[0], 196, device=imgs.device, generator=g)
            with torch.no_grad():
                loss, pred, mask = model(imgs, mask_ratio=0.75, noise=noise)
                lo, pr, mr = O.mae_forward(sd, imgs.cpu(), noise.cpu(), cfg)
            out.update(loss_rel=rel(loss, lo), pred_rel_l2=rel_l2(pred, pr), mask_equal=bool(torch.equal(mask.cpu(), mr)))
            gates = {"loss_rel": HARD_GATES["mae_loss_rel"], "pred_rel_l2": HARD_GATES["mae_pred_rel_l2"]}
            ok["mask_equal"] = out["mask_equal"]
        model.zero_grad(set_to_none=True)
    finally:
        torch.set_num_threads(prev)
    for kname, bound in gates.items():
        ok[kname] = bool(out[kname] <= bound)
    out["gates"] = {k: float(f"{v:.3e}") for k, v in gates.items()}
    out["pass"] = all(ok.values())
    out["failed"] = sorted(k for k, v in ok.items() if not v)
    # the hard gates (exit status): MAE loss / pred, fp32-mode logits
    hard = ["loss_rel", "pred_rel_l2", "mask_equal"] if workload == "mae" else \
        (list(FP16_GATES) if precision == "fp16" else ["fp32_mode_logits_max_rel"])
    out["hard_fail"] = sorted(k for k in hard if k in ok and not ok[k])
    out["seconds"] = round(time.perf_counter() - t0, 1)
    out = {k: (float(f"{v:.3e}") if isinstance(v, float) and k != "seconds" else v) for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# stock PyTorch-ROCm on the same synthetic step (context only)
# ---------------------------------------------------------------------------------------------------------------------
def torch_baseline(device, batch, steps=10, warmup=3):
    """ViT-B/16 classifier in plain torch.nn (same architecture), bf16 autocast, F.scaled_dot_product_attention, fused
    torch.optim.AdamW, BCE-with-logits: what a user gets from the library path on this box.  Never the target."""
    import torch.nn as nn
    import torch.nn.functional as F

    class Blk(nn.Module):
        def __init__(s, D=768, H=12):
            super().__init__()
            s.n1, s.n2 = nn.LayerNorm(D, eps=1e-6), nn.LayerNorm(D, eps=1e-6)
            s.qkv, s.proj, s.fc1, s.fc2, s.H = nn.Linear(D, 3 * D), nn.Linear(D, D), nn.Linear(D, 4 * D), nn.Linear(4 * D, D), H

        def forward(s, x):
            B, N, D = x.shape
            q, k, v = s.qkv(s.n1(x)).reshape(B, N, 3, s.H, D // s.H).permute(2, 0, 3, 1, 4)
            x = x + s.proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, D))
            return x + s.fc2(F.gelu(s.fc1(s.n2(x))))

    class Vit(nn.Module):
        def __init__(s, D=768):
            super().__init__()
            s.pe = nn.Conv2d(3, D, 16, 16)
            s.cls, s.pos = nn.Parameter(torch.zeros(1, 1, D)), nn.Parameter(torch.zeros(1, 197, D))
            s.blocks = nn.Sequential(*[Blk() for _ in range(12)])
            s.norm, s.head = nn.LayerNorm(D, eps=1e-6), nn.Linear(D, 2)

        def forward(s, x):
            x = s.pe(x).flatten(2).transpose(1, 2)
            x = torch.cat((s.cls.expand(x.shape[0], -1, -1), x), 1) + s.pos
            return s.head(s.norm(s.blocks(x))[:, 0])

    torch.manual_seed(0)
    m = Vit().to(device)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05, fused=True)
    imgs, labels = make_batch("cls", batch, device, 0)

    def one():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z = m(imgs)
        loss = F.binary_cross_entropy_with_logits((z[:, 1] - z[:, 0]).float(), labels.float())
        loss.backward()
        opt.step()

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del m, opt
    torch.cuda.empty_cache()
    return {"value": round(batch * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3),
            "what": f"stock PyTorch {torch.__version__} (rocBLAS/hipBLASLt GEMMs, SDPA attention, bf16 autocast, fused AdamW), "
                    f"same ViT-B/16 fine-tune step, bs={batch}, {steps} timed steps; context only, not the target"}


def held_clock():
    """The clock the chip holds under THIS step, from the committed in-kernel measurement (profiles/r4_t1_clock_power.json:
    d(s_memtime) / d(s_memrealtime) stamped inside the GEMM k-loops of the running step -- a diagnostic build, so it cannot be taken
    live here): the roofline's 2.5 PFLOP/s is 256 CUs x 2.4 GHz; at the held clock the same silicon peaks proportionally lower."""
    try:
        with open(os.path.join(REPO, "profiles", "r4_t1_clock_power.json")) as fh:
            d = json.load(fh)
        return {"mhz": d["in_kernel_clock"]["cls"]["ring_gemms"]["clock_mhz"]["median"],
                "source": "profiles/r4_t1_clock_power.json (in-kernel, cls step, ring GEMM k-loops, median over waves)"}
    except (OSError, KeyError, ValueError):
        return None


def measure_sync(ddp, step, device, n=3):
    """What the gradient exchange of a data-parallel rank looks like from inside (bench.py --gpus N, or --force-sync at N = 1):
    bytes and collectives per step from GradSync's launch log, and the EXPOSED wait -- HIP events on the compute stream around the
    first GradSync.wait() of a step (the end-of-backward callback: everything RCCL had not finished under the backward)."""
    sync = ddp.sync
    orig = sync.wait
    spans = []

    def timed_wait():
        if not spans or spans[-1][2]:       # first wait of this step (the optimizer's second call is a no-op wait on done work)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig()
            e1.record()
            spans.append([e0, e1, False])
        else:
            orig()

    sync.wait = timed_wait
    try:
        for _ in range(n):
            step()
            if spans:
                spans[-1][2] = True
        torch.cuda.synchronize(device)
    finally:
        sync.wait = orig
    launched = list(sync.launched)
    return {"collectives_per_step": len(launched), "allreduce_bytes_per_step": int(4 * sum(hi - lo for _, lo, hi in launched)),
            "largest_bucket_bytes": int(4 * max((hi - lo for _, lo, hi in launched), default=0)),
            "exposed_wait_ms": round(sum(e0.elapsed_time(e1) for e0, e1, _ in spans) / max(len(spans), 1), 4),
            "trainable_bytes": int(sync.trainable_bytes())}


def dist_config(world, rank, local, device_name, sync_info, backend):
    """Self-verification of an N > 1 line (main_pretrain.py:201-214: the reference prints world size and per-rank devices at start-up):
    what torch.distributed says the world is, every rank's (rank, LOCAL_RANK, device) gathered to rank 0, and rank 0's view of
    the gradient exchange -- flat scalars / short strings that survive in `config`.  Also the stub's path (BENCH_STUB, CPU test)."""
    mine = (rank, local, device_name)
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
    else:
        gathered = [mine]
    out = {"world_size": dist.get_world_size() if dist.is_initialized() else 1, "backend": backend,
           "ranks_seen": len({g[0] for g in gathered}), "local_ranks": ",".join(str(g[1]) for g in sorted(gathered)),
           "devices": "; ".join(f"{g[0]}:{g[2]}" for g in sorted(gathered)),
           "distinct_local_devices": len({g[1] for g in gathered})}
    if sync_info:
        out.update({f"sync_{k}": v for k, v in sync_info.items()})
    return out


def restore_initial_state(model, opt, init_state, rng_offset, device):
    """Undo the training the pre-heat did (its step count depends on how fast the clocks settle): the initial weights, zero AdamW
    moments and step counters, the initial loss scale, the device generator's offset the MAE masking noise is drawn from.
    Everything in place, so that a captured hipGraph still reads the right buffers."""
    model._rt.wait_updates()
    torch.cuda.synchronize()
    model.load_state_dict(init_state)
    for r in opt._M:
        opt._M[r].zero_()
        opt._V[r].zero_()
    for g in opt.param_groups:
        g.pop("step", None)
    if getattr(opt, "_hyper", None) is not None:  # device records: step counter, bias corrections, scaler flags
        opt._hyper.zero_()
        opt._hyper_host = None  # lr / betas / eps / wd / grad_scale are pushed again at the next step
    scaler = getattr(opt, "loss_scaler", None)
    if scaler is not None and scaler._state is not None:
        scaler._state.zero_()
        scaler._state[0] = scaler.init_scale
    torch.cuda.default_generators[device.index].set_offset(rng_offset)
    model._rt.ensure(device)  # re-cast the bf16 shadow of the restored weights (a graph replay would not)
    torch.cuda.synchronize()


RESETTLE_STEPS = 20    # untimed steps between restore_initial_state() and the W warm-up steps
DUMP_SAMPLE = 1 << 21  # elements per seeded sample of a large output (8 MB in float32)


def _sample(t, seed):
    """All of `t` if it is small, else a fixed, seeded, sorted sample of its flattened elements."""
    t = t.detach()
    if t.numel() <= DUMP_SAMPLE:
        return t.float().cpu().numpy()
    idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(seed)).sort().values
    return t.reshape(-1)[idx.to(t.device)].float().cpu().numpy()


def collect_outputs(model, step, losses):
    """What the last timed step handed its caller: its loss (and the K losses before it), the forward's results, the updated
    parameters and their gradients (both flattened in named_parameters() order and sampled).  float32, < 64 MB in all."""
    model._rt.wait_updates()
    torch.cuda.synchronize()
    out = {"losses": torch.stack(losses).float().reshape(-1).cpu().numpy()}
    out["loss"] = out["losses"][-1:].copy()
    for i, (name, t) in enumerate(sorted(step.outputs.items())):
        out[name] = _sample(t, 100 + i)
    params = [p for _, p in model.named_parameters()]
    out["param_sample"] = _sample(torch.cat([p.detach().float().reshape(-1) for p in params]), 1)
    grads = [p.grad for p in params if p.grad is not None]
    if grads:
        out["grad_sample"] = _sample(torch.cat([g.float().reshape(-1) for g in grads]), 2)
    return out


def write_outputs(path, arrays):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------
def run_workload(args, workload, batch, device, world, rank, headline, finetune_mode="full", light=False, precision=None,
                 kstats=True, eval_forward=None, factory=None):
    """Build, warm up, time exactly args.steps steps (barrier + synchronize on both sides, max over ranks).
    factory: an MAE factory other than the base one (no parity block: the cached oracle run is ViT-B's; parity of the larger
    factories is tests/test_gpu_parity_large.py's, against fixtures made by the reference).
    light: a C5 sub-record -- no kernel statistics, parity against the cached oracle run of the headline, + eval forward.
    precision: this record's precision mode (default: --precision); kstats: per-kernel HIP-event statistics."""
    args = argparse.Namespace(**{**vars(args), "precision": precision or args.precision})
    if factory:
        args = argparse.Namespace(**{**vars(args), "no_parity": True})
        kstats = False
    model, ddp, opt = build(workload, args.precision, device, world, batch, finetune_mode, force_sync=args.force_sync and world == 1,
                            factory=factory)
    imgs, labels = make_batch(workload, batch, device, rank, pool=not args.single_batch)
    pooled = isinstance(imgs, list)
    imgs0, labels0 = (imgs[0], labels[0]) if pooled else (imgs, labels)   # the batch of the parity block / the eval forward
    # the state the first step starts from (the parity block compares there; the pre-heat's training is undone to it)
    init_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rng_offset = torch.cuda.default_generators[device.index].get_offset()
    use_graph = args.graph == "on"  # auto: eager (measured faster: graph replay serialises the wgrad side stream)
    if use_graph:
        # a captured step reads fixed addresses: ONE static batch / label / noise buffer, refilled from the resident pool before every
        # replay (what a training loop over a graphed step does with each loader batch) -- the draws stay outside the graph
        from ssl4polyp_amd.graph import GraphedStep
        s_imgs, s_labels = imgs0.clone(), labels0.clone()
        noise_buf = torch.rand(batch, 196, device=device) if workload == "mae" else None
        eager_step = make_step(workload, ddp, opt, s_imgs, s_labels, args.lr_every_step, noise_buf=noise_buf)
        graphed = GraphedStep(eager_step, opt, warmup=3)  # capture failures are fatal: no silent eager fallback
        tick = [0]

        def step():
            i = tick[0]
            tick[0] = i + 1
            if pooled:
                s_imgs.copy_(imgs[i % len(imgs)])
                s_labels.copy_(labels[i % labels.shape[0]])
            if noise_buf is not None:
                noise_buf.copy_(model._draw_noise(batch, device))
            return graphed.replay()
    else:
        eager_step = make_step(workload, ddp, opt, imgs, labels, args.lr_every_step)
        step = eager_step

    host_pool, host_gen = [], torch.Generator().manual_seed(1234 + rank)
    host_input = args.input == "host" and headline
    if host_input:  # four decoded batches in pinned host memory, built outside the timed region
        hw = (576, 720) if args.augment == "device" else (224, 224)   # decoded Hyperkvasir-like frames / already resized frames
        host_pool = [(torch.randint(0, 256, (batch, *hw, 3), dtype=torch.uint8, generator=host_gen).pin_memory(),
                      (torch.rand(batch, generator=host_gen) < 0.5).long().pin_memory()) for _ in range(4)]

    def host_feed(n):
        # uint8 HWC frames + labels in pinned host memory -> DevicePrefetcher (H2D + flips + ToTensor + Normalize)
        from ssl4polyp_amd.data import DeviceAugmenter, DevicePrefetcher
        aug = DeviceAugmenter(device) if args.augment == "device" else None
        return DevicePrefetcher([host_pool[i % 4] for i in range(n)], device, flip_p=0.5, generator=host_gen, augment=aug)

    # The parity block compares at the freshly initialised weights (after tens of AdamW steps at lr 1e-3 on random labels
    # the outputs and gradients collapse towards zero and relative errors stop meaning anything), but runs AFTER the timed
    # region on a restored copy of them: its ~10 s of CPU oracle leave the GPU idle, and a timed loop that starts right
    # after an idle phase measures the clock ramp (first steps up to 1.5x slower) instead of the steady state.
    want_parity = rank == 0 and world == 1 and not args.no_parity and args.full
    if light or not kstats or not args.full:
        args = argparse.Namespace(**{**vars(args), "no_kernel_stats": True})
    # Pre-heat: untimed steps of the same step function until args.preheat seconds have passed, so that clocks and power
    # management have settled before the W warm-up steps (a process that starts timing ~0.15 s after its first launch is
    # still on the ramp: scratch/host_time.py shows 16 ms steps for the first ~15 steps, 10.8 ms afterwards).
    preheat_steps = 0
    if args.preheat > 0 and not host_input:
        t_ph = time.perf_counter()
        while True:
            for _ in range(5):
                step()
            preheat_steps += 5
            torch.cuda.synchronize()
            el = time.perf_counter() - t_ph
            if world > 1:  # every rank must leave the loop after the same number of steps (they contain all-reduces)
                t = torch.tensor([el], device=device, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = t.item()
            if el >= args.preheat:
                break
        restore_initial_state(model, opt, init_state, rng_offset, device)
        eager_step.rewind()
        if use_graph:
            tick[0] = 0
        # a fixed number of steps from the restored state: the step rate needs them to settle again after the restore's pause
        # (with the W warm-up steps alone right behind it, the timed steps ran 0.35 % slower)
        for _ in range(RESETTLE_STEPS):
            step()
        preheat_steps += RESETTLE_STEPS
    if host_input:
        if use_graph:
            sys.exit("--input host feeds a new batch every step: use eager launch")
        for im, lb in host_feed(args.warmup):
            step(im, lb)
    else:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    # host cost of enqueueing a step, measured on an empty queue (inside the timed loop the host runs ahead until the
    # HIP queue is full and is then throttled to the device's pace, so the loop's own enqueue time says nothing)
    t_enq = float("nan") if args.full else None  # (--full: the host's enqueue time of one step)
    if not host_input and args.full:
        t_h = time.perf_counter()
        for _ in range(3):
            step()
        t_enq = (time.perf_counter() - t_h) / 3
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # one event per step boundary on the step's own stream: the spread of the per-step times (DVFS ramps, a schedule that
    # settles into a slower phase) is reported beside the mean the metric is computed from
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    losses = []
    scaler = getattr(opt, "loss_scaler", None)
    skipped0 = scaler.counters()["skipped"] if scaler is not None else 0
    t0 = time.perf_counter()
    t0_unix = time.time()
    marks[0].record()
    if host_input:
        for i, (im, lb) in enumerate(host_feed(args.steps)):
            loss = step(im, lb)
            losses.append(loss.detach())
            marks[i + 1].record()
    else:
        for i in range(args.steps):
            loss = step()
            losses.append(loss.detach())
            marks[i + 1].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t1_unix = time.time()
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if headline and rank == 0 and args.dump_outputs:  # before anything else runs a step on this model
        write_outputs(args.dump_outputs, collect_outputs(model, eager_step, losses))
    busy = None
    if args.host_busy > 0 and headline and not host_input:
        # N spinners pinned to nothing in particular: the scheduler shares the granted cores between them and this process
        spin = [subprocess.Popen([sys.executable, "-c", "while True: pass"]) for _ in range(args.host_busy)]
        try:
            time.sleep(0.5)
            torch.cuda.synchronize()
            t_h = time.perf_counter()
            for _ in range(3):
                step()
            enq_b = (time.perf_counter() - t_h) / 3
            torch.cuda.synchronize()
            t_b = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            dt_b = time.perf_counter() - t_b
            busy = {"spinning_processes": args.host_busy, "host_cpus": len(os.sched_getaffinity(0)),
                    "host_enqueue_ms_per_step": round(enq_b * 1e3, 3), "value": round(batch * world * args.steps / dt_b, 2),
                    "ms_per_step": round(dt_b / args.steps * 1e3, 3)}
        finally:
            for p in spin:   # exactly the PIDs started here
                p.kill()
            for p in spin:
                p.wait()
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    step_ms = {"min": round(per_step[0], 3), "median": round(per_step[len(per_step) // 2], 3), "max": round(per_step[-1], 3),
               "first": round(marks[0].elapsed_time(marks[1]), 3), "last": round(marks[-2].elapsed_time(marks[-1]), 3)}
    loss_val = float(loss.detach())
    if not (loss_val == loss_val):
        sys.exit(f"non-finite loss in the timed region ({workload}, finetune mode {finetune_mode}, step loss {loss_val})")
    lv = torch.stack(losses).float().cpu()
    loss_mean, loss_min = float(lv.mean()), float(lv.min())
    # a live problem: rounds 1-3 timed a memorised batch (cls loss 1e-5, frozen-backbone regimes 0.0 = all-zero dlogits, i.e. backward
    # GEMMs on zeros, which hold a higher clock: MI355X_MICROARCH.md DVFS give-back).  A cls record whose loss collapsed is not a
    # measurement of the training step and is marked as such (the headline fails the run)
    degenerate = workload == "cls" and loss_min <= 1e-3
    if degenerate and headline and not args.single_batch:
        sys.exit(f"degenerate workload: the cls loss fell to {loss_min:.2e} inside the timed region (memorised batch)")
    scale_info = None
    if scaler is not None:
        c = scaler.counters()
        scale_info = {"loss_scale": scaler.get_scale(), "skipped_steps_in_timed_region": c["skipped"] - skipped0,
                      "skipped_steps_total": c["skipped"], "optimizer_steps_total": c["steps"]}
    sync_info = measure_sync(ddp, eager_step, device) if ddp.sync is not None and args.full else None
    rec = None
    stats = None
    parity = None
    if not args.no_kernel_stats:
        # EVERY rank runs the instrumented steps (they contain the gradient all-reduces: a rank that skipped them would
        # leave the others waiting in RCCL); only rank 0 reports
        stats = kernel_stats(model, eager_step)
    if want_parity:
        model._rt.wait_updates()
        torch.cuda.synchronize()
        model.load_state_dict(init_state)  # back to the initial weights (the optimizer state is not used by the comparison)
        parity = parity_block(workload, model, imgs0, labels0, args.precision, light=light)
    eval_rec = None
    if light if eval_forward is None else eval_forward:
        # evaluation forward (tc.py:4652-4812 / f3): eval mode, no autograd, forward-only workspace, same resident batch
        model.eval()
        with torch.no_grad():
            for _ in range(5):
                ddp(imgs0)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            te = time.perf_counter()
            for j in range(args.steps):
                ddp(imgs[j % len(imgs)] if pooled else imgs0)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            de = time.perf_counter() - te
        if world > 1:
            t = torch.tensor([de], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            de = t.item()
        ev_ips = batch * world * args.steps / de
        eval_rec = {"value": round(ev_ips, 1), "unit": "images/sec", "ms_per_batch": round(de / args.steps * 1e3, 3),
                    "roofline_frac": round(ev_ips / world * FWD_GFLOP_PER_IMG / 1e3 / PEAK_TFLOPS[args.precision], 4)}
        model.train()
    if rank == 0:
        ips = batch * world * args.steps / dt
        gflop = FINETUNE_GFLOP[finetune_mode] if workload == "cls" else \
            (round(mae_gflop_per_img(model), 2) if factory else GFLOP_PER_IMG[workload])
        per_gpu_tflops = ips / world * gflop / 1e3
        peak = PEAK_TFLOPS[args.precision]
        roof = {"bound": "mfma", "achieved": round(per_gpu_tflops, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(per_gpu_tflops / peak, 4), "traffic": None, "gflop_per_img": gflop,
                "basis": f"{gflop} algorithmic GFLOP/img/step x img/s/GPU (BASELINE.md §3)"}
        if stats is not None:
            ks, hb, at, gt = stats
            dom = max(ks.items(), key=lambda kv: kv[1]["launches"] * kv[1]["avg_us"])  # largest share of GPU time, as rocprof ranks
            names = {"nt_store": "gemm_v3_kernel (forward, act-typed output: qkv, decoder_pred ...)",
                     "nt_gelu": "gemm_v3_kernel (forward fc1 + GELU)", "nt_residual": "gemm_v3_kernel (forward, f32 residual epilogue: proj / fc2)",
                     "nn_store": "gemm_v3_kernel (dgrad: dY [M,K] x W [K,N])", "nn_dgelu": "gemm_v3_kernel (dgrad fc2 + dGELU)",
                     "tnn": "gemm_v3_kernel (split-K weight gradient)", "wgrad_group": "wgrad_group_kernel (the dW of a block in two launches, full-K tiles)"}
            roof["kernel"] = {"name": names.get(dom[0], dom[0]), "class": dom[0], **dom[1],
                              "frac": round(dom[1]["tflops"] / peak, 4),
                              **({"frac_on_held_cus": round(dom[1]["tflops_on_held_cus_x256"] / peak, 4)}
                                 if "tflops_on_held_cus_x256" in dom[1] else {}),
                              "share_of_gemm_time": round(dom[1]["launches"] * dom[1]["avg_us"] * 1e-6 / max(gt, 1e-12), 3),
                              "note": "the class with the largest summed in-step launch time (HIP events on its own stream); "
                                      "launches of the forward chains / of the dgrad and weight-gradient streams overlap, so "
                                      "each shares the CUs (the grouped weight gradients take 72 + 36 of the 256 CUs by design, as two "
                                      "launches side by side: `frac` prices a launch against the whole chip, `frac_on_held_cus` against "
                                      "the CUs it holds; stand-alone rates: DESIGN.md)"}
            try:  # PMC traffic of the dominant kernel, from the committed rocprofv3 --pmc passes (profiles/)
                with open(os.path.join(REPO, "profiles", "pmc_traffic.json")) as fh:
                    t = json.load(fh).get(workload, {}).get(dom[0])
                if t and args.precision == "bf16" and batch == (64 if workload == "cls" else 256):
                    roof["traffic"] = {"MB_per_launch": t["MB_per_launch"], "algorithmic_MB_per_launch": t["algorithmic_MB_per_launch"],
                                       "source": t["source"],
                                       "measured": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench (committed under "
                                                   "profiles/; PMC counters cannot be read from inside the process)"}
            except (OSError, ValueError):
                pass
            roof["gemm_by_layout"] = ks
            roof["attention"] = at          # algorithmic 4 (fwd) / 10 (bwd) N^2 dh FLOP per head over the launch time
            roof["hbm_kernels"] = hb        # in-step (beside the weight-gradient stream), algorithmic bytes / time
            roof["gemm_share_of_step"] = round(gt / (dt / args.steps), 3)
        rec = {"value": round(ips, 2), "unit": "images/sec", "ms_per_step": round(dt / args.steps * 1e3, 3),
               "host_enqueue_ms_per_step": round(t_enq * 1e3, 3) if t_enq is not None else None, "step_ms": step_ms,
               "preheat_steps": preheat_steps,
               "timed_region_unix": [round(t0_unix, 3), round(t1_unix, 3)],  # (for scratch/telemetry.py traces)
               "config": {"workload": WORKLOAD_NAME[workload] + f", bs={batch}/GPU, 224^2, AdamW, random init"
                                      + (f", finetune mode {finetune_mode} (finetune.py:49-91)" if workload == "cls" else ""),
                          "global_batch": batch * world, "parallelism": f"dp{world}" + ("+forced world-1 RCCL all-reduces" if ddp.sync is not None and world == 1 else ""),
                          "final_loss": round(loss_val, 5), "mean_loss": round(loss_mean, 5), "min_loss": round(loss_min, 5),
                          "batches": (f"{N_IMG_BATCHES} resident image batches x {N_LABEL_SETS} Bernoulli(0.5) label vectors, a new pairing "
                                      "every step" if pooled else "ONE resident batch (memorised: --single-batch A/B)"),
                          "launch": "hipGraph replay" if use_graph else "eager",
                          "lr_schedule": ("per-iteration warm-up (engine_pretrain.py:47-48; 40 epochs x 390 it)" if workload == "mae"
                                          else "new lr every step" if args.lr_every_step else "constant")},
               "roofline": roof}
        if degenerate:
            rec["degenerate"] = f"cls loss fell to {loss_min:.2e} in the timed region: not a measurement of the training step"
        if scale_info is not None:
            rec["loss_scaling"] = scale_info
        if sync_info is not None:
            rec["grad_sync"] = sync_info
        if parity is not None:
            rec["parity"] = parity
        if busy is not None:
            rec["busy_host"] = busy
        if eval_rec is not None:
            rec["eval_forward"] = eval_rec
        if light:  # trainable bytes the gradient all-reduce would carry in this mode (parallel.GradSync plan)
            rec["trainable_params"] = int(sum(p.numel() for p in model.parameters() if p.requires_grad))
    del model, ddp, opt, eager_step, step
    torch.cuda.empty_cache()
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# `python bench.py --gpus N` without a launcher: the parent starts the N ranks itself
# ---------------------------------------------------------------------------------------------------------------------
def self_launch(n: int) -> int:
    """The reference spawns its own ranks (train_classification.py:8152-8169: mp.spawn(train, nprocs=world_size)); so does
    the bench when it is called as plain `python bench.py --gpus N` (no WORLD_SIZE in the environment).  The parent never
    touches the GPU: it starts N fresh interpreters of this very command line with RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR / MASTER_PORT set (one rank per GPU, torchrun's environment contract), relays rank 0's JSON line, and returns
    non-zero if any rank fails.  A rank that dies must not leave the others parked inside an RCCL collective: the first
    non-zero exit (or the overall time limit, BENCH_LAUNCH_TIMEOUT seconds, default 3000) ends every remaining rank --
    SIGTERM to exactly the process groups started here, SIGKILL after a 10 s grace."""
    import signal
    import socket
    import tempfile
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    base = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(n))
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL needs it)
    limit = float(os.environ.get("BENCH_LAUNCH_TIMEOUT", "3000"))
    out0 = tempfile.TemporaryFile(mode="w+")
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL, start_new_session=True))

    def end_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)  # each rank leads its own session: the group is exactly what was started here
                except (ProcessLookupError, PermissionError):
                    pass

    t0 = time.monotonic()
    rc = 0
    why = ""
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                rc = bad[0][1] if bad[0][1] > 0 else 1
                why = f"rank {bad[0][0]} exited with status {bad[0][1]}"
                break
            if all(c == 0 for c in codes):
                break
            if time.monotonic() - t0 > limit:
                rc, why = 124, f"time limit of {limit:.0f} s (BENCH_LAUNCH_TIMEOUT)"
                break
            time.sleep(0.1)
    except KeyboardInterrupt:
        rc, why = 130, "interrupted"
    if rc:
        print(f"[bench] {why}: ending the other ranks", file=sys.stderr, flush=True)
        end_all(signal.SIGTERM)
        t1 = time.monotonic()
        while any(p.poll() is None for p in procs) and time.monotonic() - t1 < 10:
            time.sleep(0.1)
        end_all(signal.SIGKILL)
        for p in procs:
            p.wait()
        return rc
    # stdout of the job = rank 0's ONE JSON line; whatever else a library printed on rank 0's stdout (gloo / RCCL banners)
    # goes to stderr
    out0.seek(0)
    lines = [ln for ln in out0.read().splitlines() if ln.strip()]
    js = [i for i, ln in enumerate(lines) if ln.lstrip().startswith("{") and ln.rstrip().endswith("}")]
    for i, ln in enumerate(lines):
        if not js or i != js[-1]:
            print(ln, file=sys.stderr)
    if not js:
        print("[bench] rank 0 printed no JSON line", file=sys.stderr)
        return 1
    print(lines[js[-1]], flush=True)
    return 0


def run_stub(args, world, rank):
    """BENCH_STUB=1 (tests/test_bench_launch_cpu.py; no GPU in the build container): the launch, rendezvous, barrier /
    max-over-ranks timing and rank-0 JSON path of this file with gloo on the CPU and a stand-in step (a small all-reduce).
    Never a measurement: the line says so in `data`."""
    if os.environ.get("BENCH_STUB_FAIL_RANK") == str(rank):
        sys.exit(3)  # a rank that dies before the rendezvous: the launcher must end the others and report failure
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1:
        dist.init_process_group("gloo")
    if os.environ.get("BENCH_STUB_NOISE") == "1":  # a library banner on file descriptor 1 (what RCCL does at communicator start-up)
        os.write(1, b"RCCL version : stub banner on fd 1\nHostname     : stub\n")
    x = torch.ones(1 << 12)

    def step():
        y = x * (rank + 1)
        if world > 1:
            dist.all_reduce(y)
        return y

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = step()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    # the self-verification keys of an N > 1 line, through the same dist_config() the GPU path uses
    tw = time.perf_counter()
    step()
    sync_info = {"collectives_per_step": 1 if world > 1 else 0, "allreduce_bytes_per_step": 4 * x.numel() if world > 1 else 0,
                 "largest_bucket_bytes": 4 * x.numel() if world > 1 else 0,
                 "exposed_wait_ms": round((time.perf_counter() - tw) * 1e3, 4), "trainable_bytes": 4 * x.numel()}
    dcfg = dist_config(world, rank, int(os.environ.get("LOCAL_RANK", "0")), "cpu", sync_info if rank == 0 else None,
                       "gloo" if world > 1 else "none")
    if rank == 0:
        emit(json.dumps({"metric": "stub", "value": round(64 * world * args.steps / dt, 2), "unit": "images/sec", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "stub step on the CPU (launch-path test, not a measurement)",
                          "config": {"workload": "stub", "global_batch": 64 * world, "parallelism": f"dp{world}",
                                     "allreduce_check": float(y[0]), **dcfg}}))
    if world > 1:
        dist.destroy_process_group()


_REAL_STDOUT = None


def claim_stdout():
    """The contract is ONE JSON line on stdout.  Libraries write there too -- RCCL prints a five-line version banner on fd 1 when its
    first communicator comes up (seen under --force-sync: "RCCL version : ... Librccl path : ..."), gloo and the HIP runtime have their
    own -- so from here on file descriptor 1 IS stderr for everything in this process, and only emit() writes to the real stdout."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(line: str):
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, (line + "\n").encode())


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus))  # before anything touches the GPU in this process
    claim_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or unset WORLD_SIZE and let "
                 "bench.py start the ranks itself)")
    if os.environ.get("BENCH_STUB") == "1":
        return run_stub(args, world, rank)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X (no CPU fallback for the product path)")
    # rehearsal hook (one-GPU box): BENCH_REHEARSAL=1 puts every rank on cuda:0 and uses gloo, so the N>1 code path
    # (rendezvous, broadcast, bucketed overlap, max-over-ranks timing) can be exercised without N GPUs
    rehearsal = os.environ.get("BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import ssl4polyp_amd
    if os.environ.get("BENCH_LATE_STREAMS") != "1":  # (A/B switch of scratch/archive_r3/r3_exp20.sh)
        ssl4polyp_amd.reserve_streams(device)  # before RCCL creates its streams: one hardware queue per engine stream
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    elif args.force_sync:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=device)
    batch = args.batch or (64 if args.workload == "cls" else 256)
    head = run_workload(args, args.workload, batch, device, world, rank, True, finetune_mode=args.finetune_mode)
    # --full: the sub-records beside the headline (a plain run is the headline alone)
    default_line = args.full and args.workload == "cls" and not args.batch and args.input == "resident" and args.precision == "bf16"
    subs = {}
    if default_line and not args.no_fp16:
        # the same fine-tune step in precision mode fp16: the 16-bit mode whose parity gate is SURVEY 8-d as written
        subs["cls_fp16"] = run_workload(args, "cls", batch, device, world, rank, False, precision="fp16", kstats=False)
    if default_line and not args.no_fp32:
        # the mode that meets the north-star's 1e-3 on the LOGITS too (exact-f32 MFMA, 1/16 of the 16-bit rate): a short record, so that
        # the line carries a throughput for every parity level -- fp32 (logits 5e-6), fp16 (SURVEY 8-d as written; logits at the fp16
        # operand-rounding floor), bf16 (headline)
        a32 = argparse.Namespace(**{**vars(args), "steps": min(args.steps, 10), "warmup": min(args.warmup, 2), "preheat": 0.3,
                                    "no_parity": True})
        subs["cls_fp32"] = run_workload(a32, "cls", batch, device, world, rank, False, precision="fp32", kstats=False)
    if default_line and not args.no_mae:
        # BASELINE.json metric: "(MAE pretrain + cls finetune)" at bs=64/GPU; configs[2] / [3] run MAE at 256/GPU: both, same protocol
        subs["mae_bs256"] = run_workload(args, "mae", 256, device, world, rank, False)
        subs["mae_bs64"] = run_workload(args, "mae", 64, device, world, rank, False, kstats=False)
        if not args.no_fp16:
            subs["mae_bs256_fp16"] = run_workload(args, "mae", 256, device, world, rank, False, precision="fp16", kstats=False)
        if not args.no_vith:
            # the largest factory of the row-#1 file (models_mae.py:239-244: ViT-H/14, 632 M parameters) at the metric's batch: a short
            # record (its steps are ~10x a ViT-B step's)
            ah = argparse.Namespace(**{**vars(args), "steps": min(args.steps, 12), "warmup": min(args.warmup, 3), "preheat": 0.5})
            subs["mae_vith14_bs64"] = run_workload(ah, "mae", 64, device, world, rank, False, kstats=False, factory="mae_vit_huge_patch14")
    c5 = None
    if default_line and args.finetune_mode == "full" and not args.no_c5 and args.graph != "on":
        # configs[4] (C5): the staged fine-tune regimes of finetune.py:49-91 on the same synthetic step, + the eval forward
        c5 = {m: run_workload(args, "cls", batch, device, world, rank, False, finetune_mode=m, light=True)
              for m in ("none", "head+1", "head+2")}

    if rank == 0:
        cfg = dict(head["config"])
        roof = dict(head["roofline"])
        # ---- flat scalars: the driver's record keeps the scalar members of `config`, `roofline` and `cpu_baseline` only ----
        kern = roof.get("kernel")
        if kern:
            roof.update(kernel_name=kern["name"], kernel_class=kern["class"], kernel_launches_per_step=kern["launches"],
                        kernel_avg_us=kern["avg_us"], kernel_tflops=kern["tflops"], kernel_frac=kern["frac"],
                        kernel_share_of_gemm_time=kern["share_of_gemm_time"])
            if "frac_on_held_cus" in kern:
                roof.update(kernel_frac_on_held_cus=kern["frac_on_held_cus"], kernel_avg_cus_held=kern.get("avg_cus_held"))
        traffic = roof.get("traffic")
        if isinstance(traffic, dict):
            roof["traffic_detail"] = traffic
            roof["traffic"] = round(traffic["MB_per_launch"] * 1e6)           # HBM bytes per launch of the dominant kernel (PMC)
            roof["traffic_algorithmic_bytes"] = round(traffic["algorithmic_MB_per_launch"] * 1e6)
            roof["traffic_ratio"] = round(traffic["MB_per_launch"] / traffic["algorithmic_MB_per_launch"], 3)
            roof["traffic_source"] = traffic["source"]
        clk = held_clock()
        if clk:
            roof.update(held_clock_mhz=clk["mhz"], frac_of_peak_at_held_clock=round(roof["frac"] * 2400.0 / clk["mhz"], 4),
                        held_clock_source=clk["source"])
        if head.get("parity"):
            par = head["parity"]
            cfg.update(parity_pass=par["pass"], parity_logits_max_rel=par.get("logits_max_rel"), parity_loss_rel=par.get("loss_rel"),
                       parity_weight_grad_rel_l2_worst=par.get("weight_grad_rel_l2_worst"),
                       parity_fp32_mode_logits_max_rel=par.get("fp32_mode_logits_max_rel"))

        def flat(prefix, r, parity_keys=()):
            if r is None:
                return
            cfg[f"{prefix}_img_s"] = r["value"] if "degenerate" not in r else None
            cfg[f"{prefix}_ms_per_step"] = r["ms_per_step"]
            cfg[f"{prefix}_roofline_frac"] = r["roofline"]["frac"]
            cfg[f"{prefix}_final_loss"] = r["config"]["final_loss"]
            if "degenerate" in r:
                cfg[f"{prefix}_degenerate"] = r["degenerate"]
            if "loss_scaling" in r:
                cfg[f"{prefix}_loss_scale"] = r["loss_scaling"]["loss_scale"]
                cfg[f"{prefix}_skipped_steps_in_timed_region"] = r["loss_scaling"]["skipped_steps_in_timed_region"]
            if r.get("parity"):
                cfg[f"{prefix}_parity_pass"] = r["parity"]["pass"]
                for k in parity_keys:
                    if k in r["parity"]:
                        cfg[f"{prefix}_parity_{k}"] = r["parity"][k]
            if "eval_forward" in r:
                cfg[f"{prefix}_eval_img_s"] = r["eval_forward"]["value"]

        flat("cls_fp16", subs.get("cls_fp16"), ("logits_max_rel", "loss_rel", "weight_grad_rel_l2_worst", "vector_grad_rel_l2_worst"))
        if subs.get("cls_fp16") and subs["cls_fp16"].get("parity"):
            cfg["cls_fp16_parity_gates"] = "logits <= 2.0e-3 (fp16 operand-rounding floor 1.63e-3 + 25 %), loss <= 1e-3, every gradient <= 1e-2 rel-L2 (SURVEY 8-d)"
        flat("cls_fp32", subs.get("cls_fp32"))
        if subs.get("cls_fp32") and head.get("parity"):
            cfg["cls_fp32_parity_logits_max_rel"] = head["parity"].get("fp32_mode_logits_max_rel")   # (measured in the headline's parity block)
        flat("mae_bs256", subs.get("mae_bs256"), ("loss_rel", "pred_rel_l2"))
        flat("mae_bs64", subs.get("mae_bs64"), ("loss_rel", "pred_rel_l2"))
        flat("mae_bs256_fp16", subs.get("mae_bs256_fp16"), ("loss_rel", "pred_rel_l2"))
        flat("mae_vith14_bs64", subs.get("mae_vith14_bs64"))
        if subs.get("mae_vith14_bs64"):
            cfg["mae_vith14_bs64_gflop_per_img"] = subs["mae_vith14_bs64"]["roofline"].get("gflop_per_img")
        for m, r in (c5 or {}).items():
            flat("finetune_" + m.replace("+", "_plus_"), r, ("logits_max_rel",))
        if head.get("grad_sync") or world > 1:
            cfg.update(dist_config(world, rank, int(os.environ.get("LOCAL_RANK", "0")), torch.cuda.get_device_name(device),
                                   head.get("grad_sync"), dist.get_backend() if dist.is_initialized() else "none"))
        out = {
            "metric": "training-step images/sec/node, ViT-B/16 224^2 (" + ("cls fine-tune" if args.workload == "cls" else "MAE pre-train") + ")",
            "value": head["value"], "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.precision,
            "data": "synthetic" if args.input == "resident" else
                    ("synthetic uint8 frames in pinned host memory (PCIe-inclusive)" +
                     (", 576x720, whole train transform on the device" if args.augment == "device" else "")),
            "config": cfg, "host_enqueue_ms_per_step": head["host_enqueue_ms_per_step"], "step_ms": head["step_ms"],
            "preheat_steps": head["preheat_steps"], "timed_region_unix": head["timed_region_unix"],
            "roofline": roof,
        }
        for k in ("parity", "busy_host", "loss_scaling", "grad_sync"):
            if k in head:
                out[k] = head[k]
        for name, r in subs.items():
            out[name] = {"steps": args.steps if name != "cls_fp32" else min(args.steps, 10), "warmup": args.warmup, **r}
        if "mae_bs256" in subs:
            out["mae"] = out["mae_bs256"]   # (the name rounds 1-3 used)
        if c5 is not None:
            out["finetune_modes"] = {m: {k: v for k, v in r.items() if k not in ("host_enqueue_ms_per_step", "preheat_steps")}
                                     for m, r in c5.items()}
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.workload, args.cpu_full)
        if world == 1 and args.full and not args.no_torch_baseline and args.precision == "bf16":
            try:
                out["torch_baseline"] = torch_baseline(device, 64)
            except Exception as e:  # context only: never fail the bench line over it
                out["torch_baseline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        emit(json.dumps(out))
        recs = [("cls", out.get("parity"))] + [(n, r.get("parity")) for n, r in subs.items()]
        hard = [f"{name}: {k}" for name, rec in recs if rec for k in rec.get("hard_fail", [])]
        if hard:
            print("[bench] PARITY GATE FAILED: " + ", ".join(hard), file=sys.stderr, flush=True)
            if dist.is_initialized():
                dist.destroy_process_group()
            sys.exit(4)
    elif world > 1:
        dist_config(world, rank, int(os.environ.get("LOCAL_RANK", "0")), torch.cuda.get_device_name(device), None,
                    dist.get_backend())  # (this rank's part of the all_gather_object behind rank 0's line)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
