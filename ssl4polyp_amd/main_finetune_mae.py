"""End-to-end fine-tuning of a pre-trained MAE encoder on the MI355X engine -- the flag surface and behaviour of the reference's
src/ssl4polyp/models/mae/main_finetune.py + engine_finetune.py + util/lr_decay.py: the whole ViT of models_vit trains (global_pool by
default) under AdamW with layer-wise lr decay, lr = blr * batch_size * accum_iter / 256 (:289-292), per-iteration half-cosine schedule
with warm-up, Mixup / CutMix with SoftTargetCrossEntropy (or label smoothing, or plain cross-entropy), gradient clipping, acc@1 / acc@5
on DATA/val after every epoch, checkpoint-<epoch>.pth in the dict main_pretrain writes, one JSON line per epoch in log.txt.
(main_finetune.py of THIS package is the pack fine-tuning of the classification trainer; this is the MAE recipe.)

    python -m ssl4polyp_amd.main_finetune_mae --finetune ckpts/checkpoint-399.pth --data_path /data/imagenet --nb_classes 1000 \
        --model vit_base_patch16 --batch_size 64 --mixup 0.8 --cutmix 1.0 --smoothing 0.1 --layer_decay 0.65
    python -m ssl4polyp_amd.main_finetune_mae --resume out/ckpts/checkpoint-49.pth --eval --data_path ...

The input pipeline is main_linprobe's: the device crop of mae/util/crop.py, flip, normalise for training; Resize(256) + CenterCrop in
the workers for validation.  The crops, flips, the sampler's order and the mixing draws of epoch e depend on (seed, e) alone, so a
resumed run continues as the uninterrupted one.  The head, the pool and the loss run in f32 in every --precision.

NOT BUILT -- accepted as flags at their "off" value only, refused otherwise:
  --drop_path > 0      stochastic depth needs a per-row scale in the residual GEMM epilogues.  THE DEFAULT HERE IS 0.0; THE REFERENCE'S
                       IS 0.1: results of the reference's default recipe are not reproduced until that exists.
  --aa, --reprob, --color_jitter   timm's create_transform (RandAugment, random erasing, colour jitter).
  --dist_eval and more than one process;  --input_size other than the model's (position-embedding interpolation)."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from . import models_vit
from .lr_decay import param_groups_lrd
from .main_linprobe import _ValFrames, _val_collate
from .mixup import Mixup
from .optim import FusedAdamW, LossScaler
from .train import evaluate_probe, finetune_one_epoch, load_mae_checkpoint, save_mae_checkpoint


def get_args_parser():
    p = argparse.ArgumentParser("MAE fine-tuning for image classification (MI355X)", add_help=True)
    p.add_argument("--batch_size", default=64, type=int, help="batch size per GPU")
    p.add_argument("--epochs", default=50, type=int)
    p.add_argument("--accum_iter", "--acum_iter", dest="accum_iter", default=1, type=int)
    p.add_argument("--model", default="vit_large_patch16", type=str)
    p.add_argument("--input_size", default=224, type=int)
    p.add_argument("--drop_path", type=float, default=0.0, help="NOT BUILT: only 0.0 is accepted (the reference's default is 0.1)")
    p.add_argument("--clip_grad", type=float, default=None)
    p.add_argument("--weight_decay", type=float, default=0.05)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--blr", type=float, default=1e-3)
    p.add_argument("--layer_decay", type=float, default=0.75)
    p.add_argument("--min_lr", type=float, default=1e-6)
    p.add_argument("--warmup_epochs", type=int, default=5)
    p.add_argument("--color_jitter", type=float, default=None, help="NOT BUILT: only None is accepted")
    p.add_argument("--aa", type=str, default=None, help="NOT BUILT: only None is accepted (the reference's default is rand-m9-mstd0.5-inc1)")
    p.add_argument("--smoothing", type=float, default=0.1)
    p.add_argument("--reprob", type=float, default=0.0, help="NOT BUILT: only 0 is accepted (the reference's default is 0.25)")
    p.add_argument("--remode", type=str, default="pixel")
    p.add_argument("--recount", type=int, default=1)
    p.add_argument("--resplit", action="store_true", default=False)
    p.add_argument("--mixup", type=float, default=0.0)
    p.add_argument("--cutmix", type=float, default=0.0)
    p.add_argument("--cutmix_minmax", type=float, nargs="+", default=None)
    p.add_argument("--mixup_prob", type=float, default=1.0)
    p.add_argument("--mixup_switch_prob", type=float, default=0.5)
    p.add_argument("--mixup_mode", type=str, default="batch")
    p.add_argument("--finetune", default="", help="pre-training checkpoint to start from")
    p.add_argument("--global_pool", action="store_true")
    p.set_defaults(global_pool=True)
    p.add_argument("--cls_token", action="store_false", dest="global_pool")
    p.add_argument("--data_path", default="/datasets01/imagenet_full_size/061417/", type=str)
    p.add_argument("--nb_classes", default=1000, type=int)
    p.add_argument("--output_dir", default=os.path.join("checkpoints", "mae", "finetune"))
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--eval", action="store_true")
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--log_every", default=20, type=int)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"],
                   help="of the encoder (fp16 = the reference's `--precision amp` arithmetic, with dynamic loss scaling)")
    return p


def check_supported(args) -> None:
    """Refuse what the recipe's flags can ask for and this package has not built, naming the gap."""
    gaps = []
    if float(args.drop_path) != 0.0:
        gaps.append(f"--drop_path {args.drop_path}: stochastic depth is not built (it needs a per-row scale in the residual GEMM "
                    "epilogues); only 0.0 runs -- the reference's default is 0.1")
    if args.aa not in (None, "", "none"):
        gaps.append(f"--aa {args.aa}: timm's AutoAugment / RandAugment policies are not built")
    if float(args.reprob or 0.0) != 0.0:
        gaps.append(f"--reprob {args.reprob}: random erasing is not built")
    if args.color_jitter is not None:
        gaps.append(f"--color_jitter {args.color_jitter}: timm's create_transform colour jitter is not built")
    if args.dist_eval or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        gaps.append("--dist_eval / more than one process: the fine-tune loop runs on one GPU")
    if args.cutmix_minmax is not None:
        gaps.append("--cutmix_minmax: only cutmix alpha is built")
    if args.mixup_mode != "batch":
        gaps.append(f"--mixup_mode {args.mixup_mode}: only 'batch' is built")
    if gaps:
        raise NotImplementedError("main_finetune_mae: " + "; ".join(gaps))


def build_model(args, device):
    model = getattr(models_vit, args.model)(num_classes=args.nb_classes, global_pool=args.global_pool, precision=args.precision)
    if args.input_size != model.patch_embed.img_size[0]:
        raise NotImplementedError(f"--input_size {args.input_size}: the model runs at {model.patch_embed.img_size[0]} "
                                  "(position-embedding interpolation is not built)")
    if args.finetune and not args.eval:
        ckpt = torch.load(args.finetune, map_location="cpu", weights_only=False)
        print(f"Load pre-trained checkpoint from: {args.finetune}")
        print(models_vit.load_pretrained_for_finetune(model, ckpt["model"]))
    model.to(device)
    model._rt.ensure(device)   # binds the parameters to the flat device storage before the optimiser looks at them
    return model


def mix_rng(seed: int, epoch: int) -> np.random.RandomState:
    """The mixing draws of one epoch: a function of (seed, epoch) alone, like the crop generator."""
    return np.random.RandomState([int(seed) & 0x7FFFFFFF, int(epoch)])


def run(args, train_loader=None, val_loader=None):
    """-> (model, optimizer, history): history holds one {"epoch", "train", "test"} record per epoch run (--eval: one "test")."""
    from .data import DeviceAugmenter, draw_linprobe_boxes, preprocess_u8
    from .folder import folder_loader
    check_supported(args)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    mixup_fn = None
    if args.mixup > 0 or args.cutmix > 0.0:
        print("Mixup is activated!")
        mixup_fn = Mixup(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, prob=args.mixup_prob,
                         switch_prob=args.mixup_switch_prob, mode=args.mixup_mode, label_smoothing=args.smoothing,
                         num_classes=args.nb_classes)
    model = build_model(args, device)
    n_parameters = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print("number of params (M): %.2f" % (n_parameters / 1.0e6))
    eff = args.batch_size * args.accum_iter
    if args.lr is None:
        args.lr = args.blr * eff / 256
    print(f"base lr: {args.lr * 256 / eff:.2e}\nactual lr: {args.lr:.2e}\naccumulate grad iterations: {args.accum_iter}\n"
          f"effective batch size: {eff}")
    groups = param_groups_lrd(model, args.weight_decay, no_weight_decay_list=model.no_weight_decay(), layer_decay=args.layer_decay)
    opt = FusedAdamW(model, groups, lr=args.lr)   # torch.optim.AdamW(param_groups, lr=args.lr): its default betas
    scaler = LossScaler() if args.precision == "fp16" else None
    if args.resume:
        args.start_epoch = load_mae_checkpoint(args.resume, model, opt, args, loss_scaler=scaler)
    aug = DeviceAugmenter(device, size=args.input_size)
    gen = torch.Generator()
    sampler = None
    if val_loader is None:
        extra = {"multiprocessing_context": "spawn", "persistent_workers": True} if args.num_workers > 0 else {}
        val_loader = torch.utils.data.DataLoader(_ValFrames(os.path.join(args.data_path, "val")), batch_size=args.batch_size,
                                                 shuffle=False, num_workers=args.num_workers, pin_memory=args.pin_mem,
                                                 drop_last=False, collate_fn=_val_collate, **extra)
        prepare_val = lambda batch: (preprocess_u8(batch[0].to(device, non_blocking=True)), batch[1].to(device, non_blocking=True))
    else:
        prepare_val = None
    prepare_train = None
    if train_loader is None and not args.eval:
        train_loader = folder_loader(os.path.join(args.data_path, "train"), args.batch_size, 1, 0, args.seed, args.num_workers,
                                     args.pin_mem)
        sampler = train_loader.sampler

        def prepare_train(batch):
            frames, labels = batch
            frames = frames.to(device, non_blocking=True)
            hw = frames.sizes
            boxes = draw_linprobe_boxes(len(frames), hw[:, 0], hw[:, 1], gen)
            return aug.mae_tail(aug.random_resized_crop(frames, boxes=boxes), generator=gen), labels.to(device, non_blocking=True)

    history = []
    if args.eval:
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        return model, opt, [{"test": test}]
    ckpt_dir = os.path.join(args.output_dir, "ckpts") if args.output_dir else None
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        gen.manual_seed(args.seed + epoch)
        if mixup_fn is not None:
            mixup_fn.rng = mix_rng(args.seed, epoch)
        if sampler is not None:
            sampler.set_epoch(args.seed + epoch)
        train = finetune_one_epoch(model, train_loader, opt, device, epoch, args, mixup_fn=mixup_fn, loss_scaler=scaler,
                                   prepare=prepare_train, log_every=args.log_every, printer=None)
        if ckpt_dir:
            save_mae_checkpoint(ckpt_dir, epoch, model, opt, args, scaler_state=scaler.state_dict() if scaler is not None else None)
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        max_accuracy = max(max_accuracy, test["acc1"])
        print(f"Max accuracy: {max_accuracy:.2f}%")
        history.append({"epoch": epoch, "train": train, "test": test})
        if args.output_dir:
            os.makedirs(args.output_dir, exist_ok=True)
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:   # main_finetune.py:366-375
                f.write(json.dumps({**{f"train_{k}": v for k, v in train.items()}, **{f"test_{k}": v for k, v in test.items()},
                                    "epoch": epoch, "n_parameters": n_parameters}) + "\n")
    return model, opt, history


if __name__ == "__main__":
    run(get_args_parser().parse_args())
