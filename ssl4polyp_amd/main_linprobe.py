"""Linear probing of a pre-trained encoder on the MI355X engine -- the flag surface and behaviour of the reference's
src/ssl4polyp/models/mae/main_linprobe.py: a frozen ViT (models_vit), BatchNorm1d(affine=False) + Linear head, LARS without weight
decay, lr = blr * batch_size * accum_iter * world / 256 (:259-262), per-iteration half-cosine schedule with warm-up, softmax
cross-entropy, acc@1 / acc@5 on DATA/val after every epoch, checkpoint-<epoch>.pth in the dict main_pretrain writes.

    python -m ssl4polyp_amd.main_linprobe --finetune ckpts/checkpoint-399.pth --data_path /data/imagenet --nb_classes 1000
    python -m ssl4polyp_amd.main_linprobe --resume out/ckpts/checkpoint-89.pth --eval --data_path ...

Training frames (main_linprobe.py:144-150): folder.folder_loader on DATA/train, the workers only decode; on the device the crop of
mae/util/crop.py (data.draw_linprobe_boxes -- not torchvision's sampler) through DeviceAugmenter.random_resized_crop(bicubic), then
flip / ToTensor / Normalize (mae_tail).  Validation frames (:151-156): the workers do Resize(256, bicubic) + CenterCrop(224) with
Pillow, as the reference's workers do, and the device normalises (preprocess_u8).  The crops, flips and the sampler's order of epoch
e depend on (seed, e) alone, so a resumed run continues as the uninterrupted one.

The head, its loss and LARS run in f32 in every --precision; the encoder runs in the chosen mode (the reference's autocast also runs
the Linear in fp16).  One process, one GPU: the reference's per-rank BatchNorm under DDP and --dist_eval are accepted flags only."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from . import models_vit
from .optim import FusedLARS
from .train import evaluate_probe, linprobe_one_epoch, load_mae_checkpoint, save_mae_checkpoint


def get_args_parser():
    p = argparse.ArgumentParser("MAE linear probing (MI355X)", add_help=True)
    p.add_argument("--batch_size", default=512, type=int, help="batch size per GPU")
    p.add_argument("--epochs", default=90, type=int)
    p.add_argument("--accum_iter", default=1, type=int)
    p.add_argument("--model", default="vit_base_patch16", type=str)
    p.add_argument("--weight_decay", type=float, default=0)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--blr", type=float, default=0.1)
    p.add_argument("--min_lr", type=float, default=0.0)
    p.add_argument("--warmup_epochs", type=int, default=10)
    p.add_argument("--finetune", default="", help="pre-training checkpoint to probe")
    p.add_argument("--global_pool", action="store_true")
    p.set_defaults(global_pool=False)
    p.add_argument("--cls_token", action="store_false", dest="global_pool")
    p.add_argument("--data_path", default="/datasets01/imagenet_full_size/061417/", type=str)
    p.add_argument("--nb_classes", default=1000, type=int)
    p.add_argument("--output_dir", default="./output_dir")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--eval", action="store_true")
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"],
                   help="of the frozen encoder (fp16 = the reference's `--precision amp` arithmetic); the head runs in f32")
    return p


class _ValFrames(torch.utils.data.Dataset):
    """main_linprobe.py:151-156 in the workers: Resize(256, interpolation=3) + CenterCrop(224) with Pillow -> uint8 [224, 224, 3]."""

    def __init__(self, root: str, resize: int = 256, crop: int = 224):
        from .folder import find_classes, make_dataset
        self.classes, self.class_to_idx = find_classes(root)
        self.samples = make_dataset(root, self.class_to_idx)
        self.resize, self.crop = resize, crop

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        from PIL import Image
        path, target = self.samples[i]
        with open(path, "rb") as f:
            img = Image.open(f).convert("RGB")
        w, h = img.size
        if (w <= h and w != self.resize) or (h <= w and h != self.resize):   # torchvision Resize(int): the shorter side
            nw, nh = (self.resize, int(self.resize * h / w)) if w <= h else (int(self.resize * w / h), self.resize)
            img = img.resize((nw, nh), Image.BICUBIC)
            w, h = nw, nh
        top, left = int(round((h - self.crop) / 2.0)), int(round((w - self.crop) / 2.0))   # torchvision center_crop
        return np.asarray(img.crop((left, top, left + self.crop, top + self.crop))), target


def _val_collate(items):
    frames, labels = zip(*items)
    return torch.from_numpy(np.stack(frames)), torch.tensor(labels, dtype=torch.int64)


def build_model(args, device):
    model = getattr(models_vit, args.model)(num_classes=args.nb_classes, global_pool=args.global_pool, precision=args.precision)
    if args.finetune and not args.eval:
        ckpt = torch.load(args.finetune, map_location="cpu", weights_only=False)
        print(f"Load pre-trained checkpoint from: {args.finetune}")
        print(models_vit.load_pretrained_for_probe(model, ckpt["model"]))
    models_vit.add_probe_head(model)
    model.to(device)
    model._rt.ensure(device)   # binds the parameters to the flat device storage before the optimiser looks at them
    return model


def run(args, train_loader=None, val_loader=None):
    """-> (model, optimizer, history): history holds one {"epoch", "train", "test"} record per epoch run (--eval: one "test")."""
    from .data import DeviceAugmenter, draw_linprobe_boxes, preprocess_u8
    from .folder import folder_loader
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    model = build_model(args, device)
    eff = args.batch_size * args.accum_iter
    if args.lr is None:
        args.lr = args.blr * eff / 256
    print(f"base lr: {args.lr * 256 / eff:.2e}\nactual lr: {args.lr:.2e}\naccumulate grad iterations: {args.accum_iter}\n"
          f"effective batch size: {eff}")
    opt = FusedLARS(model.head.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    if args.resume:
        args.start_epoch = load_mae_checkpoint(args.resume, model, opt, args)
    aug = DeviceAugmenter(device, size=224)
    gen = torch.Generator()
    sampler = None
    if val_loader is None:
        extra = {"multiprocessing_context": "spawn", "persistent_workers": True} if args.num_workers > 0 else {}
        val_loader = torch.utils.data.DataLoader(_ValFrames(os.path.join(args.data_path, "val")), batch_size=args.batch_size,
                                                 shuffle=False, num_workers=args.num_workers, pin_memory=args.pin_mem,
                                                 drop_last=False, collate_fn=_val_collate, **extra)
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

    def prepare_val(batch):
        frames, labels = batch
        return preprocess_u8(frames.to(device, non_blocking=True)), labels.to(device, non_blocking=True)

    history = []
    if args.eval:
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        return model, opt, [{"test": test}]
    ckpt_dir = os.path.join(args.output_dir, "ckpts") if args.output_dir else None
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        gen.manual_seed(args.seed + epoch)
        if sampler is not None:
            sampler.set_epoch(args.seed + epoch)
        train = linprobe_one_epoch(model, train_loader, opt, device, epoch, args, prepare_train, printer=None)
        if ckpt_dir:
            save_mae_checkpoint(ckpt_dir, epoch, model, opt, args)
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        max_accuracy = max(max_accuracy, test["acc1"])
        print(f"Max accuracy: {max_accuracy:.2f}%")
        history.append({"epoch": epoch, "train": train, "test": test})
        if args.output_dir:
            os.makedirs(args.output_dir, exist_ok=True)
            with open(os.path.join(args.output_dir, "log.txt"), "a") as f:   # main_linprobe.py:327-335
                f.write(json.dumps({**{f"train_{k}": v for k, v in train.items()}, **{f"test_{k}": v for k, v in test.items()},
                                    "epoch": epoch}) + "\n")
    return model, opt, history


if __name__ == "__main__":
    run(get_args_parser().parse_args())
