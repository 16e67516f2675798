"""Linear probing of a pre-trained encoder on the MI355X engine -- the flag surface and behaviour of the reference's
src/ssl4polyp/models/mae/main_linprobe.py: a frozen ViT (models_vit), BatchNorm1d(affine=False) + Linear head, LARS without weight
decay, lr = blr * batch_size * accum_iter * world / 256 (:259-262), per-iteration half-cosine schedule with warm-up, softmax
cross-entropy, acc@1 / acc@5 on DATA/val after every epoch, checkpoint-<epoch>.pth in the dict main_pretrain writes.

    python -m ssl4polyp_amd.main_linprobe --finetune ckpts/checkpoint-399.pth --data_path /data/imagenet --nb_classes 1000
    python -m ssl4polyp_amd.main_linprobe --resume out/ckpts/checkpoint-89.pth --eval --data_path ...

The input pipeline (main_linprobe.py:144-156) and the epoch loop are mae_recipe's, shared with main_finetune_mae; a loader passed to
run() yields host batches and goes through the same device preparation as the folder loaders.

The head, its loss and LARS run in f32 in every --precision; the encoder runs in the chosen mode (the reference's autocast also runs
the Linear in fp16).  One process, one GPU: the reference's per-rank BatchNorm under DDP and --dist_eval are accepted flags only."""
from __future__ import annotations

import argparse

import torch

from . import mae_recipe, models_vit
from .optim import FusedLARS
from .train import linprobe_one_epoch


def get_args_parser():
    p = argparse.ArgumentParser("MAE linear probing (MI355X)", add_help=True)
    mae_recipe.add_common_flags(p, "of the frozen encoder (fp16 = the reference's `--precision amp` arithmetic); the head runs in f32")
    p.set_defaults(batch_size=512, epochs=90, model="vit_base_patch16", weight_decay=0, blr=0.1, min_lr=0.0, warmup_epochs=10,
                   global_pool=False, output_dir="./output_dir")
    return p


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
    device = mae_recipe.start(args)
    model = build_model(args, device)
    mae_recipe.resolve_lr(args)
    opt = FusedLARS(model.head.parameters(), lr=args.lr, weight_decay=args.weight_decay)

    def train_epoch(epoch, loader, prepare):
        return linprobe_one_epoch(model, loader, opt, device, epoch, args, prepare, printer=None)

    return mae_recipe.run_epochs(args, model, opt, device, train_epoch, crop_size=224, train_loader=train_loader, val_loader=val_loader,
                                 prepare_given=True)   # log.txt as main_linprobe.py:327-335 writes it: the locale's encoding


if __name__ == "__main__":
    run(get_args_parser().parse_args())
