"""What the two MAE image-folder recipes share (main_linprobe: linear probing; main_finetune_mae: end-to-end fine-tuning): the common
flags, the lr resolution, the input pipeline of mae/main_linprobe.py:144-156 and the epoch loop around the recipe's own train call.

Training frames: folder.folder_loader on DATA/train, the workers only decode; on the device the crop of mae/util/crop.py
(data.draw_linprobe_boxes -- not torchvision's sampler) through DeviceAugmenter.random_resized_crop(bicubic), then flip / ToTensor /
Normalize (mae_tail).  Validation frames: the workers do Resize(256, bicubic) + CenterCrop(224) with Pillow, as the reference's workers
do, and the device normalises (preprocess_u8).  The crops, flips and the sampler's order of epoch e depend on (seed, e) alone, so a
resumed run continues as the uninterrupted one.  run_epochs(..., train_aug=timm_aug.TrainAugment(...)) puts timm's RandAugment and
random erasing around the normalise (DeviceAugmenter.timm_tail), drawn from (seed, e) as well; without it nothing changes.

Two flags move the remaining host work to the device without changing a byte of any batch; both default to `host`:
  --decode device          the train workers only read and pack the files (folder_loader(decode="device")); the step decodes the
                           JpegBatch with DeviceJpegDecoder into the RaggedFrames it then crops.  Files the device decoder does not
                           take (progressive or greyscale JPEG, PNG, ...) are decoded by the packer in the workers, as elsewhere.
  --val_transform device   the val workers only decode (or, with --decode device, only read and pack); Resize + CenterCrop run on
                           the device (DeviceAugmenter.resize_center_crop: Pillow's bicubic taps for the full resized size, evaluated
                           for the crop window only) behind a DevicePrefetcher(transform="mae_eval").  build_val_loader builds
                           either input; a loader the caller passes in is used as it is."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .train import evaluate_probe, load_mae_checkpoint, save_mae_checkpoint


def add_common_flags(p, precision_help: str):
    """The flags both parsers define.  The nine whose defaults differ between the recipes (batch_size, epochs, model, weight_decay,
    blr, min_lr, warmup_epochs, global_pool, output_dir) get theirs from the caller's set_defaults."""
    p.add_argument("--batch_size", type=int, help="batch size per GPU")
    p.add_argument("--epochs", type=int)
    p.add_argument("--accum_iter", default=1, type=int)
    p.add_argument("--model", type=str)
    p.add_argument("--weight_decay", type=float)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--blr", type=float)
    p.add_argument("--min_lr", type=float)
    p.add_argument("--warmup_epochs", type=int)
    p.add_argument("--finetune", default="", help="pre-training checkpoint to start from")
    p.add_argument("--global_pool", action="store_true")
    p.add_argument("--cls_token", action="store_false", dest="global_pool")
    p.add_argument("--data_path", default="/datasets01/imagenet_full_size/061417/", type=str)
    p.add_argument("--nb_classes", default=1000, type=int)
    p.add_argument("--output_dir")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--eval", action="store_true")
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"], help=precision_help)
    p.add_argument("--decode", default="host", choices=["host", "device"],
                   help="where the files are decoded: in the workers with Pillow, or on the device (baseline JPEG; the workers then "
                        "only read and pack the files, and decode what the device does not take)")
    p.add_argument("--val_transform", default="host", choices=["host", "device"],
                   help="where the validation Resize(256, bicubic) + CenterCrop runs: in the workers with Pillow, or on the device "
                        "(the same bytes)")
    return p


VAL_RESIZE = 256   # main_linprobe.py:152: Resize(256, interpolation=3) in front of CenterCrop(224)


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


def _normalise_on(device):
    """prepare(batch) of cropped host frames: (uint8 [B, S, S, 3], labels) -> (ToTensor + Normalize, f32 [B, 3, S, S], labels) on
    the device."""
    from .data import preprocess_u8

    def prepare(batch):
        frames, labels = batch
        return preprocess_u8(frames.to(device, non_blocking=True)), labels.to(device, non_blocking=True)

    return prepare


def build_val_loader(args, device, crop_size: int):
    """The validation input over DATA/val in file order, short last batch kept -> (loader, prepare): prepare(batch) gives (images f32
    [B, 3, crop_size, crop_size], labels) on the device; the images are the same bytes whatever the flags say.
      --val_transform host:   the workers run _ValFrames (Pillow), the device normalises;
      --val_transform device: the workers only decode (--decode host: RaggedFrames) or only read and pack the files (--decode
                              device: JpegBatch, decoded by DeviceJpegDecoder), and a DevicePrefetcher(transform="mae_eval") does
                              Resize + CenterCrop + normalise on its copy stream.  Its image tensor is a per-slot buffer that is
                              refilled two batches later."""
    from .data import DeviceAugmenter, DevicePrefetcher
    from .folder import ImageFolderFrames, jpeg_collate, ragged_collate
    root = os.path.join(args.data_path, "val")
    extra = {"multiprocessing_context": "spawn", "persistent_workers": True} if args.num_workers > 0 else {}
    common = dict(batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers, pin_memory=args.pin_mem, drop_last=False,
                  **extra)
    if args.val_transform == "host":
        return torch.utils.data.DataLoader(_ValFrames(root, VAL_RESIZE, crop_size), collate_fn=_val_collate, **common), \
            _normalise_on(device)
    loader = torch.utils.data.DataLoader(ImageFolderFrames(root, decode=args.decode),
                                         collate_fn=jpeg_collate if args.decode == "device" else ragged_collate, **common)
    return DevicePrefetcher(loader, device, augment=DeviceAugmenter(device, size=crop_size), transform="mae_eval",
                            eval_resize=VAL_RESIZE), lambda batch: (batch[0], batch[-1])


def start(args) -> torch.device:
    """The process's device, made current, and the host seeds."""
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    return device


def resolve_lr(args) -> None:
    """lr = blr * batch_size * accum_iter / 256 unless --lr was given, and the reference's print-out."""
    eff = args.batch_size * args.accum_iter
    if args.lr is None:
        args.lr = args.blr * eff / 256
    print(f"base lr: {args.lr * 256 / eff:.2e}\nactual lr: {args.lr:.2e}\naccumulate grad iterations: {args.accum_iter}\n"
          f"effective batch size: {eff}")


def run_epochs(args, model, opt, device, train_epoch, *, crop_size: int, train_loader, val_loader, prepare_given: bool, scaler=None,
               log_extra=None, log_encoding=None, train_aug=None):
    """Resume, build the loaders the caller did not pass, then --eval or the epoch loop -> (model, opt, history): history holds one
    {"epoch", "train", "test"} record per epoch run (--eval: one "test").

    train_epoch(epoch, train_loader, prepare_train) -> the epoch's train statistics: the recipe's own call.
    prepare_given: whether prepare_train / prepare_val (host batch -> device batch) are applied to loaders the CALLER passed as well
      (the probe), or only to the folder loaders built here, a passed loader yielding device batches as they are (the fine-tune).
    scaler: the fp16 loss scaler restored from / saved into the checkpoints.  log_extra: further keys of the log.txt line;
    log_encoding: the encoding log.txt is opened with.
    train_aug: a timm_aug.TrainAugment -- prepare_train then runs DeviceAugmenter.timm_tail (flip -> RandAugment -> normalise ->
      random erasing) instead of mae_tail, and every epoch reseeds its host generator and erasing key from (seed, epoch).  None:
      every draw, launch and bit is the recipe's without it."""
    from .data import DeviceAugmenter, DeviceJpegDecoder, draw_linprobe_boxes
    from .folder import folder_loader
    from .jpeg import JpegBatch
    if args.resume:
        args.start_epoch = load_mae_checkpoint(args.resume, model, opt, args, loss_scaler=scaler)
    aug = DeviceAugmenter(device, size=crop_size)
    gen = torch.Generator()
    sampler = None
    decoder = DeviceJpegDecoder(device)

    def prepare_train(batch):
        frames, labels = batch
        frames = frames.to(device, non_blocking=True)
        if isinstance(frames, JpegBatch):   # (--decode device: the RaggedFrames the workers would have decoded, byte for byte)
            frames = decoder(frames)
        hw = frames.sizes
        boxes = draw_linprobe_boxes(len(frames), hw[:, 0], hw[:, 1], gen)
        crop = aug.random_resized_crop(frames, boxes=boxes)
        images = aug.mae_tail(crop, generator=gen) if train_aug is None else aug.timm_tail(crop, train_aug, generator=gen)
        return images, labels.to(device, non_blocking=True)

    prepare_val = _normalise_on(device)
    if val_loader is None:
        val_loader, prepare_val = build_val_loader(args, device, crop_size)
    elif not prepare_given:
        prepare_val = None
    if train_loader is None and not args.eval:
        train_loader = folder_loader(os.path.join(args.data_path, "train"), args.batch_size, 1, 0, args.seed, args.num_workers,
                                     args.pin_mem, decode=args.decode)
        sampler = train_loader.sampler
    elif not prepare_given:
        prepare_train = None

    if args.eval:
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        return model, opt, [{"test": test}]
    history = []
    ckpt_dir = os.path.join(args.output_dir, "ckpts") if args.output_dir else None
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        gen.manual_seed(args.seed + epoch)
        if train_aug is not None:
            train_aug.reseed(args.seed, epoch)
        if sampler is not None:
            sampler.set_epoch(args.seed + epoch)
        train = train_epoch(epoch, train_loader, prepare_train)
        if ckpt_dir:
            save_mae_checkpoint(ckpt_dir, epoch, model, opt, args, scaler_state=scaler.state_dict() if scaler is not None else None)
        test = evaluate_probe(model, val_loader, device, prepare_val)
        print(f"Accuracy of the network on the {test['samples']} test images: {test['acc1']:.1f}%")
        max_accuracy = max(max_accuracy, test["acc1"])
        print(f"Max accuracy: {max_accuracy:.2f}%")
        history.append({"epoch": epoch, "train": train, "test": test})
        if args.output_dir:
            os.makedirs(args.output_dir, exist_ok=True)
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding=log_encoding) as f:
                f.write(json.dumps({**{f"train_{k}": v for k, v in train.items()}, **{f"test_{k}": v for k, v in test.items()},
                                    "epoch": epoch, **(log_extra or {})}) + "\n")
    return model, opt, history
