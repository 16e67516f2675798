"""Image-folder input for pre-training: what the reference builds with torchvision (mae/main_pretrain.py:161-190) --
datasets.ImageFolder over `data_path[/train]`, a DistributedSampler(shuffle=True, seed) and a DataLoader with drop_last -- restated
without torchvision (not a dependency of this project).  The workers decode only: each item is the RGB frame as Pillow's pil_loader
returns it, a batch is one packed `RaggedFrames` (frames keep their native sizes), and the whole transform runs on the device
behind `data.DevicePrefetcher(..., transform="mae")`.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .data import RaggedFrames
from .jpeg import JpegBatch

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def find_classes(root: str) -> Tuple[List[str], dict]:
    """torchvision folder.find_classes: the sorted immediate subdirectories (symlinks to directories count)."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
    return classes, {c: i for i, c in enumerate(classes)}


def make_dataset(root: str, class_to_idx: dict, extensions: Sequence[str] = IMG_EXTENSIONS) -> List[Tuple[str, int]]:
    """torchvision folder.make_dataset: per class in sorted order, sorted(os.walk(..., followlinks=True)) and sorted file names,
    extensions matched case-insensitively."""
    ext = tuple(e.lower() for e in extensions)
    samples = []
    for cls in sorted(class_to_idx):
        d = os.path.join(root, cls)
        if not os.path.isdir(d):
            continue
        for dirpath, _, fnames in sorted(os.walk(d, followlinks=True)):
            for f in sorted(fnames):
                path = os.path.join(dirpath, f)
                if path.lower().endswith(ext):
                    samples.append((path, class_to_idx[cls]))
    if not samples:
        raise FileNotFoundError(f"Found no valid file for the classes {', '.join(sorted(class_to_idx))}. "
                                f"Supported extensions are: {', '.join(extensions)}")
    return samples


def pil_loader(path: str) -> np.ndarray:
    """torchvision folder.pil_loader, as a decoded uint8 [H, W, 3] array."""
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


class ImageFolderFrames(torch.utils.data.Dataset):
    """torchvision.datasets.ImageFolder(root) without a transform: item i = (decoded RGB frame uint8 [H, W, 3], class index).
    decode="device": item i = (the file's bytes, class index) -- decoding is left to data.DeviceJpegDecoder (see jpeg_collate)."""

    def __init__(self, root: str, decode: str = "host"):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device'")
        self.root, self.decode = os.fspath(root), decode
        self.classes, self.class_to_idx = find_classes(self.root)
        self.samples = make_dataset(self.root, self.class_to_idx)
        self.targets = [t for _, t in self.samples]

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, i: int):
        path, target = self.samples[i]
        if self.decode == "device":
            with open(path, "rb") as f:
                return f.read(), target
        return pil_loader(path), target


def ragged_collate(items) -> Tuple[RaggedFrames, torch.Tensor]:
    """[(frame uint8 [H_b, W_b, 3], label), ...] -> (RaggedFrames, labels int64 [B])."""
    frames, labels = zip(*items)
    return RaggedFrames.from_frames(frames), torch.tensor(labels, dtype=torch.int64)


def jpeg_collate(items) -> Tuple[JpegBatch, torch.Tensor]:
    """[(file bytes, label), ...] -> (jpeg.JpegBatch, labels int64 [B]): baseline JPEGs packed for the device decoder, every other
    file decoded here as pil_loader does."""
    files, labels = zip(*items)
    return JpegBatch.from_bytes(files), torch.tensor(labels, dtype=torch.int64)


def folder_loader(root: str, batch_size: int, world: int = 1, rank: int = 0, seed: int = 0, num_workers: int = 10,
                  pin_memory: bool = True, decode: str = "host") -> torch.utils.data.DataLoader:
    """The reference's pre-training loader over ImageFolder(root) (main_pretrain.py:170-190): DistributedSampler(num_replicas=world,
    rank=rank, shuffle=True, seed=seed), drop_last=True.  Batches are (RaggedFrames, labels); call `loader.sampler.set_epoch(e)`
    once per epoch.  Workers only decode: they are spawned (never forked from a process that has opened the device) and kept
    alive across epochs.  decode="device": the workers only read and pack the files, batches are (jpeg.JpegBatch, labels), and
    data.DevicePrefetcher decodes them on the device into the same RaggedFrames."""
    ds = ImageFolderFrames(root, decode=decode)
    sampler = torch.utils.data.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=seed)
    extra = {"multiprocessing_context": "spawn", "persistent_workers": True} if num_workers > 0 else {}
    return torch.utils.data.DataLoader(ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers, pin_memory=pin_memory,
                                       drop_last=True, collate_fn=jpeg_collate if decode == "device" else ragged_collate, **extra)
