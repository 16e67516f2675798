"""CSV-pack input for fine-tuning and evaluation: what the reference builds in classification/data/packs.py -- PackDataset over the
(paths, labels, rows) triple of a pack split, pack_collate, and the loaders of create_classification_dataloaders (:319-389) --
with the transform taken out of the workers.  An item is the decoded RGB frame (decode="host") or the file's bytes
(decode="device"), a batch is (data.RaggedFrames | jpeg.JpegBatch, labels int64 [B], rows), and the whole transform runs on the
device behind data.DevicePrefetcher: the train transform (transform="train"), or the eval transform with the rows' Exp-5
perturbations (transform="eval", data.DevicePerturber).  `device_pack_loaders` ties the pieces together; main_finetune.py is the
entry point that uses it.

A user of the reference keeps its manifest loader (SHA / count verification, snapshots) and hands `load_pack`'s triple to
`PackFrames`; `read_pack_csv` is the minimal reader for everyone else: csv.DictReader rows as they are, int labels, and the path
rule of configs/manifests.py resolve_paths.
"""
from __future__ import annotations

import csv
import os
import random
from pathlib import Path
from typing import List, Mapping, Optional, Sequence, Tuple

import torch

from .data import RaggedFrames
from .folder import pil_loader
from .jpeg import JpegBatch

REQUIRED_COLUMNS = ("frame_path", "label")   # configs/manifests.py:41


def resolve_frame_path(row: Mapping[str, str], roots_map: Optional[Mapping[str, str]] = None) -> Path:
    """The path rule of a pack (the reference's configs/manifests.py resolve_paths, pinned by tests/golden/pack_paths.json).  Three
    candidates in order of precedence, the first whose key is in the map wins: the path's first component (replaced by its root),
    the row's `store_id`, the row's `dataset` (their root is prefixed to the whole path).  Nothing in the map: the path as written."""
    if row.get("frame_path") is None:
        raise ValueError("row without a 'frame_path'")
    path = Path(row["frame_path"])
    if not roots_map or not path.parts:
        return path
    head, tail = path.parts[0], path.parts[1:]
    candidates = [(head, Path(*tail) if tail else Path())] + [(row.get(k), path) for k in ("store_id", "dataset") if row.get(k)]
    for key, rest in candidates:
        if roots_map.get(key) is not None:
            return Path(roots_map[key]) / rest
    return path


def read_pack_csv(csv_path, roots_map: Optional[Mapping[str, str]] = None, sample: int = 10) -> Tuple[List[str], List[int], List[dict]]:
    """One split of a pack -> (paths, labels, rows): the rows exactly as csv.DictReader reads them (dicts of strings: what
    data.perturbation_plan expects), labels through int() (an empty label raises), paths by `resolve_frame_path`.  As the reference
    does, up to `sample` random paths are checked for existence (FileNotFoundError)."""
    with open(csv_path, newline="") as f:
        reader = csv.DictReader(f)
        missing = set(REQUIRED_COLUMNS) - set(reader.fieldnames or [])
        if missing:
            raise ValueError(f"Missing required columns {sorted(missing)} in {csv_path}")
        rows = [dict(r) for r in reader]
    labels = []
    for i, row in enumerate(rows, start=1):
        if row["label"] in (None, ""):
            raise ValueError(f"Empty label in {csv_path} row {i}")
        labels.append(int(row["label"]))
    paths = [resolve_frame_path(r, roots_map) for r in rows]
    for p in random.sample(paths, min(sample, len(paths))):
        if not p.exists():
            raise FileNotFoundError(f"Missing file referenced in manifest: {p}")
    return [str(p) for p in paths], labels, rows


class PackFrames(torch.utils.data.Dataset):
    """PackDataset (packs.py:24-80) without its transform, over the triple the reference's load_pack (or read_pack_csv) returns:
    item i = (frame, label, row), or (frame, row) when labels is None.  frame: the decoded RGB frame uint8 [H, W, 3]
    (decode="host", folder.pil_loader) or the file's bytes (decode="device": decoding is left to data.DeviceJpegDecoder)."""

    def __init__(self, paths: Sequence, labels: Optional[Sequence], rows: Optional[Sequence[Mapping]], decode: str = "host"):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device'")
        self.paths = [os.fspath(p) for p in paths]
        self.decode = decode
        self.labels = None
        if labels is not None:
            if len(labels) != len(self.paths):
                raise ValueError("one label per path")
            self.labels = []
            for label in labels:
                if label in (None, ""):
                    raise ValueError("Encountered empty label while preparing PackFrames.")
                self.labels.append(int(label))
        self.rows = [dict(r) for r in rows] if rows else [{} for _ in self.paths]
        if len(self.rows) != len(self.paths):
            raise ValueError("one metadata row per path")

    def __len__(self) -> int:
        return len(self.paths)

    def __getitem__(self, i: int):
        path = self.paths[i]
        if self.decode == "device":
            with open(path, "rb") as f:
                frame = f.read()
        else:
            frame = pil_loader(path)
        if self.labels is None:
            return frame, self.rows[i]
        return frame, self.labels[i], self.rows[i]


def _split_samples(batch):
    """(frames, labels int64 [B] or None, rows) of a list of PackFrames items.  Every item must have the shape of the first one --
    (frame, label, row) or (frame, row): a batch mixing labelled and unlabelled samples raises, as the reference's pack_collate
    does."""
    if not batch:
        raise ValueError("cannot collate an empty batch")
    width = len(batch[0])
    if width not in (2, 3):
        raise ValueError(f"a sample is (frame, label, row) or (frame, row), got {width} elements")
    if any(len(sample) != width for sample in batch):
        raise ValueError("Mixed batch with and without labels is not supported")
    frames = [sample[0] for sample in batch]
    rows = [sample[-1] for sample in batch]
    labels = torch.tensor([int(sample[1]) for sample in batch], dtype=torch.int64) if width == 3 else None
    return frames, labels, rows


def pack_ragged_collate(batch):
    """[(frame uint8 [H_b, W_b, 3], label, row), ...] -> (RaggedFrames, labels int64 [B], rows): pack_collate with the image tensor
    replaced by the untransformed batch ((RaggedFrames, rows) for unlabelled samples)."""
    frames, labels, rows = _split_samples(batch)
    x = RaggedFrames.from_frames(frames)
    return (x, rows) if labels is None else (x, labels, rows)


def pack_jpeg_collate(batch):
    """[(file bytes, label, row), ...] -> (jpeg.JpegBatch, labels int64 [B], rows): baseline JPEGs packed for the device decoder,
    every other file decoded here as folder.pil_loader does."""
    files, labels, rows = _split_samples(batch)
    x = JpegBatch.from_bytes(files)
    return (x, rows) if labels is None else (x, labels, rows)


def pack_loader(dataset: PackFrames, batch_size: int, stage: str, world: int = 1, rank: int = 0, seed: int = 0, num_workers: int = 8,
                pin_memory: bool = True, drop_last: Optional[bool] = None) -> torch.utils.data.DataLoader:
    """One loader of create_classification_dataloaders (packs.py:319-389).  stage="train": shuffled -- DistributedSampler(shuffle=True,
    seed=seed, drop_last=...) when world > 1 (call `loader.sampler.set_epoch(e)` per epoch), else a RandomSampler whose generator is
    seeded from `seed` (repeatable runs); drop_last defaults to True and is switched off when the dataset, or a replica's share of
    it, is smaller than batch_size; zero train batches raise the reference's RuntimeError.  "val" / "test": sequential, complete.
    Workers only read (and decode): spawned -- never forked from a process that has opened the device -- and kept alive across
    epochs, as in folder.folder_loader."""
    if stage not in ("train", "val", "test"):
        raise ValueError("stage must be 'train', 'val' or 'test'")
    n = len(dataset)
    sampler = None
    drop = False
    zero = ("Training dataloader constructed zero batches; reduce batch_size or disable drop_last. "
            f"Samples available={n}, batch_size={batch_size}, world_size={world}.")
    if stage == "train":
        if n == 0:   # (a sampler over nothing cannot even be built)
            raise RuntimeError(zero)
        drop = True if drop_last is None else bool(drop_last)
        if n < batch_size:
            drop = False
        elif world > 1 and drop and n // world < batch_size:
            drop = False
        if world > 1:
            sampler = torch.utils.data.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, seed=seed, drop_last=drop)
        else:
            sampler = torch.utils.data.RandomSampler(dataset, generator=torch.Generator().manual_seed(seed))
    extra = {"multiprocessing_context": "spawn", "persistent_workers": True} if num_workers > 0 else {}
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, sampler=sampler, num_workers=num_workers,
                                         pin_memory=pin_memory, drop_last=drop,
                                         collate_fn=pack_jpeg_collate if dataset.decode == "device" else pack_ragged_collate, **extra)
    if stage == "train" and len(loader) == 0:
        raise RuntimeError(zero)
    return loader


def device_pack_loaders(splits: Mapping[str, Tuple], device, batch_size: int, image_size: int = 224, decode: str = "host",
                        world: int = 1, rank: int = 0, seed: int = 0, num_workers: int = 8, pin_memory: bool = True,
                        perturbation_splits: Sequence[str] = (), hmac_key: Optional[bytes] = None, fused_decode: bool = False,
                        drop_last: Optional[bool] = None):
    """splits: {"train" | "val" | "test": (paths, labels, rows)} -> ({split: data.DevicePrefetcher}, train sampler or None).  Every
    loader yields (images f32 [B, 3, S, S] on the device, labels, rows) -- what train.train_epoch_cls / evaluate_cls iterate over.
    train: the train transform on the device, its draws from a generator seeded with seed + rank, labels on the device.
    val / test: the eval transform, with the rows' perturbations only for the splits named in perturbation_splits (packs.py
    _build_transforms), labels left on the host (evaluate_cls reads them there).  The sampler is the train loader's (set_epoch
    when it is a DistributedSampler)."""
    from .data import DEFAULT_HMAC_KEY, DeviceAugmenter, DevicePerturber, DevicePrefetcher
    unknown = set(splits) - {"train", "val", "test"}
    if unknown:
        raise ValueError(f"unknown splits {sorted(unknown)}")
    perturbed = {s.lower() for s in perturbation_splits}
    loaders, sampler = {}, None
    for split, (paths, labels, rows) in splits.items():
        loader = pack_loader(PackFrames(paths, labels, rows, decode=decode), batch_size, split, world, rank, seed, num_workers,
                             pin_memory, drop_last)
        augment = DeviceAugmenter(device, size=image_size)
        if split == "train":
            sampler = loader.sampler
            loaders[split] = DevicePrefetcher(loader, device, augment=augment, transform="train", fused_decode=fused_decode,
                                              generator=torch.Generator().manual_seed(seed + rank))
        else:
            perturb = DevicePerturber(device, key=hmac_key or DEFAULT_HMAC_KEY) if split in perturbed else None
            loaders[split] = DevicePrefetcher(loader, device, augment=augment, transform="eval", perturb=perturb,
                                              rest_to_device=False, fused_decode=fused_decode)
    return loaders, sampler
