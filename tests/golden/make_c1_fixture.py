"""Generator of tests/golden/c1_sun_full.json -- the data side of BASELINE.json configs[0] ("ViT-B/16 SUP-imnet fine-tune on
the sun_full manifest, bs=8, fp32, CPU reference path: plumbing").

Runs the REFERENCE's own loaders in the build container (they import as-is):
    ssl4polyp.configs.manifests.load_split        data_packs/sun_full/{train,val,test}.csv
    ssl4polyp.configs.layered.load_layered_config config/exp/exp1.yaml (-> base.yaml defaults)
and derives what train_classification.py derives from them before its first step: per-class counts, the class weights
N / (n_class * count) (tc.py:5613-5630), pos_weight = neg / pos for the two-class packs (tc.py:6090-6102), the optimizer /
schedule settings (config/base.yaml), and -- with torch, as the reference does (nn.BCEWithLogitsLoss(pos_weight)) -- the loss
of a fixed logit vector on 8 training labels (every 577th row).  Only data is stored: counts, labels, numbers.

What the loaders returned is stored beside the fixture as well (tests/golden/c1_sun_full_inputs.npz: every row's label and
frame path per split, the resolved config as JSON), so that the derivation can be replayed without the reference checkout
(tests/test_c1_plumbing_cpu.py).

    SSL4POLYP_REFERENCE=<reference checkout> python tests/golden/make_c1_fixture.py
"""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

SPLITS = ("train", "val", "test")
CONFIG_KEYS = ("optimizer", "lr", "weight_decay", "batch_size", "epochs", "amp", "image_size")
INPUTS = Path(__file__).with_name("c1_sun_full_inputs.npz")


def read_reference(ref):
    """What the reference's loaders return for the sun_full pack and exp1.yaml: {split: (labels, frame paths)}, config."""
    sys.path.insert(0, str(Path(ref) / "src"))
    from ssl4polyp.configs import layered as L
    from ssl4polyp.configs import manifests as M
    pack = Path(ref) / "data_packs" / "sun_full"
    splits = {}
    for split in SPLITS:
        rows = M.load_split(pack / f"{split}.csv")
        splits[split] = ([int(r["label"]) for r in rows], [r["frame_path"] for r in rows])
    cfg = L.load_layered_config("exp/exp1.yaml")
    config = {k: cfg[k] for k in CONFIG_KEYS}
    config["scheduler"] = dict(cfg["scheduler"])
    config["seeds"] = list(cfg["seeds"])
    return splits, config


def save_inputs(splits, config, path=INPUTS):
    arrays = {"config_json": np.array(json.dumps(config, sort_keys=True))}
    for split, (labels, frames) in splits.items():
        arrays[f"{split}_labels"] = np.asarray(labels, dtype=np.int8)
        arrays[f"{split}_frame_paths"] = np.asarray(frames, dtype=np.str_)
    np.savez_compressed(path, **arrays)


def load_inputs(arrays):
    """The inverse of save_inputs, from the npz's arrays."""
    splits = {s: ([int(v) for v in arrays[f"{s}_labels"]], [str(v) for v in arrays[f"{s}_frame_paths"]]) for s in SPLITS}
    return splits, json.loads(str(arrays["config_json"]))


def derive(splits, config):
    out = {"pack": "sun_full", "splits": {}}
    for split in SPLITS:
        lab, frames = splits[split]
        counts = np.bincount(lab, minlength=2).tolist()
        out["splits"][split] = {"rows": len(lab), "class_counts": counts, "first_frame": frames[0]}
    train = splits["train"][0]
    counts = np.bincount(train, minlength=2)
    n_class = len(set(train))
    out["n_class"] = n_class
    out["class_weights"] = [float(len(train) / (n_class * c)) for c in counts]   # tc.py:5621-5624
    out["pos_weight"] = float(counts[0]) / float(counts[1])                      # tc.py:6092-6096
    out["config"] = dict(config)
    # C1: per-rank batch 8, fp32.  First 8 training labels + a fixed logit vector through the reference's loss construction.
    first8 = train[:: len(train) // 8][:8]  # (the CSV is ordered by case: a strided sample carries both classes)
    rng = np.random.Generator(np.random.PCG64(77))
    logits = rng.standard_normal((8, 2)).astype(np.float32)
    z = torch.from_numpy(logits)
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(out["pos_weight"], dtype=torch.float32))(
        z[:, 1] - z[:, 0], torch.tensor(first8, dtype=torch.float32))
    out["c1_batch"] = {"labels": first8, "logits": logits.tolist(), "bce_loss": float(loss)}
    return out


def build(ref=None):
    return derive(*read_reference(ref or os.environ["SSL4POLYP_REFERENCE"]))


if __name__ == "__main__":
    splits, config = read_reference(os.environ["SSL4POLYP_REFERENCE"])
    save_inputs(splits, config)
    dst = Path(__file__).with_name("c1_sun_full.json")
    dst.write_text(json.dumps(derive(splits, config), indent=1, sort_keys=True) + "\n")
    print("wrote", dst, "and", INPUTS)
