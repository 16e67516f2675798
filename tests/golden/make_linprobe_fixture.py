"""Writes tests/golden/linprobe.npz by running the reference's linear-probe pieces themselves, in float64, on stored features:
  LARS                       loaded from <reference>/src/ssl4polyp/models/mae/util/lars.py by file path
  adjust_learning_rate       loaded from .../util/lr_sched.py
  RandomResizedCrop.get_params  loaded from .../util/crop.py, with `torchvision.transforms` stubbed (the sampler itself
                             only needs torch and math; the stub's _get_image_size returns the (width, height) it is given)
  the head                   torch.nn.Sequential(BatchNorm1d(D, affine=False, eps=1e-6), Linear(D, C)), torch.nn.CrossEntropyLoss()
and the training step of engine_finetune.train_one_epoch as main_linprobe calls it: lr adjusted when step % accum_iter == 0 at
step / len(loader) + epoch, loss / accum_iter, update + zero_grad every accum_iter steps.

Runs (12 micro-steps each, accum_iter 2, 4 micro-batches per epoch -> 3 epochs, warm-up 1 epoch: the run crosses its end):
  c2_wd0, c2_wd5, c7_wd0, c7_wd5   B = 16, D = 64, C in {2, 7}, weight_decay in {0, 0.05}
  vitb                             B = 8, D = 768, C = 2, two steps of accum_iter 1 (the first at the warm-up's lr 0)
Beside the head's weight and bias the optimiser holds two planted matrices: `zero` (all-zero parameter, non-zero gradient: the
param_norm == 0 branch of lars.py:36 until the first non-zero lr moves it) and `still` (non-zero parameter, zero gradient: with
weight_decay 0 the update_norm == 0 branch).  Recorded after every micro-step: loss (undivided), lr, head.*, every mu, the planted
matrices; once: features, targets, gradients of the planted matrices, the initial values, the eval-mode logits of the final head,
the state_dict key lists, the boxes of get_params.

Usage: python tests/golden/make_linprobe_fixture.py <reference checkout>"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ACCUM, PER_EPOCH, STEPS = 2, 4, 12
LR, MIN_LR, WARMUP, EPOCHS = 0.5, 0.0, 1, 3
RUNS = {"c2_wd0": (16, 64, 2, 0.0), "c2_wd5": (16, 64, 2, 0.05), "c7_wd0": (16, 64, 7, 0.0), "c7_wd5": (16, 64, 7, 0.05)}
BOX_SEED, BOX_SIZES = 11, [(224, 224), (640, 480), (333, 500), (17, 9)]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stub_torchvision():
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")
    fn._get_image_size = lambda img: img
    tr.RandomResizedCrop = type("RandomResizedCrop", (), {})
    tr.functional = fn
    tv.transforms = tr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})


def _inputs(B, D, C, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(PER_EPOCH, B, D, generator=g, dtype=torch.float64) * 1.5 + 0.3
    feats[..., 5] = 0.75                                 # a constant column: zero variance, xhat exactly 0
    targets = torch.randint(0, C, (PER_EPOCH, B), generator=g)
    targets[targets == C - 1] = 0 if C > 2 else 1        # with C > 2 the last class is never a target
    W0 = torch.nn.init.trunc_normal_(torch.empty(C, D, dtype=torch.float64), std=0.01, generator=g)
    b0 = torch.randn(C, generator=g, dtype=torch.float64) * 0.01
    still0 = torch.randn(5, 6, generator=g, dtype=torch.float64)
    zero_grad = torch.randn(3, 7, generator=g, dtype=torch.float64)
    return feats, targets, W0, b0, still0, zero_grad


def run(LARS, adjust, B, D, C, wd, seed, steps=STEPS, accum=ACCUM, per_epoch=PER_EPOCH):
    feats, targets, W0, b0, still0, zero_grad = _inputs(B, D, C, seed)
    head = torch.nn.Sequential(torch.nn.BatchNorm1d(D, affine=False, eps=1e-6), torch.nn.Linear(D, C)).double()
    with torch.no_grad():
        head[1].weight.copy_(W0)
        head[1].bias.copy_(b0)
    zero = torch.nn.Parameter(torch.zeros(3, 7, dtype=torch.float64))
    still = torch.nn.Parameter(still0.clone())
    named = [("head.1.weight", head[1].weight), ("head.1.bias", head[1].bias), ("zero", zero), ("still", still)]
    opt = LARS([p for _, p in named], lr=LR, weight_decay=wd)
    args = types.SimpleNamespace(lr=LR, min_lr=MIN_LR, warmup_epochs=WARMUP, epochs=EPOCHS)
    crit = torch.nn.CrossEntropyLoss()
    rec = {k: [] for k in ("loss", "lr", "acc1", "acc5", "running_mean", "running_var", "tracked", "updated")}
    rec.update({n: [] for n, _ in named})
    rec.update({"mu." + n: [] for n, _ in named})
    head.train()
    opt.zero_grad()
    for it in range(steps):
        epoch, step = divmod(it, per_epoch)
        if step % accum == 0:
            adjust(opt, step / per_epoch + epoch, args)
        x, y = feats[step % feats.shape[0]], targets[step % feats.shape[0]]
        out = head(x)
        loss = crit(out, y)
        rec["loss"].append(loss.item())
        k = min(5, C)
        top = out.topk(k, 1).indices
        rec["acc1"].append(int((top[:, 0] == y).sum()))
        rec["acc5"].append(int((top == y[:, None]).any(1).sum()))
        (loss / accum).backward()
        for p, g in ((zero, zero_grad), (still, torch.zeros_like(still))):  # the planted gradients accumulate like the head's
            p.grad = g / accum if p.grad is None else p.grad + g / accum
        update = (step + 1) % accum == 0
        if update:
            opt.step()
            opt.zero_grad()
        rec["updated"].append(int(update))
        rec["lr"].append(opt.param_groups[0]["lr"])
        rec["running_mean"].append(head[0].running_mean.clone().numpy())
        rec["running_var"].append(head[0].running_var.clone().numpy())
        rec["tracked"].append(int(head[0].num_batches_tracked))
        for n, p in named:
            rec[n].append(p.detach().clone().numpy())
            mu = opt.state[p].get("mu")
            rec["mu." + n].append(mu.clone().numpy() if mu is not None else np.zeros(tuple(p.shape)))
    head.eval()
    with torch.no_grad():
        eval_logits = head(feats[0]).numpy()
    out = {k: np.asarray(v) for k, v in rec.items()}
    out.update(feats=feats.numpy(), targets=targets.numpy(), W0=W0.numpy(), b0=b0.numpy(), still0=still0.numpy(),
               zero_grad=zero_grad.numpy(), eval_logits=eval_logits, weight_decay=np.float64(wd))
    osd = opt.state_dict()
    keys = dict(model_keys=np.array(["head." + k for k in head.state_dict().keys()]),
                optim_group_keys=np.array(sorted(osd["param_groups"][0].keys())),
                optim_state_keys=np.array(sorted({k for st in osd["state"].values() for k in st.keys()})))
    return out, keys


def main(reference):
    util = os.path.join(reference, "src", "ssl4polyp", "models", "mae", "util")
    LARS = _load(os.path.join(util, "lars.py"), "ref_lars").LARS
    adjust = _load(os.path.join(util, "lr_sched.py"), "ref_lr_sched").adjust_learning_rate
    _stub_torchvision()
    crop = _load(os.path.join(util, "crop.py"), "ref_crop").RandomResizedCrop
    data = {}
    for i, (name, (B, D, C, wd)) in enumerate(RUNS.items()):
        out, keys = run(LARS, adjust, B, D, C, wd, seed=100 + i // 2)   # (the two weight decays of a shape share their inputs)
        if wd != 0.0:  # shared with the wd = 0 run of the same shape
            for k in ("feats", "targets", "W0", "b0", "still0", "zero_grad"):
                del out[k]
        data.update({f"{name}.{k}": v for k, v in out.items()})
    data.update(keys)
    out, _ = run(LARS, adjust, 8, 768, 2, 0.0, seed=200, steps=2, accum=1, per_epoch=2)   # (the first lr of a warm-up is 0)
    out["feats"] = out["feats"][:2]
    out["targets"] = out["targets"][:2]
    data.update({f"vitb.{k}": v for k, v in out.items()})
    data["schedule"] = np.array([ACCUM, PER_EPOCH, STEPS, WARMUP, EPOCHS], dtype=np.int64)
    data["schedule_lr"] = np.array([LR, MIN_LR])
    torch.manual_seed(BOX_SEED)
    boxes = []
    for n in range(32):
        W, H = BOX_SIZES[n % len(BOX_SIZES)]
        boxes.append(crop.get_params((W, H), (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)))
    data["boxes"] = np.array(boxes, dtype=np.int64)
    data["box_sizes"] = np.array(BOX_SIZES, dtype=np.int64)
    data["box_seed"] = np.int64(BOX_SEED)
    path = os.path.join(HERE, "linprobe.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", len(data), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
