#!/usr/bin/env python3
"""Recorded results of the reference's staged fine-tuning helpers, by RUNNING THE REFERENCE's own functions
(src/ssl4polyp/classification/train_classification.py: _sanitize_finetune_schedule_config :721-776, _materialize_finetune_schedule
:860-903, FinetuneScheduleRuntime :906-953, create_scheduler :3943-3971, _resolve_monitor_mode / _improved :3297-3333,
_should_trigger_early_stop :3903-3915):

    python tests/golden/make_finetune_schedule_fixture.py [--reference /root/reference]        (build container only)

train_classification.py imports torchvision through the package's transforms; torchvision is not installed, so an EMPTY module of that
name is put into sys.modules for the import, as make_perturb_fixtures.py does.  Written: tests/golden/finetune_schedule.json, which
holds results only -- the input specs (the four Exp-5C budget files' `protocol.finetune_schedule` lists, read with PyYAML, and a few
edge specs), the materialised stages, per-epoch traces of stage / mode / group lrs / trainable parameters under each scheduler, the
monitor modes, and the early-stopping traces.  tests/test_finetune_schedule_cpu.py holds ssl4polyp_amd.train to every value with ==.
"""
import argparse
import dataclasses
import json
import os
import sys
import types

import torch
import torch.nn as nn
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))

EDGE_SPECS = {
    "backbone_lr_scale": [{"mode": "head+2", "epochs": 3, "backbone_lr_scale": 0.1}],
    "stage_lr": [{"mode": "full", "epochs": 2, "lr": 2e-4}, {"epochs": 2, "lr": 1e-4, "backbone_lr_scale": 0.5}],
    "none_without_backbone_lr": [{"mode": "none", "epochs": 4, "head_lr": 1e-3, "backbone_lr_scale": 0.25}],
    "no_head_lr": [{"name": "warm", "mode": "none", "epochs": 1}, {"name": "top", "mode": "head+1", "epochs": 2, "backbone_lr": 1e-5}],
    "backbone_lr_wins": [{"mode": "none", "epochs": 2, "backbone_lr": 3e-6, "backbone_lr_scale": 0.5, "lr": 7e-4}],
}
BASE_LR = 1e-3
EPOCHS = 30
MONITOR_NAMES = [["val_loss", None], ["loss", None], ["loss_total", None], ["val_auprc", None], ["val_f1", "auto"], ["val_auprc", "min"],
                 ["val_loss", "MAX"], [None, None], ["", ""], ["VAL_LOSS", "Auto"], ["lossy_metric", None], ["val_loss_x", None]]
NAN = float("nan")
STOP_SERIES = {
    # a NaN, a tie inside min_delta, a stop that min_epochs holds back
    "val_loss": {"mode": None, "patience": 2, "min_delta": 5e-5, "min_epochs": 6,
                 "values": [0.70, 0.69, 0.68998, NAN, 0.70, 0.71, 0.65, 0.66, 0.67, 0.68]},
    "val_auprc": {"mode": None, "patience": 3, "min_delta": 1e-3, "min_epochs": 3,
                  "values": [NAN, 0.50, 0.5005, 0.52, 0.5205, NAN, 0.51, 0.519, 0.60]},
    "val_loss_first_nan_then_early": {"mode": "min", "patience": 1, "min_delta": 0.0, "min_epochs": 4,
                                      "values": [NAN, NAN, 1.0, 1.0, 1.0, 0.9]},
}
PLATEAU_SERIES = [0.5, 0.6, 0.6, 0.6, 0.6, 0.61, 0.61, 0.61, 0.61, 0.61, 0.61, 0.7] + [0.7] * 18


class Toy(nn.Module):
    """What configure_finetune_parameters touches: lin_head, blocks, other backbone parameters, `.frozen`."""

    def __init__(self):
        super().__init__()
        self.patch = nn.Linear(3, 4)
        self.blocks = nn.ModuleList([nn.Linear(4, 4) for _ in range(3)])
        self.norm = nn.LayerNorm(4)
        self.lin_head = nn.Linear(4, 2)
        self.frozen = False


def toy_optimizer(model, lr):
    head = list(model.lin_head.parameters())
    ids = {id(p) for p in head}
    return torch.optim.AdamW([{"params": head, "lr": lr, "name": "head"},
                              {"params": [p for p in model.parameters() if id(p) not in ids], "lr": lr, "name": "backbone"}],
                             lr=lr, weight_decay=0.05)


def jsonable(x):
    if isinstance(x, float) and x != x:
        return "nan"
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, dict):
        return {k: jsonable(v) for k, v in x.items()}
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    sys.path.insert(0, os.path.join(args.reference, "src"))
    from ssl4polyp.classification import train_classification as tc

    specs = {}
    for budget in ("s50", "s100", "s200", "s500"):
        with open(os.path.join(args.reference, "config", "exp", "exp5c", "budgets", budget + ".yaml")) as fh:
            specs["exp5c_" + budget] = yaml.safe_load(fh)["protocol"]["finetune_schedule"]
    specs.update(EDGE_SPECS)

    out = {"base_lr": BASE_LR, "epochs": EPOCHS, "specs": specs, "stages": {}, "traces": [], "monitor_modes": [], "early_stop": {}}
    for name, spec in specs.items():
        stages = tc._materialize_finetune_schedule(tc._sanitize_finetune_schedule_config(spec, default_mode="full"), base_lr=BASE_LR)
        out["stages"][name] = [dataclasses.asdict(s) for s in stages]

    for spec_name in ("exp5c_s50", "exp5c_s500", "no_head_lr"):
        for sched, kw in (("cosine", {"warmup_epochs": 6}), ("none", {}), ("plateau", {"min_lr": 1e-6, "scheduler_patience": 2,
                                                                                      "scheduler_factor": 0.5})):
            torch.manual_seed(0)
            model = Toy()
            stages = tc._materialize_finetune_schedule(tc._sanitize_finetune_schedule_config(specs[spec_name], default_mode="full"),
                                                       base_lr=BASE_LR)
            runtime = tc.FinetuneScheduleRuntime(stages)
            # the order of the reference's set-up (tc.py:5740-5768, 5975, 5984-5987): the first stage's mode, the optimizer, the
            # scheduler, then the first stage applied
            tc.configure_finetune_parameters(model, runtime.stage_for_epoch(1).mode)
            opt = toy_optimizer(model, BASE_LR)
            scheduler = tc.create_scheduler(opt, types.SimpleNamespace(scheduler=sched, epochs=EPOCHS, **kw))
            runtime.apply_if_needed(model, opt, 1, rank=1)
            rows = []
            for epoch in range(1, EPOCHS + 1):
                stage = runtime.apply_if_needed(model, opt, epoch, rank=1)   # tc.py:6620-6623
                rows.append({"epoch": epoch, "stage": stage.index, "mode": stage.mode, "lr_groups": [g["lr"] for g in opt.param_groups],
                             "trainable": [n for n, p in model.named_parameters() if p.requires_grad], "frozen": bool(model.frozen)})
                opt.step()
                if scheduler is not None:   # tc.py:6818-6833
                    if sched == "plateau":
                        scheduler.step(PLATEAU_SERIES[epoch - 1])
                    else:
                        scheduler.step()
            out["traces"].append({"spec": spec_name, "scheduler": sched, "args": kw, "monitor": PLATEAU_SERIES if sched == "plateau" else None,
                                  "rows": rows})

    for monitor, mode in MONITOR_NAMES:
        out["monitor_modes"].append([monitor, mode, tc._resolve_monitor_mode(monitor, mode)])

    for name, cfg in STOP_SERIES.items():
        monitor = "val_auprc" if "auprc" in name else "val_loss"
        mode = tc._resolve_monitor_mode(monitor, cfg["mode"])
        min_delta = tc._safe_min(float(cfg["min_delta"]))
        best, no_improve, rows = None, 0, []
        for i, value in enumerate(cfg["values"]):   # tc.py:6841-6846, 7182-7192, 7211-7243
            better = tc._improved(float(value), best, mode=mode, min_delta=min_delta)
            if better:
                best, no_improve = float(value), 0
            else:
                no_improve += 1
            if best is not None and best != best:
                best = None
            stop = tc._should_trigger_early_stop(no_improve, cfg["patience"], i + 1, cfg["min_epochs"])
            rows.append({"value": value, "improved": better, "best": best, "no_improve": no_improve, "stop": stop})
            if stop:
                break
        out["early_stop"][name] = dict(cfg, monitor=monitor, resolved_mode=mode, rows=rows)

    dst = os.path.join(HERE, "finetune_schedule.json")
    with open(dst, "w") as fh:
        json.dump(jsonable(out), fh, indent=1)
    print(f"wrote {dst}: {os.path.getsize(dst) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
