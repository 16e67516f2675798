"""Classification fine-tuning from CSV packs on the MI355X engine -- a small command over what the package already has, not a port
of the reference's train_classification.py: the split CSVs of a pack (`frame_path,label` + metadata, classification/data/packs.py)
are read by packs.read_pack_csv, the workers only decode (or, `--decode device`, only read and pack the files), and the whole
transform -- the train augmentation, the eval Resize + row perturbations -- runs on the device (packs.device_pack_loaders).

    python -m ssl4polyp_amd.main_finetune --train_csv data_packs/sun_full/train.csv --val_csv data_packs/sun_full/val.csv \\
        --test_csv data_packs/sun_full/test.csv --root sun=/data/SUN --mae_checkpoint out/ckpts/last.pth --decode device

Training is the reference's: configure_finetune_parameters(--finetune_mode), AdamW over a head and a backbone group
(tc.py:5751-5768), the per-epoch cosine factor with warm-up (tc.py:3952-3957), BCE with pos_weight = neg / pos of the train labels
(tc.py:6092-6096), evaluation on val after every epoch and on test at the end.  One JSON line per epoch goes to
<output_dir>/log.txt (train loss, lr, img/s, val loss from the returned logits).  `--metrics` adds the reference's binary metrics at
tau = 0.5 to the val and test records; `--bootstrap R` adds their 95 % cluster-bootstrap intervals (`bootstrap`, `ci_lower`,
`ci_upper`) to the test record, with or without `--metrics` (metrics.py: one device call per chunk of replicates); a value that is
not finite is logged as null.  `--threshold_policy` chooses the decision threshold as the reference does (classification/metrics/
thresholds.py; metrics.select_threshold, one device launch): f1_opt_on_val / youden_on_val / val_opt_youden / youden select tau on
the val scores after every epoch (`val_tau`, `val_threshold` = the reference's record with split `<dataset_name>/val`, with
`--metrics` also `val_metrics_at_tau`; the previous epoch's tau is carried into a one-class epoch), the checkpoint keeps it under
`thresholds` / `threshold_records[<dataset>_val_<policy>]`, and the test record reports `test_tau`, `test_metrics_at_tau` and the
bootstrap intervals at that tau; sun_val_frozen takes the tau from `--threshold_from`, such a checkpoint with exactly one
threshold.  Without the flag nothing changes: tau = 0.5 and the records and checkpoints of before.  `run(args)` returns the model
and the last val logits.  `--group_metrics morphology|perturbation` (repeatable) adds the reference's per-group blocks to the test
record at the tau in force: `test_strata` (overall / flat_plus_negs / polypoid_plus_negs from the rows' `morphology`) and
`test_perturbation_metrics` (`per_tag` in the reference's order of report, `per_case` recall / F1 / count per tag and case_id), with
`--bootstrap R` also `test_strata_ci` / `test_perturbation_ci` (`ci_lower`, `ci_upper` per group and reported metric, from the draws
of the overall interval; metrics.bootstrap_group_metrics, one device call per chunk whatever the number of groups).
`--threshold_policy f1-morph` selects tau on val as the reference's _compute_f1_morph_threshold does and falls back to `youden` where
that gives none (`val_threshold` = policy, tau, split, epoch, fallback).  `--curve_export POINTS` writes the ROC and PR curve files of
val and test under --output_dir and names them in the records (`val_curves`, `test_curves`).  Not here: sharded evaluation through
the prefetcher.

Staged fine-tuning (the reference's Exp-5C): `--finetune_schedule FILE` takes a YAML or JSON list in the shape of the reference's
`protocol.finetune_schedule` (train.materialize_finetune_schedule / FinetuneScheduleRuntime), runs the optimizer with torch's
per-parameter steps (FusedAdamW(per_parameter_steps=True)) and drives the lrs through torch's scheduler objects as the reference
does (`--scheduler cosine|plateau|none`, train.create_scheduler) -- including the reference's behaviour that LambdaLR rewrites both
group lrs from base_lrs x lambda after every epoch, so a stage's head_lr / backbone_lr hold for the first epoch of the stage only.
`--early_stop_*` stops the run as the reference's patience tracker does (train.EarlyStopping; rank 0 decides, the others follow).
Every epoch record then carries `stage`, `mode` and `lr_groups` (the lrs in force during the epoch), with early stopping also
`monitor`, `best`, `no_improve` and `stopped`; the checkpoints carry the stage index, the scheduler state and the early-stopping
counters, and `--resume CKPT` continues from them.  Without these options the records, checkpoints and bits are unchanged.
"""
from __future__ import annotations

import argparse
import json
import math
import os

import torch
import torch.distributed as dist

from . import models
from .optim import FusedAdamW, LossScaler
from .parallel import DataParallel
from .train import (FINETUNE_MODES, FinetuneScheduleRuntime, cls_cosine_lambda, configure_finetune_parameters, create_scheduler, evaluate_cls,
                    load_cls_checkpoint, save_cls_checkpoint, train_epoch_cls)


SELECTING_POLICIES = ("f1_opt_on_val", "youden_on_val", "val_opt_youden", "youden")   # metrics.POLICIES
FROZEN_POLICY = "sun_val_frozen"
MORPH_POLICY = "f1-morph"   # metrics.f1_morph_threshold: a grid search over two strata, not one of pm_select_tau's policies
GROUP_KINDS = ("morphology", "perturbation")


def get_args_parser():
    p = argparse.ArgumentParser("Classification fine-tuning from CSV packs (MI355X)", add_help=True)
    p.add_argument("--train_csv", default=None, help="train split of the pack (frame_path,label + metadata columns)")
    p.add_argument("--val_csv", default=None)
    p.add_argument("--test_csv", default=None)
    p.add_argument("--root", action="append", default=[], metavar="KEY=PATH",
                   help="roots map entry: KEY is the first component of frame_path, or a row's store_id / dataset (repeatable)")
    p.add_argument("--batch_size", default=64, type=int, help="batch size per GPU")
    p.add_argument("--epochs", default=50, type=int)
    p.add_argument("--lr", default=1e-3, type=float)
    p.add_argument("--weight_decay", default=0.05, type=float)
    p.add_argument("--warmup_epochs", default=0, type=int)
    p.add_argument("--finetune_mode", default="full", choices=sorted(FINETUNE_MODES))
    p.add_argument("--mae_checkpoint", default=None, help="MAE pre-training checkpoint for the backbone (default: random init)")
    p.add_argument("--imagenet_weights", default=None, help="augreg ViT-B/16 .npz on local disk: the ImageNet-initialised ViT instead")
    p.add_argument("--random_vit", action="store_true", help="the randomly initialised timm-style ViT instead of the MAE encoder")
    p.add_argument("--num_classes", default=2, type=int)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--decode", default="host", choices=["host", "device"],
                   help="where the frames are decoded: 'device' = the workers only read and pack the files, baseline JPEGs are "
                        "decoded on the GPU bit for bit as Pillow does (others still on the host)")
    p.add_argument("--fused_decode", action="store_true",
                   help="with --decode device: decode straight into the resized frame, no full-size RGB in between (same bytes)")
    p.add_argument("--num_workers", default=8, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--perturb_test", action="store_true", help="render the test rows' perturbations (Exp-5 packs)")
    p.add_argument("--output_dir", default="./output_dir")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--log_every", default=20, type=int)
    p.add_argument("--clip_grad", type=float, default=None, metavar="NORM",
                   help="clip the gradient by global norm inside the optimizer step (default: no clipping); the log records then "
                        "carry grad_norm_groups, grad_norm and clip_coef")
    p.add_argument("--group_grad_norms", action="store_true", help="log one gradient norm per param group")
    p.add_argument("--metrics", action="store_true",
                   help="log the binary metrics of val and test at tau = 0.5 (AUPRC, AUROC, recall, precision, F1, balanced accuracy, MCC, loss)")
    p.add_argument("--bootstrap", default=0, type=int, metavar="R",
                   help="R > 0: 95 %% intervals of the test metrics from R cluster-bootstrap replicates (clusters: case_id per label)")
    p.add_argument("--bootstrap_seed", default=12345, type=int)
    p.add_argument("--threshold_policy", default="none", choices=["none", *SELECTING_POLICIES, MORPH_POLICY, FROZEN_POLICY],
                   help="how the decision threshold tau is chosen (the reference's threshold_policy): on the val split after every "
                        "epoch, on the device; f1-morph needs a `morphology` column and falls back to youden; sun_val_frozen reuses the "
                        "tau of --threshold_from")
    p.add_argument("--dataset_name", default="dataset", help="names the val split in the threshold record and its checkpoint key")
    p.add_argument("--threshold_from", default=None, metavar="CKPT",
                   help="with --threshold_policy sun_val_frozen: a checkpoint of this command that holds exactly one threshold")
    p.add_argument("--group_metrics", action="append", default=[], choices=list(GROUP_KINDS),
                   help="per-group test metrics at the tau in force (repeatable): morphology = the strata overall / flat_plus_negs / "
                        "polypoid_plus_negs, perturbation = per perturbation tag and per (tag, case); with --bootstrap their intervals")
    p.add_argument("--curve_export", default=0, type=int, metavar="POINTS",
                   help="POINTS >= 2: write <output_dir>/curves_<split>_roc_curve.csv and _pr_curve.csv for val and test over that many thresholds")
    p.add_argument("--finetune_schedule", default=None, metavar="FILE",
                   help="staged fine-tuning: a YAML or JSON list in the shape of the reference's protocol.finetune_schedule (per stage: "
                        "name, mode, epochs, lr, head_lr, backbone_lr, backbone_lr_scale); replaces --finetune_mode and turns the "
                        "optimizer's per-parameter steps on")
    p.add_argument("--scheduler", default="cosine", choices=["cosine", "plateau", "none"],
                   help="the epoch scheduler (the reference's create_scheduler): cosine = the factor with warm-up of before")
    p.add_argument("--min_lr", default=1e-6, type=float, help="--scheduler plateau: lower bound of the lr")
    p.add_argument("--scheduler_patience", default=2, type=int, help="--scheduler plateau")
    p.add_argument("--scheduler_factor", default=0.5, type=float, help="--scheduler plateau")
    p.add_argument("--early_stop_monitor", default="val_loss", help="val_loss, or val_<key> for a key of metrics.METRIC_KEYS")
    p.add_argument("--early_stop_mode", default=None, choices=["min", "max", "auto"], help="default: min for a loss, else max")
    p.add_argument("--early_stop_patience", default=0, type=int, help="epochs without improvement before the run stops (0 = off)")
    p.add_argument("--early_stop_min_delta", default=0.0, type=float)
    p.add_argument("--early_stop_min_epochs", default=0, type=int)
    p.add_argument("--resume", default=None, metavar="CKPT",
                   help="continue from a checkpoint of this command (e.g. <output_dir>/ckpts/last.pth): model, optimizer, loss scaler, "
                        "scheduler, the schedule's stage and the early-stopping counters")
    return p


def load_finetune_schedule(args) -> list:
    """The stages of --finetune_schedule (train.materialize_finetune_schedule over the file's list, base lr = --lr), [] without the
    option.  The option replaces --finetune_mode: giving both is refused."""
    if not args.finetune_schedule:
        return []
    if args.finetune_mode != "full":
        raise SystemExit("--finetune_schedule sets the mode per stage: it cannot be combined with --finetune_mode")
    if not os.path.exists(args.finetune_schedule):
        raise SystemExit(f"--finetune_schedule {args.finetune_schedule}: no such file")
    with open(args.finetune_schedule) as fh:
        text = fh.read()
    if str(args.finetune_schedule).lower().endswith(".json"):
        spec = json.loads(text)
    else:
        import yaml
        spec = yaml.safe_load(text)
    if isinstance(spec, dict):   # a whole budget file: protocol.finetune_schedule, as in config/exp/exp5c/budgets/*.yaml
        spec = (spec.get("protocol") or {}).get("finetune_schedule", spec.get("finetune_schedule"))
    from .train import materialize_finetune_schedule
    try:
        stages = materialize_finetune_schedule(spec, float(args.lr))
    except (TypeError, ValueError) as e:
        raise SystemExit(f"--finetune_schedule {args.finetune_schedule}: {e}")
    if not stages:
        raise SystemExit(f"--finetune_schedule {args.finetune_schedule}: no stages")
    return stages


def early_stopping(args):
    """train.EarlyStopping of the --early_stop_* options, None when --early_stop_patience is 0."""
    if int(args.early_stop_patience or 0) <= 0:
        return None
    from . import metrics as MX
    from .train import EarlyStopping
    monitor = str(args.early_stop_monitor or "val_loss")
    if monitor != "val_loss" and not (monitor.startswith("val_") and monitor[4:] in MX.METRIC_KEYS):
        raise SystemExit(f"--early_stop_monitor {monitor}: expected val_loss or val_<key> with a key of {list(MX.METRIC_KEYS)}")
    if not args.val_csv:
        raise SystemExit("--early_stop_patience watches the val split: it needs --val_csv")
    if monitor != "val_loss" and args.num_classes != 2:
        raise SystemExit(f"--early_stop_monitor {monitor} is a binary metric: it needs --num_classes 2")
    return EarlyStopping(monitor, args.early_stop_mode, args.early_stop_patience, args.early_stop_min_delta, args.early_stop_min_epochs)


def monitor_value(name: str, record: dict, val_logits, val_targets, device) -> float:
    """What early stopping and the plateau scheduler watch after an epoch: the record's val_loss, or the val metric `name[4:]` at
    tau = 0.5 from the existing device metrics; 0.0 without a val split (tc.py:6807-6810)."""
    if val_targets is None or val_logits is None:
        return 0.0
    if name == "val_loss":
        return float(record["val_loss"])
    from . import metrics as MX
    return float(MX.binary_metrics(MX.positive_probs(val_logits.to(device)), val_targets, METRICS_TAU, device=device)[name[4:]])


def broadcast_value(value: float, device, world: int) -> float:
    """Rank 0's value on every rank (tc.py:6823-6829, 7211-7229)."""
    if world <= 1:
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.broadcast(t, src=0)
    return float(t.item())


def parse_roots(specs) -> dict:
    roots = {}
    for spec in specs or []:
        key, sep, path = str(spec).partition("=")
        if not sep or not key or not path:
            raise SystemExit(f"--root takes KEY=PATH (got {spec!r})")
        roots[key] = path
    return roots


def build_model(args):
    if args.imagenet_weights or args.random_vit:
        return models.get_ImageNet_or_random_ViT(True, args.num_classes, False, None, args.imagenet_weights or False,
                                                 precision=args.precision)
    return models.get_MAE_backbone(args.mae_checkpoint, True, args.num_classes, False, None, precision=args.precision)


def host_loss(logits: torch.Tensor, targets: torch.Tensor, pos_weight) -> float:
    """The fine-tune loss (tc.py:3347-3374) of a finished pass, on the host from the returned logits."""
    import torch.nn.functional as F
    if logits.numel() == 0:
        return float("nan")
    if logits.shape[1] == 2:
        pw = None if pos_weight is None else torch.tensor(float(pos_weight))
        return F.binary_cross_entropy_with_logits(logits[:, 1] - logits[:, 0], targets.float(), pos_weight=pw).item()
    return F.cross_entropy(logits, targets.long()).item()


METRICS_TAU = 0.5


def strict(values) -> list:
    """The values as a list with None where one is not finite: json.dumps would write a bare NaN, which is not JSON."""
    return [v if math.isfinite(v) else None for v in values]


def metric_records(prefix: str, logits: torch.Tensor, targets: torch.Tensor, rows, device, metrics: bool = True, bootstrap: int = 0,
                   seed: int = 0, tau=None) -> dict:
    """The entries `--metrics` / `--bootstrap` add to a record.  metrics: <prefix>_metrics, the 16 values of the reference's
    compute_binary_metrics at tau = 0.5.  bootstrap > 0: `bootstrap`, ci_lower / ci_upper per reported metric from that many
    replicates that resample whole cases per label (rows without a case_id are clusters of their own).  A value that is not finite
    (AUROC of a split without positives or without negatives) is logged as null, so that every line stays strict JSON.
    tau (f64 [1] on the device, the selected threshold): <prefix>_tau, with metrics also <prefix>_metrics_at_tau, and the intervals
    are taken at that tau; it goes to the device calls as the tensor it is."""
    import numpy as np
    from . import metrics as MX
    probs = MX.positive_probs(logits.to(device))
    out = {}
    if metrics:
        values = MX.binary_metrics(probs, targets, METRICS_TAU, device=device)
        out[f"{prefix}_metrics"] = dict(zip(values, strict(values.values())))
    if tau is not None:
        out[f"{prefix}_tau"] = float(tau[0])
        if metrics:
            values = MX.binary_metrics(probs, targets, tau, device=device)
            out[f"{prefix}_metrics_at_tau"] = dict(zip(values, strict(values.values())))
    if bootstrap > 0 and logits.shape[0] > 0:
        clusters = MX.build_cluster_set(rows, targets.tolist())
        draws = MX.draw_cluster_samples(clusters, np.random.default_rng(seed), bootstrap)
        reps = MX.bootstrap_binary_metrics(probs, targets, METRICS_TAU if tau is None else tau, clusters.cluster, draws,
                                           n_clusters=clusters.n_clusters,
                                           device=device)[:, 0, len(MX.METRIC_KEYS) - len(MX.REPORTED_KEYS):]
        lo, hi = MX.percentile_ci(reps, 0.95)
        out["bootstrap"] = int(bootstrap)
        out["ci_lower"] = dict(zip(MX.REPORTED_KEYS, strict(lo.tolist())))
        out["ci_upper"] = dict(zip(MX.REPORTED_KEYS, strict(hi.tolist())))
    return out


def group_records(logits: torch.Tensor, targets: torch.Tensor, rows, device, kinds, bootstrap: int = 0, seed: int = 0, tau=None) -> dict:
    """The entries `--group_metrics` adds to the test record, at tau (f64 [1] on the device) or 0.5.  morphology: test_strata
    {stratum: the 16 values}, a stratum without a positive left out as the reference's test() leaves it out.  perturbation:
    test_perturbation_metrics {per_tag: {tag: the 16 values} in the reference's order of report, per_case: {tag: {case_id: recall,
    f1, count}} when the rows have case ids}.  bootstrap > 0: test_strata_ci / test_perturbation_ci = {ci_lower, ci_upper: {group:
    {reported metric: bound}}} from the replicates metric_records draws for the overall interval (same clusters, same seed).
    Values that are not finite are null."""
    import numpy as np
    from . import metrics as MX
    if logits.shape[0] == 0:
        return {}
    probs = MX.positive_probs(logits.to(device))
    at = METRICS_TAU if tau is None else tau
    labels = targets.tolist()
    out, sets = {}, {}
    if "morphology" in kinds:
        sets["test_strata"] = MX.morphology_groups(rows, labels)
        out["test_strata"] = {g: dict(zip(v, strict(v.values()))) for g, v in MX.group_metrics(probs, targets, at, sets["test_strata"], device=device).items()}
    if "perturbation" in kinds:
        groups = sets["test_perturbation"] = MX.perturbation_groups(rows)
        block = {"per_tag": {g: dict(zip(v, strict(v.values()))) for g, v in MX.group_metrics(probs, targets, at, groups, device=device).items()}}
        case_ids = [str(r.get("case_id") or "") for r in rows]
        if any(case_ids):
            names = sorted(set(case_ids))
            index = {c: i for i, c in enumerate(names)}
            per = {k: v.tolist() for k, v in MX.group_case_metrics(probs, targets, at, groups, [index[c] for c in case_ids], len(names), device=device).items()}
            block["per_case"] = {tag: {c: {"recall": per["recall"][g][i], "f1": per["f1"][g][i], "count": float(per["count"][g][i])}
                                       for i, c in enumerate(names) if per["count"][g][i] > 0} for g, tag in enumerate(groups.names)}
        out["test_perturbation_metrics"] = block
    if bootstrap > 0:
        clusters = MX.build_cluster_set(rows, labels)
        draws = MX.draw_cluster_samples(clusters, np.random.default_rng(seed), bootstrap)
        first = len(MX.METRIC_KEYS) - len(MX.REPORTED_KEYS)
        for key, groups in sets.items():
            reps = MX.bootstrap_group_metrics(probs, targets, at, groups, clusters.cluster, draws, n_clusters=clusters.n_clusters, device=device)
            lo, hi = MX.percentile_ci(reps[:, 0, :, first:], 0.95)
            out[key.replace("_metrics", "") + "_ci"] = {name: {g: dict(zip(MX.REPORTED_KEYS, strict(row))) for g, row in zip(groups.names, bound.tolist())}
                                                        for name, bound in (("ci_lower", lo), ("ci_upper", hi))}
    return out


def frozen_threshold(path):
    """(tau, key, record) of the one threshold a checkpoint of this command holds (`thresholds` / `threshold_records`, written by a
    run with a selecting --threshold_policy): what `--threshold_policy sun_val_frozen --threshold_from` reuses."""
    if not path:
        raise SystemExit("--threshold_policy sun_val_frozen reuses a selected tau: it needs --threshold_from CKPT")
    if not os.path.exists(path):
        raise SystemExit(f"--threshold_from {path}: no such file")
    payload = torch.load(path, map_location="cpu", weights_only=False)
    thresholds = payload.get("thresholds") if isinstance(payload, dict) else None
    if not isinstance(thresholds, dict) or len(thresholds) != 1:
        raise SystemExit(f"--threshold_from {path}: expected a checkpoint of this command with exactly one entry under 'thresholds' "
                         f"(found {sorted(thresholds) if isinstance(thresholds, dict) else 'none'})")
    (key, tau), = thresholds.items()
    if not isinstance(tau, (int, float)) or not math.isfinite(float(tau)):
        raise SystemExit(f"--threshold_from {path}: the threshold under {key!r} is not a finite number ({tau!r})")
    record = dict((payload.get("threshold_records") or {}).get(key) or {})
    return float(tau), key, record


def run(args):
    if not (args.train_csv or args.val_csv or args.test_csv):
        raise SystemExit("no data: pass --train_csv (and --val_csv / --test_csv), each a split CSV of a pack")
    if (args.metrics or args.bootstrap > 0) and args.num_classes != 2:
        raise SystemExit("--metrics / --bootstrap report the binary metrics: they need --num_classes 2")
    if args.fused_decode and args.decode != "device":
        raise SystemExit("--fused_decode needs --decode device")
    if args.group_metrics and args.num_classes != 2:
        raise SystemExit("--group_metrics reports the binary metrics per group: it needs --num_classes 2")
    if args.curve_export and (args.curve_export < 2 or args.num_classes != 2):
        raise SystemExit("--curve_export takes at least two grid points and needs --num_classes 2")
    policy = args.threshold_policy
    selecting = policy in SELECTING_POLICIES or policy == MORPH_POLICY
    if policy != "none" and args.num_classes != 2:
        raise SystemExit("--threshold_policy chooses a binary decision threshold: it needs --num_classes 2")
    if selecting and not args.val_csv:
        raise SystemExit(f"--threshold_policy {policy} selects tau on the val split: it needs --val_csv")
    frozen = frozen_threshold(args.threshold_from) if policy == FROZEN_POLICY else None
    if policy != FROZEN_POLICY and args.threshold_from:
        raise SystemExit("--threshold_from goes with --threshold_policy sun_val_frozen")
    stages = load_finetune_schedule(args)
    stopper = early_stopping(args)
    if args.resume and not os.path.exists(args.resume):
        raise SystemExit(f"--resume {args.resume}: no such file")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    from .engine import reserve_streams
    reserve_streams(device)  # before RCCL creates its streams: one hardware queue per engine stream (engine.reserve_streams)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
    from .packs import device_pack_loaders, read_pack_csv
    roots = parse_roots(args.root)
    splits = {name: read_pack_csv(path, roots) for name, path in
              (("train", args.train_csv), ("val", args.val_csv), ("test", args.test_csv)) if path}
    loaders, sampler = device_pack_loaders(splits, device, args.batch_size, decode=args.decode, world=world, rank=rank, seed=args.seed,
                                           num_workers=args.num_workers, pin_memory=args.pin_mem,
                                           perturbation_splits=("test",) if args.perturb_test else (),
                                           fused_decode=args.fused_decode)
    torch.manual_seed(args.seed)   # the same initialisation on every rank
    model = build_model(args)
    runtime = FinetuneScheduleRuntime(stages) if stages else None
    # tc.py:5735-5740: the first stage's mode before the optimizer exists; the stage itself is applied after the scheduler (below)
    configure_finetune_parameters(model, runtime.stage_for_epoch(1).mode if runtime else args.finetune_mode)
    ddp = DataParallel(model, device)
    head = list(model.lin_head.parameters())
    head_ids = {id(p) for p in head}
    groups = [{"params": head, "name": "head"},   # tc.py:5751-5768: every parameter, frozen ones are skipped for want of a gradient
              {"params": [p for p in model.parameters() if id(p) not in head_ids], "name": "backbone"}]
    # a schedule changes the set of parameters with a gradient mid-run: torch's per-parameter steps (optim.FusedAdamW)
    opt = FusedAdamW(model, groups, lr=args.lr, betas=(0.9, 0.999), weight_decay=args.weight_decay, per_parameter_steps=bool(stages))
    opt.grad_sync = ddp.sync
    opt.grad_scale = 1.0 / world
    scaler = LossScaler() if args.precision == "fp16" else None
    # The epoch scheduler.  Without the new options the cosine factor is written into the groups before every epoch, as before; a
    # schedule or another scheduler goes through torch's scheduler objects as the reference does (tc.py:5975), INCLUDING what
    # follows from that: LambdaLR.step() rewrites both group lrs from base_lrs x lambda after every epoch, so a stage's head_lr /
    # backbone_lr hold for the first epoch of the stage only.  `lr_groups` in every record shows the lrs in force.
    staged = runtime is not None or args.scheduler != "cosine"
    scheduler = create_scheduler(opt, args.scheduler, args.epochs, args.warmup_epochs, args.min_lr, args.scheduler_patience,
                                 args.scheduler_factor) if staged else None
    start_epoch = 0
    if args.resume:
        model._rt.ensure(device)   # the optimizer state loads into the flat storage
        resumed = load_cls_checkpoint(args.resume, model, opt, scheduler, loss_scaler=scaler)
        start_epoch = resumed.start_epoch - 1
        if resumed.best_val_perf is None:
            # load_cls_checkpoint restores optimizer, scheduler and loss scaler only beside a monitor value, as the reference does
            # (tc.py:5976-5980); a checkpoint of a run without a val split has none, and --resume must not go on with fresh state
            payload = torch.load(str(resumed.source), map_location="cpu", weights_only=False)
            if "optimizer_state_dict" not in payload:
                raise SystemExit(f"--resume {args.resume}: the checkpoint holds no optimizer state")
            opt.load_state_dict(payload["optimizer_state_dict"])
            if scheduler is not None and "scheduler_state_dict" in payload:
                scheduler.load_state_dict(payload["scheduler_state_dict"])
            if scaler is not None and payload.get("scaler_state_dict"):
                scaler.load_state_dict(payload["scaler_state_dict"])
        if runtime is not None:
            runtime.restore(model, resumed.finetune_stage_index)
        if stopper is not None and resumed.early_stop_state:
            stopper.load_state_dict(resumed.early_stop_state)
    elif runtime is not None:
        runtime.apply_if_needed(model, opt, 1, printer=print if rank == 0 else None)   # tc.py:5984-5987
    pos_weight = pos_weight_host = None
    if "train" in splits and args.num_classes == 2:
        labels = splits["train"][1]
        pos = sum(1 for v in labels if v == 1)
        pos_weight_host = (len(labels) - pos) / pos if pos > 0 else 1.0   # tc.py:6092-6096
        pos_weight = torch.tensor(pos_weight_host, dtype=torch.float32, device=device)
    log_path = os.path.join(args.output_dir, "log.txt")
    val_logits = None
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)

    def log(record):
        if rank == 0:
            with open(log_path, "a") as f:
                f.write(json.dumps(record) + "\n")

    tau_dev = None if frozen is None else torch.tensor([frozen[0]], dtype=torch.float64, device=device)   # f64 [1]: the tau in force
    extra = None

    def select(record, epoch):
        """tau of this epoch's val scores (every rank holds all of them): val_tau / val_threshold into the record, the checkpoint's
        `thresholds` / `threshold_records`; the tau stays on the device and is the next epoch's previous_tau."""
        nonlocal tau_dev, extra
        from . import metrics as MX
        probs = MX.positive_probs(val_logits.to(device))
        found = MX.f1_morph_threshold(probs, val_targets, [r.get("morphology") for r in splits["val"][2]], device=device) \
            if policy == MORPH_POLICY else None
        if found is not None:
            rec = {"policy": policy, "tau": found, "split": f"{args.dataset_name}/val", "epoch": int(epoch), "fallback": None}
            tau_dev = torch.tensor([found], dtype=torch.float64, device=device)
        else:   # a selecting policy, or f1-morph without both kinds of positives: the reference then takes Youden's J (tc.py:7281-7285)
            by = "youden" if policy == MORPH_POLICY else policy
            row = MX.select_threshold(probs, val_targets, by, previous_tau=tau_dev, device=device)
            try:
                rec = MX.threshold_record(row[0], by, f"{args.dataset_name}/val", epoch)
            except ValueError as e:
                raise SystemExit(f"--threshold_policy {policy} on {args.val_csv}: {e}")
            if policy == MORPH_POLICY:
                rec = {"policy": policy, "tau": rec["tau"], "split": rec["split"], "epoch": rec["epoch"], "fallback": by}
            tau_dev = row[:, 0].contiguous()
        key = MX.format_threshold_key(args.dataset_name, "val", policy)
        extra = {"thresholds": {key: rec["tau"]}, "threshold_records": {key: rec}}
        record["val_threshold"] = rec
        if rank == 0:
            record.update(metric_records("val", val_logits, val_targets, splits["val"][2], device, args.metrics, tau=tau_dev))

    def curves(record, split, logits, targets):
        if args.curve_export and rank == 0 and logits.shape[0] > 0:
            from . import metrics as MX
            record[f"{split}_curves"] = MX.export_curves(os.path.join(args.output_dir, "curves"), split, MX.positive_probs(logits.to(device)),
                                                         targets, args.curve_export, device=device)

    if "train" in loaders:
        for epoch in range(start_epoch, args.epochs):
            if isinstance(sampler, torch.utils.data.DistributedSampler):
                sampler.set_epoch(epoch)
            stage = None
            if not staged:
                factor = cls_cosine_lambda(epoch, args.warmup_epochs, args.epochs)
                for g in opt.param_groups:
                    g["lr"] = args.lr * factor
            elif runtime is not None:   # tc.py:6620-6623: the reference's epochs are 1-based
                stage = runtime.apply_if_needed(model, opt, epoch + 1, printer=print if rank == 0 else None)
            lr_groups = [float(g["lr"]) for g in opt.param_groups]   # the lrs in force during this epoch
            stats = train_epoch_cls(ddp, loaders["train"], opt, device, pos_weight=pos_weight, log_every=args.log_every,
                                    printer=(lambda r: print(f"epoch {epoch} {json.dumps(r)}", flush=True)) if rank == 0 else None,
                                    loss_scaler=scaler, clip_grad=args.clip_grad, group_grad_norms=args.group_grad_norms)
            record = {"epoch": epoch, "train_loss": stats.loss, "lr": stats.lr, "samples_per_sec": stats.samples_per_sec}
            if staged or stopper is not None:
                record.update(stage=stage.index if stage is not None else None,
                              mode=stage.mode if stage is not None else args.finetune_mode, lr_groups=lr_groups)
            if "val" in loaders:
                val_logits, val_targets, _ = evaluate_cls(model, loaders["val"], device, shard=False, return_probs=True)
                record["val_loss"] = host_loss(val_logits, val_targets, pos_weight_host)
                if selecting:
                    select(record, epoch + 1)   # the record's epoch is the checkpoint's
                elif args.metrics and rank == 0:
                    record.update(metric_records("val", val_logits, val_targets, splits["val"][2], device))
                curves(record, "val", val_logits, val_targets)
            monitor = None
            if stopper is not None or args.scheduler == "plateau":
                monitor = monitor_value(args.early_stop_monitor or "val_loss", record, val_logits, val_targets if "val" in loaders else None,
                                        device)
            if scheduler is not None and stats.steps > 0:   # tc.py:6816-6833
                if args.scheduler == "plateau":
                    scheduler.step(broadcast_value(monitor, device, world))
                else:
                    scheduler.step()
            stop = False
            state = {}
            if stopper is not None:   # tc.py:6840-6846, 7182-7192, 7211-7243: rank 0 decides, every rank follows
                stop = stopper.update(monitor, epoch + 1)
                stop = bool(broadcast_value(1.0 if stop else 0.0, device, world))
                record.update(monitor=None if not math.isfinite(monitor) else monitor, best=stopper.best, no_improve=stopper.no_improve,
                              stopped=stop)
                state["early_stop_state"] = stopper.state_dict()
            if staged or stopper is not None:
                state["finetune_stage_index"] = runtime.state_dict()["stage_index"] if runtime is not None else None
                state["monitor_value"] = record.get("val_loss", stats.loss)   # load_cls_checkpoint restores the optimizer with it
            log(record)
            save_cls_checkpoint(os.path.join(args.output_dir, "ckpts", f"finetune_e{epoch + 1}.pth"), epoch + 1, model, opt,
                                scheduler=scheduler, loss=record.get("val_loss", stats.loss),
                                extra={**(extra or {}), **state} if state else extra,
                                pointer=os.path.join(args.output_dir, "ckpts", "last.pth"), loss_scaler=scaler)
            if stop:
                if rank == 0:
                    print("Early stopping triggered after reaching patience limit.", flush=True)
                break
    elif "val" in loaders:
        val_logits, val_targets, _ = evaluate_cls(model, loaders["val"], device, shard=False, return_probs=True)
        record = {"val_loss": host_loss(val_logits, val_targets, pos_weight_host)}
        if selecting:
            select(record, 0)
        elif args.metrics and rank == 0:
            record.update(metric_records("val", val_logits, val_targets, splits["val"][2], device))
        curves(record, "val", val_logits, val_targets)
        log(record)
    if "test" in loaders:
        test_logits, test_targets, _ = evaluate_cls(model, loaders["test"], device, shard=False, return_probs=True)
        record = {"test_loss": host_loss(test_logits, test_targets, pos_weight_host), "test_samples": int(test_logits.shape[0])}
        if (args.metrics or args.bootstrap > 0 or tau_dev is not None) and rank == 0:
            record.update(metric_records("test", test_logits, test_targets, splits["test"][2], device, args.metrics, args.bootstrap,
                                         args.bootstrap_seed, tau=tau_dev))
            if frozen is not None:   # where the tau comes from
                record["test_threshold"] = {"policy": FROZEN_POLICY, "tau": frozen[0], "source_key": frozen[1],
                                            "source_policy": frozen[2].get("policy"), "source_split": frozen[2].get("split"),
                                            "source_checkpoint": str(args.threshold_from)}
        if args.group_metrics and rank == 0:
            record.update(group_records(test_logits, test_targets, splits["test"][2], device, args.group_metrics, args.bootstrap,
                                        args.bootstrap_seed, tau=tau_dev))
        curves(record, "test", test_logits, test_targets)
        log(record)
    if world > 1:
        dist.destroy_process_group()
    return model, val_logits


if __name__ == "__main__":
    run(get_args_parser().parse_args())
