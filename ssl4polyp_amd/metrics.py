"""Binary test metrics and their cluster-bootstrap intervals on the device (include/polypmae.h: pm_boot_metrics).

The reference reports AUPRC, AUROC, recall, precision, F1, balanced accuracy, MCC and loss at a threshold tau, each with a 95 %
interval from a bootstrap that resamples whole clusters (cases) per label: classification/analysis/common_metrics.py
(compute_binary_metrics, build_cluster_set, sample_cluster_ids) driven 1000-2000 times per cell by the exp*_report modules.  Here
the clusters and the draws are made on the host exactly as the reference makes them (the same calls on a numpy Generator, so
replicate r is the reference's replicate r) and every replicate is evaluated by one HIP launch sequence: a replicate is a weight
per frame, nothing is gathered (DESIGN.md "Bootstrap intervals of the test metrics").  There is no host fallback.

The threshold itself is chosen on the validation scores by the reference's policies (classification/metrics/thresholds.py), here by
one launch over the same sorted order: select_threshold / threshold_record (pm_select_tau; DESIGN.md "Threshold selection on the
device").
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

METRIC_KEYS = ("count", "n_pos", "n_neg", "prevalence", "tp", "fp", "tn", "fn", "auprc", "auroc", "recall", "precision", "f1",
               "balanced_accuracy", "mcc", "loss")
REPORTED_KEYS = METRIC_KEYS[8:]   # the reference's default metric set (common_metrics.py:30-39)
SCAN_TILE = 1024                  # sorted frames per scan tile of pm_boot_metrics (pm_metrics.hip kTile)
MAX_REPLICATES_PER_CALL = 4096    # pm_boot_metrics' limit on R
CHUNK = 512                       # replicates per call of bootstrap_binary_metrics (bounds the workspace: R * C counters)


class ClusterSet:
    """Clusters of one evaluation set: `cluster` int32 [N] numbers the positives' clusters first (0 .. n_pos - 1), then the
    negatives', each in order of first appearance -- ClusterSet.positives + ClusterSet.negatives of the reference."""

    def __init__(self, cluster: np.ndarray, n_pos: int, n_neg: int):
        self.cluster = np.ascontiguousarray(cluster, dtype=np.int32)
        self.n_pos, self.n_neg = int(n_pos), int(n_neg)

    @property
    def n_clusters(self) -> int:
        return self.n_pos + self.n_neg


def build_cluster_set(rows, labels, positive_key="case_id", negative_key="case_id") -> ClusterSet:
    """common_metrics.build_cluster_set over CSV rows (dicts): a positive frame's cluster is its `positive_key` value, a negative
    frame's its `negative_key` value; a frame whose key is missing or empty is a cluster of its own.  The two classes never share a
    cluster.  A key may also be a callable row -> str | None.  The value is taken as the reference takes it (`key(record) or
    <own cluster>`): it is not stripped, so a key of blanks is a key like any other, and only a false value (None, "") is missing."""
    def value(row, key):
        return (key(row) if callable(key) else row.get(key)) or None
    index = ({}, {})
    where = []
    for i, (row, label) in enumerate(zip(rows, labels)):
        pos = int(label) == 1
        key = value(row, positive_key if pos else negative_key)
        table = index[0 if pos else 1]
        where.append((pos, table.setdefault(("frame", i) if key is None else ("key", key), len(table))))
    n_pos, n_neg = len(index[0]), len(index[1])
    return ClusterSet(np.array([c if pos else n_pos + c for pos, c in where], dtype=np.int32), n_pos, n_neg)


def draw_cluster_samples(cluster_sets, rng: np.random.Generator, R: int):
    """R replicates of common_metrics.sample_cluster_ids for every set, as cluster indices: int32 [R, n_clusters] per set.  The
    generator is consumed as the reports consume it: the replicate is the outer loop, the sets the inner one, and per set
    `rng.integers(0, n_pos, n_pos)` then the same over the negatives (an empty class draws nothing)."""
    single = isinstance(cluster_sets, ClusterSet)
    sets = [cluster_sets] if single else list(cluster_sets)
    out = [np.empty((R, cs.n_clusters), dtype=np.int32) for cs in sets]
    for r in range(R):
        for cs, d in zip(sets, out):
            if cs.n_pos:
                d[r, :cs.n_pos] = rng.integers(0, cs.n_pos, size=cs.n_pos)
            if cs.n_neg:
                d[r, cs.n_pos:] = cs.n_pos + rng.integers(0, cs.n_neg, size=cs.n_neg)
    return out[0] if single else out


def _workspace_bytes(N, M, R, K, C) -> int:
    need = ctypes.c_size_t(0)
    _lib.check(_lib.load().pm_boot_metrics_workspace(N, M, R, K, C, ctypes.byref(need)), "pm_boot_metrics_workspace")
    return need.value


def bootstrap_binary_metrics(probs, labels, tau, cluster, draws, n_clusters=None, chunk=CHUNK, device=None) -> torch.Tensor:
    """The 16 values of compute_binary_metrics (METRIC_KEYS order) for every replicate and run: f64 [R, M, 16] on the device.

    probs [M, N] (or [N]): probabilities of the positive class, M runs over the same N frames (they share the draws); labels [N]
    0 / 1; tau: a float or one per run; cluster int [N]; draws int [R, K] cluster indices, -1 = padding.  Tensors on the device
    are used where they are; anything else is uploaded.  A float tau is compared as the f64 it is (the reference compares against
    float(tau)).  The replicates run `chunk` at a time against one workspace, whose sorted view the first call builds and the later
    ones reuse; the result does not depend on the chunk size, bit for bit."""
    if device is None:
        device = probs.device if isinstance(probs, torch.Tensor) and probs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = lambda x, dt: torch.as_tensor(x).to(device=device, dtype=dt).contiguous()
    score = dev(probs, torch.float64)
    if score.ndim == 1:
        score = score[None]
    M, N = score.shape
    label = dev(labels, torch.uint8)
    cl = dev(cluster, torch.int32)
    dr = dev(draws, torch.int32)
    if dr.ndim != 2 or label.shape != (N,) or cl.shape != (N,):
        raise ValueError(f"shapes: probs {tuple(score.shape)}, labels {tuple(label.shape)}, cluster {tuple(cl.shape)}, draws {tuple(dr.shape)}")
    R, K = dr.shape
    C = int(n_clusters) if n_clusters is not None else int(np.asarray(cluster.cpu() if isinstance(cluster, torch.Tensor) else cluster).max()) + 1
    tau_d = dev(torch.full((M,), float(tau), dtype=torch.float64) if np.ndim(tau) == 0 else tau, torch.float64)
    if tau_d.shape != (M,):
        raise ValueError(f"tau: one value or one per run ({M}), got {tuple(tau_d.shape)}")
    order = torch.sort(score, dim=1, descending=True, stable=True).indices.to(torch.int32).contiguous()
    chunk = max(1, min(int(chunk), MAX_REPLICATES_PER_CALL, max(R, 1)))
    ws = torch.empty(_workspace_bytes(N, M, chunk, K, C), dtype=torch.uint8, device=device)
    out = torch.empty((R, M, len(METRIC_KEYS)), dtype=torch.float64, device=device)
    lib = _lib.load()
    stream = torch.cuda.current_stream(device).cuda_stream
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        _lib.check(lib.pm_boot_metrics(score.data_ptr(), order.data_ptr(), label.data_ptr(), cl.data_ptr(), dr[r0:].data_ptr(),
                                       tau_d.data_ptr(), out[r0:].data_ptr(), N, M, n, K, C, int(r0 > 0), ws.data_ptr(), ws.numel(),
                                       stream), "pm_boot_metrics")
    return out


def binary_metrics(probs, labels, tau, device=None) -> dict:
    """One evaluation: compute_binary_metrics(probs, labels, tau) as a dict in METRIC_KEYS order (R = 1, every frame once)."""
    n = int(torch.as_tensor(labels).numel())
    if n == 0:   # common_metrics.py:112-125
        return {k: (0.0 if k in ("count", "n_pos", "n_neg", "tp", "fp", "tn", "fn") else float("nan")) for k in METRIC_KEYS}
    out = bootstrap_binary_metrics(probs, labels, tau, np.zeros(n, dtype=np.int32), np.zeros((1, 1), dtype=np.int32), n_clusters=1,
                                   device=device)
    return dict(zip(METRIC_KEYS, out[0, 0].tolist()))


TAU_KEYS = ("tau", "n_candidates", "degenerate", "objective", "tp", "fp", "tn", "fn", "recall", "precision", "f1", "tpr", "fpr",
            "youden_j", "n_unique", "index")   # the columns of pm_select_tau's `out`
TAU_METRIC_KEYS = TAU_KEYS[4:14]                # thresholds._compute_metrics_for_tau
POLICIES = {"f1_opt_on_val": 0, "youden_on_val": 1, "val_opt_youden": 2, "youden": 3}   # pm_select_tau's `policy`
MAX_CANDIDATES = 200                            # thresholds._MAX_THRESHOLD_CANDIDATES


def format_threshold_key(dataset: str, split: str, policy: str) -> str:
    """thresholds.format_threshold_key: the name a threshold is kept under in a checkpoint."""
    return f"{dataset.lower()}_{split.lower()}_{policy.lower()}"


def select_threshold(probs, labels, policy, previous_tau=None, return_candidates=False, device=None):
    """The decision threshold of every run under one of the reference's policies (POLICIES; classification/metrics/thresholds.py
    compute_policy_threshold and compute_youden_j_threshold): f64 [M, 16] on the device in TAU_KEYS order, by one launch of
    pm_select_tau after the sort.  Nothing is read back: `[:, 0]` goes to bootstrap_binary_metrics(tau=...) as it is.

    probs [M, N] (or [N]): P(class 1) in [0, 1] as positive_probs returns it -- values outside [0, 1] or NaN are outside the
    contract; labels [N] 0 / 1; previous_tau: None, a float or one per run (NaN = none), used only when the labels hold one class.
    With return_candidates the result is (rows, candidates f64 [M, 200], NaN beyond the list).  A run with one class only has
    degenerate = 1; for `youden` its tau is NaN and threshold_record raises the reference's error."""
    name = str(policy).strip().lower()
    if name not in POLICIES:
        raise ValueError(f"Unsupported threshold policy '{policy}' (one of {', '.join(POLICIES)})")
    if device is None:
        device = probs.device if isinstance(probs, torch.Tensor) and probs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = lambda x, dt: torch.as_tensor(x).to(device=device, dtype=dt).contiguous()
    score = dev(probs, torch.float64)
    if score.ndim == 1:
        score = score[None]
    M, N = score.shape
    label = dev(labels, torch.uint8)
    if label.shape != (N,):
        raise ValueError(f"shapes: probs {tuple(score.shape)}, labels {tuple(label.shape)}")
    if previous_tau is None:
        prev = torch.full((M,), float("nan"), dtype=torch.float64, device=device)
    else:
        prev = dev(torch.full((M,), float(previous_tau), dtype=torch.float64) if np.ndim(previous_tau) == 0 else previous_tau, torch.float64)
    if prev.shape != (M,):
        raise ValueError(f"previous_tau: one value or one per run ({M}), got {tuple(prev.shape)}")
    order = torch.sort(score, dim=1, descending=True, stable=True).indices.to(torch.int32).contiguous()
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    _lib.check(lib.pm_select_tau_workspace(N, M, ctypes.byref(need)), "pm_select_tau_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=device)
    out = torch.empty((M, len(TAU_KEYS)), dtype=torch.float64, device=device)
    cand = torch.empty((M, MAX_CANDIDATES), dtype=torch.float64, device=device) if return_candidates else None
    _lib.check(lib.pm_select_tau(score.data_ptr(), order.data_ptr(), label.data_ptr(), prev.data_ptr(), POLICIES[name], out.data_ptr(),
                                 cand.data_ptr() if return_candidates else None, N, M, ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(device).cuda_stream), "pm_select_tau")
    return (out, cand) if return_candidates else out


def threshold_record(row, policy, split_name, epoch, candidates=None) -> dict:
    """One row of select_threshold as the reference's record (thresholds._build_policy_record, :275-296, plus `metrics` =
    _compute_metrics_for_tau): policy, tau, split, n_candidates, tiebreakers, epoch, degenerate_val, notes, metrics.  With
    `candidates` (that run's row of the candidate tensor) the list is added under `candidates`.  This reads the row back."""
    name = str(policy).strip().lower()
    if name not in POLICIES:
        raise ValueError(f"Unsupported threshold policy '{policy}'")
    v = dict(zip(TAU_KEYS, (row.detach().cpu() if isinstance(row, torch.Tensor) else np.asarray(row)).tolist()))
    degenerate = bool(v["degenerate"])
    if degenerate and name == "youden":
        raise ValueError("Youden's J threshold requires both positive and negative samples")
    notes = {}
    if degenerate:   # thresholds.py:326-332; the row's index says which: -2 previous_tau carried forward, -1 the default
        notes = {"carried_forward": True} if v["index"] == -2.0 else {"default_tau": 0.5}
    record = {"policy": name, "tau": float(v["tau"]), "split": split_name, "n_candidates": int(v["n_candidates"]),
              "tiebreakers": ["higher_recall", "lower_tau"], "epoch": int(epoch), "degenerate_val": degenerate, "notes": notes,
              "metrics": {k: float(v[k]) for k in TAU_METRIC_KEYS}}
    if candidates is not None:
        c = np.asarray(candidates.detach().cpu() if isinstance(candidates, torch.Tensor) else candidates, dtype=np.float64)
        record["candidates"] = c[~np.isnan(c)].tolist()
    return record


def positive_probs(logits: torch.Tensor) -> torch.Tensor:
    """P(class 1) of two-class logits [N, 2] in f64 (softmax over the pair = sigmoid of the difference)."""
    z = logits.to(torch.float64)
    return torch.sigmoid(z[:, 1] - z[:, 0])


def percentile_ci(samples, level: float = 0.95, baseline=None):
    """(lower, upper) of the replicates as the reports take them (exp5a_report._ci_bounds): np.percentile at (1 -+ level) / 2 over
    the finite replicates, on the host.  `samples` [R] or [R, ...] (the interval is over axis 0, per trailing entry); with `baseline`
    (same shape: a second run over the same draws) the interval is that of the paired delta samples - baseline.  A column without
    a finite replicate gives (nan, nan)."""
    a = np.asarray(samples.cpu() if isinstance(samples, torch.Tensor) else samples, dtype=np.float64)
    if baseline is not None:
        a = a - np.asarray(baseline.cpu() if isinstance(baseline, torch.Tensor) else baseline, dtype=np.float64)
    flat = a.reshape(a.shape[0], -1)
    lo, hi = np.full(flat.shape[1], np.nan), np.full(flat.shape[1], np.nan)
    for j in range(flat.shape[1]):
        v = flat[:, j][np.isfinite(flat[:, j])]
        if v.size:
            lo[j], hi[j] = np.percentile(v, (1.0 - level) / 2.0 * 100.0), np.percentile(v, (1.0 + level) / 2.0 * 100.0)
    shape = a.shape[1:]
    return (float(lo[0]), float(hi[0])) if not shape else (lo.reshape(shape), hi.reshape(shape))
