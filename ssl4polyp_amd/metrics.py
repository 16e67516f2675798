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

The reference's test() reports per group -- per perturbation tag and (tag, case), per morphology stratum -- and selects the
`f1-morph` threshold from two strata.  Here a group is a segment of an entry list (GroupSet; morphology_groups, perturbation_groups)
and every group's replicates come from one launch sequence over the segments (bootstrap_group_metrics, group_metrics;
pm_group_metrics), bit for bit what bootstrap_binary_metrics gives on the group's frames alone; the per-case counts, the threshold
grid (f1_morph_threshold, curve_rows / export_curves) are integer-exact torch plumbing (DESIGN.md "Per-group test metrics").
"""
from __future__ import annotations

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
    ws = torch.empty(_lib.workspace_bytes("pm_boot_metrics_workspace", N, M, chunk, K, C), dtype=torch.uint8, device=device)
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
    ws = torch.empty(_lib.workspace_bytes("pm_select_tau_workspace", N, M), dtype=torch.uint8, device=device)
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


# ---- per-group metrics: perturbation tags, morphology strata (pm_group_metrics; DESIGN.md "Per-group test metrics") -------------

MAX_GROUP_ENTRIES = 1 << 22       # pm_group_metrics' limit on E
MAX_GROUPS = 1 << 16              # ... and on G
CLEAN_TAG, ALL_PERTURBED = "clean", "ALL-perturbed"
STRATA = ("overall", "flat_plus_negs", "polypoid_plus_negs")
F1_MORPH_POLICY = "f1-morph"      # not one of POLICIES: it is selected on the host from threshold_grid_counts, not by pm_select_tau
_PLACEHOLDER_WORDS = {"nan", "none", "null"}
_TAG_NUMERIC_FIELDS = ("blur_sigma", "jpeg_q", "brightness", "contrast", "bbox_area_frac")


class GroupSet:
    """G named groups of the frames of one evaluation set as segments: `entry_frame` int32 [E] holds one entry per (group, frame)
    pair, group after group, the frames of a group in ascending order; group g owns entries seg[g] .. seg[g + 1] - 1 (`seg` int32
    [G + 1]).  Groups may overlap and may be empty."""

    def __init__(self, names, entry_frame, seg):
        self.names = tuple(str(n) for n in names)
        self.entry_frame = np.ascontiguousarray(entry_frame, dtype=np.int32).reshape(-1)
        self.seg = np.ascontiguousarray(seg, dtype=np.int32).reshape(-1)
        if self.seg.shape != (len(self.names) + 1,) or self.seg[0] != 0 or self.seg[-1] != self.entry_frame.size or \
                (np.diff(self.seg) < 0).any():
            raise ValueError(f"seg: {len(self.names) + 1} non-decreasing offsets from 0 to {self.entry_frame.size}, got {self.seg.tolist()}")
        if len(set(self.names)) != len(self.names):
            raise ValueError(f"group names repeat: {self.names}")

    @classmethod
    def from_members(cls, names, members) -> "GroupSet":
        """One index list (or boolean mask over the frames) per group."""
        lists = []
        for m in members:
            m = np.asarray(m)
            lists.append(np.sort(np.flatnonzero(m) if m.dtype == np.bool_ else m.astype(np.int64).reshape(-1)))
        seg = np.concatenate([[0], np.cumsum([len(m) for m in lists])]) if lists else np.zeros(1)
        return cls(names, np.concatenate(lists) if lists else np.zeros(0), seg)

    def __len__(self) -> int:
        return len(self.names)

    @property
    def sizes(self) -> np.ndarray:
        return np.diff(self.seg)

    def frames(self, g) -> np.ndarray:
        """The frame indices of group g (an index or a name), ascending."""
        g = self.names.index(g) if isinstance(g, str) else int(g)
        return self.entry_frame[self.seg[g]:self.seg[g + 1]]

    def subset(self, which) -> "GroupSet":
        """The named (or indexed) groups alone, in the order given."""
        idx = [self.names.index(g) if isinstance(g, str) else int(g) for g in which]
        return GroupSet.from_members([self.names[g] for g in idx], [self.frames(g) for g in idx])


def _morphology_array(morphology) -> np.ndarray:
    """train_classification.py:3064: str(value).strip().lower(), None and "" -> "".  An item may be a row (its `morphology`)."""
    values = [(m.get("morphology") if hasattr(m, "get") else m) for m in morphology]
    return np.array([str(v).strip().lower() if v not in (None, "") else "" for v in values], dtype=object)


def morphology_groups(rows, labels, omit_empty: bool = True) -> GroupSet:
    """The strata of _build_morphology_strata_metrics (train_classification.py:3041-3089): `overall`, then `flat_plus_negs` = every
    negative + the positives whose morphology is flat, then `polypoid_plus_negs` alike.  rows: CSV rows (dicts with a `morphology`
    column) or the morphology values themselves.  omit_empty: a stratum without a positive is left out, as the reference's test()
    does (:3069, :3079); False keeps all three, as exp3_report.compute_strata_metrics does.  No frames: no groups."""
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    if y.size == 0:
        return GroupSet((), np.zeros(0), np.zeros(1))
    morph = _morphology_array(rows)
    if len(morph) != y.size:
        raise ValueError(f"one morphology value per frame: {len(morph)} for {y.size} labels")
    pos, neg = y == 1, y == 0
    names, members = [STRATA[0]], [np.arange(y.size)]
    for name, kind in zip(STRATA[1:], ("flat", "polypoid")):
        own = pos & (morph == kind)
        if own.any() or not omit_empty:
            names.append(name)
            members.append(neg | own)
    return GroupSet.from_members(names, members)


def _is_placeholder(value) -> bool:
    """What a manifest writes where a perturbation field does not apply: None, "", blanks, nan / none / null, a non-finite number,
    -1 in any spelling (train_classification.py:82-110).  A bool is a value."""
    if value is None or (isinstance(value, str) and value == ""):
        return True
    if isinstance(value, (bool, np.bool_)):
        return False
    if isinstance(value, (int, np.integer)):
        return int(value) == -1
    if isinstance(value, (float, np.floating)):
        return not np.isfinite(float(value)) or float(value) == -1.0
    if isinstance(value, str):
        text = value.strip()
        if not text or text.lower() in _PLACEHOLDER_WORDS:
            return True
        try:
            number = float(text)
        except ValueError:
            return False
        return not np.isfinite(number) or number == -1.0
    return False


def _numeric_token(value) -> str:
    """_format_numeric_token (:619-632): bools lower-case, integers plain, floats with at most four decimals and no trailing zeros."""
    if isinstance(value, (bool, np.bool_)):
        return str(bool(value)).lower()
    if isinstance(value, (int, np.integer)):
        return str(int(value))
    if isinstance(value, (float, np.floating)):
        number = float(value)
        if not np.isfinite(number):
            return str(number)
        return f"{number:.4f}".rstrip("0").rstrip(".") or "0"
    return str(value)


def perturbation_tag(row):
    """The canonical perturbation tag of a row, or None (_canonicalize_perturbation_tag, :635-666): its `perturbation_id` if that
    is a value, else `field=value` joined by `|` over blur_sigma, jpeg_q, brightness, contrast, bbox_area_frac that hold one, else
    its `variant`."""
    if not hasattr(row, "get"):
        return None
    if not _is_placeholder(row.get("perturbation_id")):
        text = str(row.get("perturbation_id")).strip()
        if text:
            return text
    parts = [f"{f}={_numeric_token(row.get(f))}" for f in _TAG_NUMERIC_FIELDS if not _is_placeholder(row.get(f))]
    if parts:
        return "|".join(parts)
    if not _is_placeholder(row.get("variant")):
        return str(row.get("variant")).strip() or None
    return None


def _tag_sort_key(tag: str):
    """:5272-5288: `clean` first; a tag is compared component by component (`name=value` between `|`), by name, then numeric values
    before textual ones, numbers by value.  The tag itself breaks the ties the reference leaves to the order of a set."""
    if tag == CLEAN_TAG:
        return (0, (), tag)
    parts = []
    for segment in str(tag).split("|"):
        name, _, value = segment.partition("=")
        name, value = name.strip(), value.strip()
        if not name and not value:
            continue
        try:
            parts.append((name, 0, float(value), ""))
        except ValueError:
            parts.append((name, 1, 0.0, value))
    return (1, tuple(parts), tag)


def perturbation_groups(rows) -> GroupSet:
    """One group per perturbation tag of the rows, in the reference's order of report (:5272-5291, :5449-5457): `clean` (a row
    without a tag is clean, :4779-4786 and :5060-5062), every other tag by _tag_sort_key, then `ALL-perturbed` = every frame that is
    not clean, when there is one."""
    tags = np.array([perturbation_tag(r) or CLEAN_TAG for r in rows], dtype=object)
    names = sorted(set(tags.tolist()), key=_tag_sort_key)
    members = [tags == t for t in names]
    if (tags != CLEAN_TAG).any():
        names.append(ALL_PERTURBED)
        members.append(tags != CLEAN_TAG)
    return GroupSet.from_members(names, members)


def _device_of(probs, device):
    if device is not None:
        return device
    return probs.device if isinstance(probs, torch.Tensor) and probs.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _entries(groups: GroupSet, N: int, device):
    """(entry_frame i64 [E], group of every entry i64 [E]) on the device; the tables are checked on the host, where they live."""
    ef = groups.entry_frame
    if ef.size and (ef.min() < 0 or ef.max() >= N):
        raise ValueError(f"a group names frame {int(ef.min() if ef.min() < 0 else ef.max())}: the set has {N} frames")
    grp = np.repeat(np.arange(len(groups), dtype=np.int64), groups.sizes)
    return torch.from_numpy(ef.astype(np.int64)).to(device), torch.from_numpy(grp).to(device)


def group_member_order(score: torch.Tensor, groups: GroupSet) -> torch.Tensor:
    """pm_group_metrics' `member` i32 [M, E] for score f64 [M, N] on the device: per run the entries by group ascending, then by
    score descending, entries of one group and one score in ascending frame order -- a group's segment is the stable descending
    sort of its gathered frames, which is what bootstrap_binary_metrics builds for the subset.  Two stable sorts on the device."""
    ef, grp = _entries(groups, score.shape[1], score.device)
    by_score = torch.sort(score[:, ef], dim=1, descending=True, stable=True).indices
    by_group = torch.sort(grp[by_score], dim=1, stable=True).indices
    return ef[by_score.gather(1, by_group)].to(torch.int32).contiguous()


def bootstrap_group_metrics(probs, labels, tau, groups: GroupSet, cluster, draws, n_clusters=None, chunk=CHUNK,
                            device=None) -> torch.Tensor:
    """bootstrap_binary_metrics per group: f64 [R, M, G, 16] on the device, G = len(groups), by one pm_group_metrics call per chunk
    of replicates whatever G is.  cluster and draws are those of the whole set: replicate r of a group is replicate r of the set
    restricted to the group, so the groups' intervals and the overall one come from the same resamples.  Group g's values are, bit
    for bit, bootstrap_binary_metrics on the frames groups.frames(g) alone (probs[:, f], labels[f], cluster[f], the same draws and
    n_clusters), and do not depend on the other groups or on the chunk size."""
    device = _device_of(probs, device)
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
    G = len(groups)
    C = int(n_clusters) if n_clusters is not None else int(np.asarray(cluster.cpu() if isinstance(cluster, torch.Tensor) else cluster).max()) + 1
    tau_d = dev(torch.full((M,), float(tau), dtype=torch.float64) if np.ndim(tau) == 0 else tau, torch.float64)
    if tau_d.shape != (M,):
        raise ValueError(f"tau: one value or one per run ({M}), got {tuple(tau_d.shape)}")
    out = torch.empty((R, M, G, len(METRIC_KEYS)), dtype=torch.float64, device=device)
    if G == 0 or R == 0:
        return out
    if groups.entry_frame.size:
        member = group_member_order(score, groups)
    else:   # every group is empty: one padding entry that belongs to no segment
        _entries(groups, N, device)
        member = torch.full((M, 1), -1, dtype=torch.int32, device=device)
    E = member.shape[1]
    seg = torch.from_numpy(groups.seg).to(device)
    lib = _lib.load()
    chunk = max(1, min(int(chunk), MAX_REPLICATES_PER_CALL, R))
    ws = torch.empty(_lib.workspace_bytes("pm_group_metrics_workspace", N, M, E, G, chunk, K, C), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        _lib.check(lib.pm_group_metrics(score.data_ptr(), member.data_ptr(), seg.data_ptr(), label.data_ptr(), cl.data_ptr(),
                                        dr[r0:].data_ptr(), tau_d.data_ptr(), out[r0:].data_ptr(), N, M, E, G, n, K, C, int(r0 > 0),
                                        ws.data_ptr(), ws.numel(), stream), "pm_group_metrics")
    return out


def group_metrics(probs, labels, tau, groups: GroupSet, device=None) -> dict:
    """One evaluation per group: {name: the 16 values of compute_binary_metrics on the group's frames} in the groups' order (R = 1,
    every frame once) -- _binary_subset_metrics of every stratum, the per-tag block of the reference's test()."""
    n = int(torch.as_tensor(labels).numel())
    if n == 0 or len(groups) == 0:
        return {}
    out = bootstrap_group_metrics(probs, labels, tau, groups, np.zeros(n, dtype=np.int32), np.zeros((1, 1), dtype=np.int32),
                                  n_clusters=1, device=device)[0, 0].tolist()
    return {name: dict(zip(METRIC_KEYS, row)) for name, row in zip(groups.names, out)}


def group_case_metrics(probs, labels, tau, groups: GroupSet, case_index, n_cases=None, device=None) -> dict:
    """Recall, F1 and frame count per (group, case) of one run, as train_classification.py:5335-5371 reports them per (tag, case):
    {"count": i64 [G, n_cases], "recall": f64, "f1": f64} on the device.  case_index int [N]: the case of every frame as an index
    in [0, n_cases).  The four counts come from torch.bincount and each value is one f64 division of integers -- recall_score and
    f1_score(zero_division=0): 0 where the denominator is empty.  A (group, case) pair without a frame has count 0."""
    device = _device_of(probs, device)
    score = torch.as_tensor(probs).to(device=device, dtype=torch.float64).reshape(-1)
    N = score.numel()
    y = torch.as_tensor(labels).to(device=device, dtype=torch.int64).reshape(-1)
    case = torch.as_tensor(case_index).to(device=device, dtype=torch.int64).reshape(-1)
    if y.shape != (N,) or case.shape != (N,):
        raise ValueError(f"shapes: probs {N}, labels {tuple(y.shape)}, case_index {tuple(case.shape)}")
    host_case = np.asarray(case_index.cpu() if isinstance(case_index, torch.Tensor) else case_index).reshape(-1)
    n_cases = int(n_cases) if n_cases is not None else (int(host_case.max()) + 1 if N else 0)
    if N and (host_case.min() < 0 or host_case.max() >= n_cases):
        raise ValueError(f"case_index outside [0, {n_cases})")
    G = len(groups)
    t = torch.as_tensor(tau).to(device=device, dtype=torch.float64).reshape(-1)[:1] if np.ndim(tau) else \
        torch.full((1,), float(tau), dtype=torch.float64, device=device)
    ef, grp = _entries(groups, N, device)
    key = grp * n_cases + case[ef]
    pred, truth = score[ef] >= t, y[ef] == 1
    count = lambda mask: torch.bincount(key[mask], minlength=G * n_cases).reshape(G, n_cases)
    tp, fp, fn = count(pred & truth), count(pred & ~truth), count(~pred & truth)
    total = torch.bincount(key, minlength=G * n_cases).reshape(G, n_cases)
    ratio = lambda a, b: torch.where(b > 0, a.to(torch.float64) / b.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=device))
    return {"count": total, "recall": ratio(tp, tp + fn), "f1": ratio(2 * tp, 2 * tp + fp + fn)}


def threshold_grid_counts(probs, labels, taus, groups: GroupSet = None, device=None) -> torch.Tensor:
    """tp, fp, tn, fn of `score >= tau` for every run, group and threshold: i64 [M, G, T, 4] on the device (groups None: one group
    of every frame).  Per run the entries are sorted once by (group, score); a threshold is a torch.searchsorted into a group's
    segment and its counts are differences of one cumulative sum of the labels: exact integers, T thresholds for the price of one."""
    device = _device_of(probs, device)
    score = torch.as_tensor(probs).to(device=device, dtype=torch.float64)
    if score.ndim == 1:
        score = score[None]
    M, N = score.shape
    y = torch.as_tensor(labels).to(device=device, dtype=torch.int64).reshape(-1)
    t = torch.as_tensor(taus).to(device=device, dtype=torch.float64).reshape(-1)
    if y.shape != (N,):
        raise ValueError(f"shapes: probs {tuple(score.shape)}, labels {tuple(y.shape)}")
    if groups is None:
        groups = GroupSet(("all",), np.arange(N), (0, N))
    G, T = len(groups), t.numel()
    ef, grp = _entries(groups, N, device)
    by_score = torch.sort(score[:, ef], dim=1, stable=True)
    by_group = torch.sort(grp[by_score.indices], dim=1, stable=True).indices
    s_sorted = by_score.values.gather(1, by_group)
    positives = torch.cat([torch.zeros((M, 1), dtype=torch.int64, device=device),
                           torch.cumsum((y[ef] == 1).to(torch.int64)[by_score.indices.gather(1, by_group)], dim=1)], dim=1)
    out = torch.zeros((M, G, T, 4), dtype=torch.int64, device=device)
    want = t[None].expand(M, T).contiguous()
    for g in range(G):
        a, b = int(groups.seg[g]), int(groups.seg[g + 1])
        if a == b:
            continue
        below = torch.searchsorted(s_sorted[:, a:b].contiguous(), want)   # entries of the segment with score < tau
        P = (positives[:, b] - positives[:, a])[:, None]
        fn = positives.gather(1, a + below) - positives[:, a:a + 1]
        tp = P - fn
        fp = (b - a) - below - tp
        out[:, g] = torch.stack([tp, fp, (b - a) - P - fp, fn], dim=-1)
    return out


def f1_morph_threshold(probs, labels, morphology, grid_points: int = 512, device=None):
    """The reference's `f1-morph` threshold (_compute_f1_morph_threshold, train_classification.py:3092-3126): over
    numpy.linspace(0, 1, max(2, grid_points)) the first tau that maximises the mean of the two strata's F1 (flat + negatives,
    polypoid + negatives; F1 = 0 where its denominator is empty), as a float; None where the reference gives none -- no frames, not
    one morphology value per frame, or no flat or no polypoid positive -- and the caller falls back to `youden`."""
    y = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64).reshape(-1)
    if y.size == 0 or int(torch.as_tensor(probs).numel()) == 0 or len(morphology) != y.size:
        return None
    morph = _morphology_array(morphology)
    if not ((y == 1) & (morph == "flat")).any() or not ((y == 1) & (morph == "polypoid")).any():
        return None
    taus = np.linspace(0.0, 1.0, num=max(2, int(grid_points)), endpoint=True)
    strata = morphology_groups(morph.tolist(), y, omit_empty=False).subset(STRATA[1:])
    counts = threshold_grid_counts(torch.as_tensor(probs).reshape(-1), y, taus, strata, device=device)[0].cpu().numpy()
    tp, fp, fn = counts[..., 0], counts[..., 1], counts[..., 3]
    den = 2 * tp + fp + fn
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    return float(taus[int(np.argmax(0.5 * (f1[0] + f1[1])))])   # the first maximum: the reference replaces on `>` alone


def curve_rows(probs, labels, grid_points: int = 200, device=None):
    """(roc rows, pr rows) of _export_curve_sets (train_classification.py:3129-3206) over numpy.linspace(0, 1, grid_points): dicts
    with threshold = round(tau, 10), the counts, and tpr / fpr resp. precision / recall / f1, None where a denominator is empty
    (f1 also where precision + recall is 0)."""
    if grid_points is None or int(grid_points) < 2:
        raise ValueError("Curve export requires at least two grid points.")
    n = int(torch.as_tensor(labels).numel())
    if int(torch.as_tensor(probs).numel()) != n:
        raise ValueError("Mismatch between probability and target counts for curve export.")
    if n == 0:
        raise ValueError("Curve export received no samples.")
    taus = np.linspace(0.0, 1.0, num=int(grid_points), endpoint=True)
    counts = threshold_grid_counts(torch.as_tensor(probs).reshape(-1), labels, taus, device=device)[0, 0].tolist()
    frac = lambda a, b: float(a) / float(b) if b > 0 else None
    roc, pr = [], []
    for tau, (tp, fp, tn, fn) in zip(taus, counts):
        tpr, fpr, precision = frac(tp, tp + fn), frac(fp, fp + tn), frac(tp, tp + fp)
        f1 = None
        if precision is not None and tpr is not None and precision + tpr > 0:
            f1 = 2.0 * precision * tpr / (precision + tpr)
        base = {"threshold": round(float(tau), 10)}
        tail = {"tp": tp, "fp": fp, "tn": tn, "fn": fn}
        roc.append({**base, "tpr": tpr, "fpr": fpr, **tail})
        pr.append({**base, "precision": precision, "recall": tpr, "f1": f1, **tail})
    return roc, pr


def export_curves(stem, split: str, probs, labels, grid_points: int = 200, device=None) -> dict:
    """Writes <stem>_<split>_roc_curve.csv and <stem>_<split>_pr_curve.csv (the reference's columns; an undefined value is an empty
    cell) and returns {"roc_csv", "pr_csv", "grid_points"}.  `stem` is a path without extension, as a checkpoint's."""
    import csv
    from pathlib import Path
    roc, pr = curve_rows(probs, labels, grid_points, device=device)
    stem = Path(stem)
    paths = {kind: stem.with_name(f"{stem.name}_{split}_{kind}_curve.csv") for kind in ("roc", "pr")}
    stem.parent.mkdir(parents=True, exist_ok=True)
    for kind, rows in (("roc", roc), ("pr", pr)):
        with paths[kind].open("w", newline="") as f:
            writer = csv.DictWriter(f, fieldnames=list(rows[0]))
            writer.writeheader()
            writer.writerows(rows)
    return {"roc_csv": str(paths["roc"]), "pr_csv": str(paths["pr"]), "grid_points": int(grid_points)}
