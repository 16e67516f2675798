"""Generator of tests/golden/boot_metrics.npz -- bootstrap replicates of the binary metrics, as the REFERENCE computes them.

Every expected value in the file is what the reference's classification/analysis/common_metrics.py returns: clusters from its
build_cluster_set, draws from its sample_cluster_ids on a numpy Generator, and the 16 values of its compute_binary_metrics
(scikit-learn) on the gathered sample of every replicate.  The draws are stored as cluster indices (positives' clusters numbered
first, in the reference's order); the generator checks that expanding them gives exactly the frame list sample_cluster_ids
returned.  Only data is stored: inputs, draws, expected values.

    PYTHONPATH=<reference checkout>/src python tests/golden/make_boot_metrics_fixture.py      (needs scikit-learn)

Contents (scores are stored as float32 and used as float64 = what a model's probabilities are):
  size<N>/...           N in SIZES around the scan tile, R = 16 stratified draws, three runs per score kind ("cont" continuous,
                        "round" two decimals = tie groups that cross tiles, "equal" one group), tau per run below / inside / above
                        the score range
  a/..., b/...          two row sets (case_id per label, some rows without one) with their reference clusters, 37 replicates drawn
                        for both sets interleaved (the replicate is the outer loop), set a with two runs; a/single is the one
                        evaluation of the full set
  mult/...              set a with hand-made draws: one cluster 300 times, two clusters, a multiplicity above 65 535
  frame/...             per-frame clusters drawn over both classes at once, R = 64: replicates whose top tie group has weight
                        zero, replicates without positives and without negatives
"""
import os
import sys
import warnings
from pathlib import Path

import numpy as np

OUT = Path(__file__).with_name("boot_metrics.npz")
TILE = 1024
SIZES = (2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
KINDS = ("cont", "round", "equal")
KEYS = ("count", "n_pos", "n_neg", "prevalence", "tp", "fp", "tn", "fn", "auprc", "auroc", "recall", "precision", "f1",
        "balanced_accuracy", "mcc", "loss")


def reference():
    ref = os.environ.get("SSL4POLYP_REFERENCE")
    if ref:
        sys.path.insert(0, str(Path(ref) / "src"))
    try:
        from ssl4polyp.classification.analysis import common_metrics
    except ImportError as e:
        raise SystemExit(f"the reference is not importable ({e}): put <reference checkout>/src on PYTHONPATH")
    return common_metrics


def metrics_row(C, probs, labels, tau):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # scikit-learn's notes on absent classes
        m = C.compute_binary_metrics(np.asarray(probs, dtype=np.float64), np.asarray(labels, dtype=int), float(tau))
    assert tuple(m) == KEYS, tuple(m)
    return [m[k] for k in KEYS]


def cluster_index(C, frame_ids, labels, case_ids):
    """The reference's clusters of these rows -> (ClusterSet, cluster index per frame: positives first, then negatives)."""
    rows = list(zip(frame_ids, labels, case_ids))
    cs = C.build_cluster_set(rows, is_positive=lambda r: r[1] == 1, record_id=lambda r: r[0],
                             positive_key=lambda r: f"pos_case::{r[2]}" if r[2] else None,
                             negative_key=lambda r: f"neg_case::{r[2]}" if r[2] else None)
    where = {}
    for c, members in enumerate(cs.positives + cs.negatives):
        for fid in members:
            assert fid not in where
            where[fid] = c
    return cs, np.array([where[f] for f in frame_ids], dtype=np.int32)


def draw(C, cs, rng):
    """One call of the reference's sample_cluster_ids -> (frame ids it returned, the draws as cluster indices).  The indices come
    from a twin generator in the same state and are verified by expanding them."""
    twin = np.random.Generator(type(rng.bit_generator)())
    twin.bit_generator.state = rng.bit_generator.state
    ids = C.sample_cluster_ids(cs, rng)
    idx = []
    if cs.positives:
        idx += [int(i) for i in twin.integers(0, len(cs.positives), size=len(cs.positives))]
    if cs.negatives:
        idx += [len(cs.positives) + int(i) for i in twin.integers(0, len(cs.negatives), size=len(cs.negatives))]
    assert twin.bit_generator.state == rng.bit_generator.state
    both = cs.positives + cs.negatives
    assert [f for i in idx for f in both[i]] == ids
    return ids, np.array(idx, dtype=np.int32)


def expand(draws, cluster):
    """Frame indices of a replicate given as cluster indices (-1 = padding), in draw order."""
    members = {}
    for i, c in enumerate(cluster):
        members.setdefault(int(c), []).append(i)
    return np.array([i for c in draws if c >= 0 for i in members[int(c)]], dtype=np.int64)


def replicate_refs(C, score, labels, tau, cluster, draws):
    """[R, M, 16] of the reference on the gathered samples."""
    out = np.empty((len(draws), score.shape[0], 16))
    for r, d in enumerate(draws):
        take = expand(d, cluster)
        for m in range(score.shape[0]):
            out[r, m] = metrics_row(C, score[m].astype(np.float64)[take], labels[take], tau[m])
    return out


def rows_set(rng, n, n_cases, prefix, missing):
    labels = (rng.random(n) < 0.4).astype(np.uint8)
    labels[:2] = (1, 0)
    frame_ids = [f"{prefix}{i:04d}" for i in range(n)]
    case_ids = [f"case{int(c):03d}" for c in rng.integers(0, n_cases, n)]
    for i in rng.choice(n, missing, replace=False):
        case_ids[int(i)] = ""
    return frame_ids, labels, case_ids


def scores(rng, labels, kind, runs):
    n = len(labels)
    if kind == "equal":
        return np.full((runs, n), 0.5, dtype=np.float32)
    s = np.clip(0.35 * labels[None, :] + rng.uniform(0.02, 0.63, (runs, n)), 0.0, 1.0).astype(np.float32)
    return np.round(s, 2).astype(np.float32) if kind == "round" else s


def taus(score):
    """Per run: below, inside (the median score: frames AT tau are predicted positive), above the score range."""
    s = score.astype(np.float64)
    kinds = (lambda v: v.min() - 0.1, lambda v: float(np.median(v)), lambda v: v.max() + 0.1)
    return np.array([kinds[m % 3](s[m]) for m in range(s.shape[0])])


def main():
    C = reference()
    import sklearn
    fx = {"keys": np.array(KEYS), "sklearn_version": np.array(sklearn.__version__), "tile": np.array(TILE)}
    rng = np.random.default_rng(20240518)

    # ---- the sizes around the scan tile
    for n in SIZES:
        if n == 2:
            frame_ids, labels, case_ids = ["s0", "s1"], np.array([1, 0], dtype=np.uint8), ["x", "x"]
        else:
            frame_ids, labels, case_ids = rows_set(rng, n, max(2, n // 12), "s", n // 50)
        cs, cluster = cluster_index(C, frame_ids, labels, case_ids)
        draws = np.stack([draw(C, cs, rng)[1] for _ in range(16)])
        fx[f"size{n}/label"], fx[f"size{n}/cluster"], fx[f"size{n}/draws"] = labels, cluster, draws
        for kind in KINDS:
            s = scores(rng, labels, kind, 3)
            tau = taus(s)
            fx[f"size{n}/{kind}/score"], fx[f"size{n}/{kind}/tau"] = s, tau
            fx[f"size{n}/{kind}/ref"] = replicate_refs(C, s, labels, tau, cluster, draws)
        print(f"size {n}: {len(cs.positives)} + {len(cs.negatives)} clusters")

    # ---- two row sets, drawn interleaved as the reports draw over seeds
    sets = {}
    for name, n, n_cases, runs in (("a", 700, 260, 2), ("b", 50, 12, 1)):
        frame_ids, labels, case_ids = rows_set(rng, n, n_cases, name, n // 10)
        cs, cluster = cluster_index(C, frame_ids, labels, case_ids)
        s = scores(rng, labels, "cont", runs)
        if runs > 1:
            s[1] = np.round(s[1], 1)   # heavy ties
        sets[name] = (cs, cluster, labels, s)
        fx[f"{name}/frame_id"], fx[f"{name}/case_id"] = np.array(frame_ids), np.array(case_ids)
        fx[f"{name}/label"], fx[f"{name}/cluster"], fx[f"{name}/score"] = labels, cluster, s
        fx[f"{name}/n_pos_clusters"] = np.array(len(cs.positives))
        fx[f"{name}/tau"] = np.full(runs, 0.5)
    assert int(sets["a"][1].max()) + 1 >= 300
    fx["ab/seed"] = np.array(77)
    rng_ab = np.random.default_rng(77)
    drawn = {"a": [], "b": []}
    for _ in range(37):
        for name in ("a", "b"):
            drawn[name].append(draw(C, sets[name][0], rng_ab)[1])
    for name in ("a", "b"):
        cs, cluster, labels, s = sets[name]
        fx[f"{name}/draws"] = np.stack(drawn[name])
        fx[f"{name}/ref"] = replicate_refs(C, s, labels, fx[f"{name}/tau"], cluster, fx[f"{name}/draws"])
    cs, cluster, labels, s = sets["a"]
    fx["a/single"] = np.array([metrics_row(C, s[m].astype(np.float64), labels, 0.5) for m in range(2)])

    # ---- multiplicities: set a, hand-made draws (the centre-level form: any list of clusters is a replicate)
    pos_c, neg_c = 3, len(cs.positives) + 5
    big = 70000
    d = np.full((5, big), -1, dtype=np.int32)
    d[0, :300] = pos_c                                  # one cluster 300 times: a multiplicity above 255, no negatives
    d[1, :300] = neg_c                                  # no positives
    d[2, :150], d[2, 150:300] = pos_c, neg_c
    d[3, :299], d[3, 299] = pos_c, neg_c
    d[4, :66000], d[4, 66000:] = pos_c, neg_c           # a multiplicity above 65 535
    fx["mult/draws"] = d
    fx["mult/ref"] = replicate_refs(C, s, labels, fx["a/tau"], cluster, d)

    # ---- per-frame clusters drawn over both classes at once: absent classes, a top tie group of weight zero
    n = 6
    labels = np.array([1, 0, 0, 1, 0, 0], dtype=np.uint8)
    s = np.array([[0.9, 0.9, 0.4, 0.4, 0.2, 0.7]], dtype=np.float32)
    cluster = np.arange(n, dtype=np.int32)
    d = rng.integers(0, n, (64, n)).astype(np.int32)
    d[62], d[63] = (0, 3, 3, 0, 0, 3), (1, 2, 4, 5, 5, 1)
    tau = np.array([0.5])
    fx["frame/label"], fx["frame/score"], fx["frame/cluster"], fx["frame/draws"], fx["frame/tau"] = labels, s, cluster, d, tau
    fx["frame/ref"] = replicate_refs(C, s, labels, tau, cluster, d)
    top = [i for i in range(n) if s[0, i] == s[0].max()]
    assert any(not np.isin(top, row).any() for row in d), "no replicate whose top tie group has weight zero"
    assert any(fx["frame/ref"][r, 0, 1] == 0 for r in range(64)) and any(fx["frame/ref"][r, 0, 2] == 0 for r in range(64)), \
        "no replicate with an absent class"
    for r in range(64):
        if fx["frame/ref"][r, 0, 1] == 0 or fx["frame/ref"][r, 0, 2] == 0:
            print(f"frame replicate {r}: " + ", ".join(f"{k}={v:g}" for k, v in zip(KEYS, fx['frame/ref'][r, 0])))

    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(fx)} arrays)")


if __name__ == "__main__":
    main()
