"""Generator of tests/golden/group_metrics.npz -- per-group metrics (perturbation tags, morphology strata), as the REFERENCE computes
them.

Every expected value in the file is what the reference's own functions returned:
  * common_metrics.compute_binary_metrics on the gathered sample of every (replicate, run, group): the frames of the group whose
    cluster the replicate drew, as often as it drew it (an empty sample included);
  * train_classification._build_morphology_strata_metrics / _binary_subset_metrics (the strata of one evaluation),
    _compute_f1_morph_threshold, _export_curve_sets (the text of the two CSV files) and _canonicalize_perturbation_tag;
  * the per-(tag, case) values are the recall_score / f1_score(zero_division=0) calls test() makes (train_classification.py:5352-5361).
train_classification imports with an empty `torchvision` module in sys.modules (it is not installed; nothing used here touches it).
Only data is stored: inputs, draws, expected values, CSV text.  The order in which test() reports the tags comes from a nested
function that cannot be called; the CPU test pins it by a literal list.

    SSL4POLYP_REFERENCE=<reference checkout> python tests/golden/make_group_metrics_fixture.py      (needs scikit-learn)

Contents (scores are stored as float32 and used as float64):
  sizes/...     6 T + 8 frames (T = the scan tile) dealt at random to groups of 0, 1, 2, T - 1, T, T + 1, 3 T + 5 frames, plus one
                group of every frame; R = 16 stratified draws; three runs per score kind (cont / round / equal) with tau below /
                inside / above the range; ref [R, M, G, 16] per kind
  morph/...     rows with mixed-case and padded morphology spellings, a third morphology and missing values; strata of one
                evaluation per run; replicates over the always-three strata, the last two of them hand-made so that a stratum gets
                weight zero; the f1-morph tau per run
  noflat/...    the same rows with every flat positive turned into a negative: the stratum is omitted / has no positives
  grid/...      a larger set for the f1-morph tau and the curve files
  tags/...      rows as typed values (JSON) and as CSV strings with the tag of each
  pert/...      a multi-tag set over a few cases: replicates per tag and for ALL-perturbed, per-(tag, case) recall / F1 / count
"""
import json
import os
import sys
import tempfile
import types
import warnings
from pathlib import Path

import numpy as np

OUT = Path(__file__).with_name("group_metrics.npz")
TILE = 1024
GROUP_SIZES = (0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
KINDS = ("cont", "round", "equal")
KEYS = ("count", "n_pos", "n_neg", "prevalence", "tp", "fp", "tn", "fn", "auprc", "auroc", "recall", "precision", "f1",
        "balanced_accuracy", "mcc", "loss")


def reference():
    root = os.environ.get("SSL4POLYP_REFERENCE")
    if root:
        sys.path.insert(0, str(Path(root) / "src"))
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    try:
        from ssl4polyp.classification import train_classification as tc
        from ssl4polyp.classification.analysis import common_metrics
    except ImportError as e:
        raise SystemExit(f"the reference is not importable ({e}): set SSL4POLYP_REFERENCE=<reference checkout>")
    return tc, common_metrics


def metrics_row(C, probs, labels, tau):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # scikit-learn's notes on absent classes
        m = C.compute_binary_metrics(np.asarray(probs, dtype=np.float64), np.asarray(labels, dtype=int), float(tau))
    assert tuple(m) == KEYS, tuple(m)
    return [m[k] for k in KEYS]


def stratified_draws(rng, cluster, labels, R):
    """Cluster indices per replicate as sample_cluster_ids draws them: the positives' clusters, then the negatives'."""
    n_pos = len(set(cluster[labels == 1].tolist()))
    n_all = int(cluster.max()) + 1
    assert set(cluster[labels == 1].tolist()) == set(range(n_pos))   # positives' clusters are numbered first
    return np.stack([np.concatenate([rng.integers(0, n_pos, n_pos), n_pos + rng.integers(0, n_all - n_pos, n_all - n_pos)])
                     for _ in range(R)]).astype(np.int32)


def clusters_by_case(labels, case):
    """Positives' clusters first, then negatives', each in order of first appearance (a case never spans the classes)."""
    table, out = {}, np.empty(len(labels), dtype=np.int32)
    for want in (1, 0):
        for i, (y, c) in enumerate(zip(labels, case)):
            if y == want:
                out[i] = table.setdefault((want, c), len(table))
    return out


def group_refs(C, score, labels, tau, cluster, draws, members):
    """[R, M, G, 16] of the reference on the gathered samples: the replicate's frames that belong to the group."""
    out = np.empty((len(draws), score.shape[0], len(members), 16))
    s64 = score.astype(np.float64)
    by_cluster = {}
    for i, c in enumerate(cluster):
        by_cluster.setdefault(int(c), []).append(i)
    for r, d in enumerate(draws):
        take = np.array([i for c in d if c >= 0 for i in by_cluster.get(int(c), [])], dtype=np.int64)
        for g, frames in enumerate(members):
            mine = take[np.isin(take, frames)]
            for m in range(score.shape[0]):
                out[r, m, g] = metrics_row(C, s64[m][mine], labels[mine], tau[m])
    return out


def scores(rng, labels, kind, runs):
    n = len(labels)
    if kind == "equal":
        return np.full((runs, n), 0.5, dtype=np.float32)
    s = np.clip(0.35 * labels[None, :] + rng.uniform(0.02, 0.63, (runs, n)), 0.0, 1.0).astype(np.float32)
    return np.round(s, 2).astype(np.float32) if kind == "round" else s


def taus(score):
    """Per run: below, inside (the median score), above the score range."""
    s = score.astype(np.float64)
    kinds = (lambda v: v.min() - 0.1, lambda v: float(np.median(v)), lambda v: v.max() + 0.1)
    return np.array([kinds[m % 3](s[m]) for m in range(s.shape[0])])


def strata_block(tc, score64, labels, tau, morphology):
    """_build_morphology_strata_metrics -> (names, [len(names), 16])."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        strata = tc._build_morphology_strata_metrics(positive_scores=score64, preds=(score64 >= tau).astype(int), labels=labels.astype(int),
                                                     morphology=morphology)
    for v in strata.values():
        assert tuple(v) == KEYS
    return np.array(list(strata)), np.array([[v[k] for k in KEYS] for v in strata.values()], dtype=np.float64)


def read(path):
    with open(path, newline="") as f:   # the csv module's own line ends
        return f.read()


def main():
    tc, C = reference()
    import sklearn
    import torch
    from sklearn.metrics import f1_score, recall_score
    fx = {"keys": np.array(KEYS), "sklearn_version": np.array(sklearn.__version__), "tile": np.array(TILE)}
    rng = np.random.default_rng(20241020)

    # ---- group sizes around the scan tile
    n = sum(GROUP_SIZES)
    labels = (rng.random(n) < 0.4).astype(np.uint8)
    case = rng.integers(0, n // 12, n)
    cluster = clusters_by_case(labels, case)
    deal = rng.permutation(n)
    cuts = np.concatenate([[0], np.cumsum(GROUP_SIZES)])
    members = [np.sort(deal[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [np.arange(n)]
    for frames in members[1:]:
        assert set(labels[frames].tolist()) <= {0, 1}
    draws = stratified_draws(rng, cluster, labels, 16)
    fx["sizes/label"], fx["sizes/cluster"], fx["sizes/draws"] = labels, cluster, draws
    fx["sizes/group_of_frame"] = np.empty(n, dtype=np.int32)
    for g, frames in enumerate(members[:-1]):
        fx["sizes/group_of_frame"][frames] = g
    fx["sizes/group_sizes"] = np.array(GROUP_SIZES)
    for kind in KINDS:
        s = scores(rng, labels, kind, 3)
        tau = taus(s)
        fx[f"sizes/{kind}/score"], fx[f"sizes/{kind}/tau"] = s, tau
        fx[f"sizes/{kind}/ref"] = group_refs(C, s, labels, tau, cluster, draws, members)
        print(f"sizes/{kind}: done")

    # ---- morphology strata
    n = 90
    labels = (np.arange(n) % 3 != 0).astype(np.uint8)           # 60 positives, 30 negatives
    spell = {"flat": ("flat", " Flat", "FLAT  "), "polypoid": ("polypoid", "Polypoid ", "  POLYPOID"), "other": ("", "sessile", "  ")}
    kind_of = np.array([("flat", "polypoid", "polypoid", "other")[i % 4] if labels[i] else "" for i in range(n)], dtype=object)
    morphology = [spell[k][i % 3] if k else ("", " ", "flat")[(i // 3) % 3] for i, k in enumerate(kind_of)]   # a negative's value does not matter
    case = np.array([f"c{i // 3:02d}" for i in range(n)])      # a case holds a negative and two positives: clusters split per class
    cluster = clusters_by_case(labels, case)
    s = scores(rng, labels, "cont", 3)
    s[1] = np.round(s[1], 1)
    tau = taus(s)
    draws = stratified_draws(rng, cluster, labels, 16)
    flat_clusters = sorted(set(cluster[(labels == 1) & (kind_of == "flat")].tolist()))
    poly_only = sorted(set(cluster[(labels == 1) & (kind_of == "polypoid")].tolist()) - set(flat_clusters))
    assert poly_only
    draws[14] = -1
    draws[14, :3] = poly_only[:3]                               # no negative, no flat positive: flat_plus_negs has weight zero
    flat_no_poly = sorted(set(flat_clusters) - set(cluster[(labels == 1) & (kind_of == "polypoid")].tolist()))
    assert flat_no_poly
    draws[15] = -1
    draws[15, :2] = flat_no_poly[:2]                            # no negative, no polypoid positive: polypoid_plus_negs has weight zero
    pos, neg = labels == 1, labels == 0
    norm = np.array([str(v).strip().lower() for v in morphology], dtype=object)
    three = [np.arange(n), np.flatnonzero(neg | (pos & (norm == "flat"))), np.flatnonzero(neg | (pos & (norm == "polypoid")))]
    fx["morph/label"], fx["morph/cluster"], fx["morph/draws"], fx["morph/score"], fx["morph/tau"] = labels, cluster, draws, s, tau
    fx["morph/morphology"] = np.array(morphology)
    fx["morph/boot_ref"] = group_refs(C, s, labels, tau, cluster, draws, three)
    assert fx["morph/boot_ref"][14, 0, 1, 0] == 0 and fx["morph/boot_ref"][14, 0, 2, 0] > 0 and fx["morph/boot_ref"][15, 0, 0, 0] > 0
    assert fx["morph/boot_ref"][15, 0, 2, 0] == 0 and fx["morph/boot_ref"][15, 0, 1, 0] > 0 and np.isnan(fx["morph/boot_ref"][14, 0, 1, 8:]).all()
    for m in range(3):
        names, block = strata_block(tc, s[m].astype(np.float64), labels, tau[m], morphology)
        assert names.tolist() == ["overall", "flat_plus_negs", "polypoid_plus_negs"]
        fx[f"morph/strata{m}"] = block
    f1m = [tc._compute_f1_morph_threshold(positive_scores=s[m].astype(np.float64), labels=labels.astype(int), morphology=morphology)
           for m in range(3)]
    assert all(t is not None for t in f1m)
    fx["morph/f1_morph_tau"] = np.array(f1m)
    fx["morph/f1_morph_tau_64"] = np.array(tc._compute_f1_morph_threshold(positive_scores=s[0].astype(np.float64), labels=labels.astype(int),
                                                                          morphology=morphology, grid_points=64))

    # ---- no flat positive
    labels2 = labels.copy()
    labels2[(labels == 1) & (norm == "flat")] = 0
    cluster2 = clusters_by_case(labels2, case)
    draws2 = stratified_draws(rng, cluster2, labels2, 16)
    pos, neg = labels2 == 1, labels2 == 0
    three2 = [np.arange(n), np.flatnonzero(neg | (pos & (norm == "flat"))), np.flatnonzero(neg | (pos & (norm == "polypoid")))]
    fx["noflat/label"], fx["noflat/cluster"], fx["noflat/draws"] = labels2, cluster2, draws2
    fx["noflat/boot_ref"] = group_refs(C, s, labels2, tau, cluster2, draws2, three2)
    names, block = strata_block(tc, s[0].astype(np.float64), labels2, tau[0], morphology)
    assert names.tolist() == ["overall", "polypoid_plus_negs"]
    fx["noflat/strata_names"], fx["noflat/strata0"] = names, block
    assert tc._compute_f1_morph_threshold(positive_scores=s[0].astype(np.float64), labels=labels2.astype(int), morphology=morphology) is None
    assert (fx["noflat/boot_ref"][:, :, 1, 1] == 0).all() and np.isnan(fx["noflat/boot_ref"][:, :, 1, 9]).all()

    # ---- a larger set: the f1-morph tau and the curve files
    n = 2000
    labels = (rng.random(n) < 0.35).astype(np.uint8)
    morph_g = [("flat", "polypoid", "Polypoid", "")[int(v)] if y else "" for v, y in zip(rng.integers(0, 4, n), labels)]
    s = scores(rng, labels, "cont", 2)
    s[1] = np.round(s[1], 2)
    fx["grid/label"], fx["grid/score"], fx["grid/morphology"] = labels, s, np.array(morph_g)
    fx["grid/f1_morph_tau"] = np.array([tc._compute_f1_morph_threshold(positive_scores=s[m].astype(np.float64), labels=labels.astype(int),
                                                                       morphology=morph_g) for m in range(2)])
    with tempfile.TemporaryDirectory() as tmp:
        for m, points in ((0, 200), (1, 33)):
            got = tc._export_curve_sets(Path(tmp) / f"stem{m}", "test", probabilities=torch.from_numpy(s[m]), targets=torch.from_numpy(labels.astype(np.int64)),
                                        grid_points=points)
            assert got["roc_csv"].name == f"stem{m}_test_roc_curve.csv" and got["pr_csv"].name == f"stem{m}_test_pr_curve.csv"
            fx[f"grid/roc_csv{m}"] = np.array(read(got["roc_csv"]))
            fx[f"grid/pr_csv{m}"] = np.array(read(got["pr_csv"]))
            fx[f"grid/points{m}"] = np.array(points)
        one = np.array([0.2, 0.9], dtype=np.float32)          # negatives only: tpr, precision, recall and f1 are undefined
        got = tc._export_curve_sets(Path(tmp) / "neg", "val", probabilities=torch.from_numpy(one), targets=torch.zeros(2, dtype=torch.long), grid_points=3)
        fx["grid/neg_score"], fx["grid/neg_roc_csv"], fx["grid/neg_pr_csv"] = one, np.array(read(got["roc_csv"])), np.array(read(got["pr_csv"]))

    # ---- tags: typed values and CSV strings
    nan = float("nan")
    typed = [
        {"perturbation_id": "blur_sigma=1.5", "blur_sigma": 2.0},
        {"perturbation_id": "  padded id ", "variant": "x"},
        {"perturbation_id": None, "blur_sigma": 1.5, "jpeg_q": -1, "variant": "blur"},
        {"perturbation_id": "", "blur_sigma": 1.0, "jpeg_q": 40},
        {"perturbation_id": "nan", "jpeg_q": 40, "brightness": 1.25, "contrast": 0.123456},
        {"perturbation_id": -1, "bbox_area_frac": 0.2, "variant": "occ"},
        {"perturbation_id": "NULL", "blur_sigma": nan, "jpeg_q": -1.0, "variant": " jpeg_q40 "},
        {"perturbation_id": "none", "variant": "clean"},
        {"variant": ""},
        {"variant": "-1"},
        {"perturbation_id": 7},
        {"perturbation_id": True, "blur_sigma": True},
        {"perturbation_id": " ", "blur_sigma": False},
        {"blur_sigma": 3, "contrast": 1.0, "brightness": 0.00004},
        {"blur_sigma": "1.50", "jpeg_q": "-1", "brightness": " 1.2 ", "contrast": "inf", "bbox_area_frac": "abc"},
        {"jpeg_q": "-1.0", "variant": "None"},
        {},
    ]
    fx["tags/typed_rows"] = np.array(json.dumps(typed))
    fx["tags/typed_expected"] = np.array(json.dumps([tc._canonicalize_perturbation_tag(r) for r in typed]))
    assert tc._canonicalize_perturbation_tag("not a row") is None

    # ---- a multi-tag set with cases
    columns = ("perturbation_id", "blur_sigma", "jpeg_q", "brightness", "contrast", "bbox_area_frac", "variant")
    variants = [dict(variant="clean"), dict(blur_sigma="1.5", variant="blur"), dict(blur_sigma="3", variant="blur"),
                dict(blur_sigma="10", variant="blur"), dict(jpeg_q="40", variant="jpeg"), dict(jpeg_q="5", variant="jpeg"),
                dict(brightness="1.3", contrast="0.7", variant="bc"), dict(bbox_area_frac="0.2", variant="occ"),
                dict(perturbation_id="custom"), dict(variant="odd_variant"), dict(perturbation_id="blur_sigma=abc")]
    n_cases, per = 5, 6
    rows, labels, case = [], [], []
    for v in variants:
        for c in range(n_cases):
            for k in range(per):
                rows.append({col: v.get(col, "-1" if col not in ("perturbation_id", "variant") else "") for col in columns})
                labels.append(1 if c < 3 else 0)        # cases 0-2 positive, 3-4 negative
                case.append(f"case{c}")
    labels, case = np.array(labels, dtype=np.uint8), np.array(case)
    rows[0]["variant"] = ""                                 # a row without any tag is clean
    n = len(rows)
    tags = np.array([tc._canonicalize_perturbation_tag(r) or "clean" for r in rows])
    cluster = clusters_by_case(labels, case)
    s = scores(rng, labels, "cont", 3)
    s[2] = np.round(s[2], 1)
    tau = np.array([0.5, float(np.median(s[1].astype(np.float64))), 0.45])
    draws = stratified_draws(rng, cluster, labels, 16)
    names = sorted(set(tags.tolist())) + ["ALL-perturbed"]   # NOT the order of report: the tests index by name
    members = [np.flatnonzero(tags == t) for t in names[:-1]] + [np.flatnonzero(tags != "clean")]
    for col in columns:
        fx[f"pert/col/{col}"] = np.array([r[col] for r in rows])
    fx["pert/case_id"], fx["pert/label"], fx["pert/cluster"], fx["pert/draws"], fx["pert/score"], fx["pert/tau"] = case, labels, cluster, draws, s, tau
    fx["pert/tag"], fx["pert/ref_names"] = tags, np.array(names)
    fx["pert/boot_ref"] = group_refs(C, s, labels, tau, cluster, draws, members)
    single = np.zeros((1, 1), dtype=np.int32)
    fx["pert/single_ref"] = group_refs(C, s, labels, tau, np.zeros(n, dtype=np.int32), single, members)[0]
    cases = sorted(set(case.tolist()))
    fx["pert/case_names"] = np.array(cases)
    per_case = np.full((3, len(names), len(cases), 3), np.nan)      # recall, f1, count
    for m in range(3):
        preds = (s[m].astype(np.float64) >= tau[m]).astype(int)
        for g, frames in enumerate(members):
            for ci, cname in enumerate(cases):
                idx = frames[case[frames] == cname]
                if idx.size:
                    per_case[m, g, ci] = (recall_score(labels[idx], preds[idx], zero_division=0),
                                          f1_score(labels[idx], preds[idx], zero_division=0), float(idx.size))
    fx["pert/per_case"] = per_case

    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(fx)} arrays)")


if __name__ == "__main__":
    main()
