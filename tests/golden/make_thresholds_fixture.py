"""Generator of tests/golden/thresholds.npz -- decision thresholds as the REFERENCE selects them.

Every expected value in the file is what the reference's classification/metrics/thresholds.py returned: compute_policy_threshold
(tau, record["n_candidates"], record["degenerate_val"], the metrics dict, the candidate list) for f1_opt_on_val, youden_on_val and
val_opt_youden, and compute_youden_j_threshold (tau) for youden, whose counts and metrics at that tau come from the reference's
_compute_confusion_arrays / _compute_metrics_for_tau and whose n_candidates is the number of points scikit-learn's roc_curve
returned.  Only data is stored: scores (f64), labels, previous taus, expected values.

    SSL4POLYP_REFERENCE=<reference checkout> python tests/golden/make_thresholds_fixture.py      (needs scikit-learn)

Contents, per case <c>: <c>/score f64 [M, N], <c>/label u8 [N], <c>/prev f64 [M] (NaN = none; <c>/prev_absent marks the runs
called without a previous_tau at all), <c>/cand f64 [M, 200] (NaN-padded, the same for the three candidate policies),
<c>/<policy>/exp f64 [M, 13] in `expected_keys` order; a one-class case has <c>/youden/error (the reference's message) instead.
  size<N>              N in SIZES around the scan tile; runs: continuous, rounded (a tie group across a tile boundary), all equal
  u199 u200 u201       U = 199, 200 and 201 unique values of {0} + scores + {1}: n_candidates 199, 200, and 200 out of 201
  u1000                U > 1000
  ends01               runs whose scores hold exactly 0.0 and 1.0, only 0.0, only 1.0 (every other case holds neither)
  perfect, inverted    separation; inverted run 0: youden = nextafter(max, 1.0); run 1 the same with a top score of exactly 1.0
  slope1               a slope-1 run of the ROC on which an interior point's J exceeds the kept end's by an ulp
  tie_recall, tie_tau  an objective tie (|S0| > 1) decided by recall, and one decided by the lower tau
  onepos, oneneg       one class only, previous_tau finite / NaN / absent
"""
import os
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).with_name("thresholds.npz")
TILE = 1024
SIZES = (2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
POLICIES = ("f1_opt_on_val", "youden_on_val", "val_opt_youden", "youden")
EXPECTED = ("tau", "n_candidates", "degenerate", "tp", "fp", "tn", "fn", "recall", "precision", "f1", "tpr", "fpr", "youden_j")
METRICS = EXPECTED[3:]


def reference():
    ref = os.environ.get("SSL4POLYP_REFERENCE")
    if ref:
        sys.path.insert(0, str(Path(ref) / "src"))
    try:
        from ssl4polyp.classification.metrics import thresholds
    except ImportError as e:
        raise SystemExit(f"the reference is not importable ({e}): put <reference checkout>/src on PYTHONPATH")
    return thresholds


def policy_row(T, score, label, policy, prev, absent):
    kw = {} if absent else {"previous_tau": None if prev is None else float(prev)}
    r = T.compute_policy_threshold(score.tolist(), label.tolist(), policy=policy, split_name="x/val", epoch=1, **kw)
    assert set(r.metrics) == set(METRICS) and r.tau == r.record["tau"]
    row = [r.tau, r.record["n_candidates"], float(r.record["degenerate_val"])] + [r.metrics[k] for k in METRICS]
    return row, list(r.candidates), r.record


def youden_row(T, score, label):
    import torch
    from sklearn.metrics import roc_curve
    with np.errstate(divide="ignore"):
        logits = torch.from_numpy(np.log(score) - np.log1p(-score))   # the reference takes logits: its sigmoid must give the scores back
    back = torch.sigmoid(logits).numpy().astype(float)
    if not np.array_equal(back, score):
        raise AssertionError("sigmoid(logit(score)) != score: choose scores that survive the round trip")
    tau = T.compute_youden_j_threshold(logits, torch.from_numpy(label.astype(np.int64)))
    n_points = len(roc_curve(label.astype(int), score)[2])
    tp, fp, tn, fn = T._compute_confusion_arrays(score, label.astype(int), np.array([tau]))
    m = T._compute_metrics_for_tau(int(tp[0]), int(fp[0]), int(tn[0]), int(fn[0]))
    return [tau, n_points, 0.0] + [m[k] for k in METRICS]


def objective_set(T, score, label, policy):
    """|S0| and the recalls inside it, from the reference's own helpers."""
    cand = T._prepare_candidate_thresholds(score)
    tp, fp, tn, fn = T._compute_confusion_arrays(score, label.astype(int), cand)
    rec = T._safe_divide(tp, tp + fn)
    obj = T._safe_divide(2 * tp, 2 * tp + fp + fn) if policy == "f1_opt_on_val" else rec - T._safe_divide(fp, fp + tn)
    s0 = obj >= obj.max() - T._EPS
    return int(s0.sum()), rec[s0]


def survive(score):
    """Scores as a model gives them: sigmoid of an f64 logit, fixed under logit -> sigmoid (the youden entry takes logits)."""
    import torch
    s = np.asarray(score, dtype=np.float64)
    for _ in range(8):
        with np.errstate(divide="ignore"):
            z = np.log(s) - np.log1p(-s)
        t = torch.sigmoid(torch.from_numpy(z)).numpy().astype(np.float64)
        if np.array_equal(t, s):
            return s
        s = t
    raise AssertionError("no fixed point of logit -> sigmoid")


def add_case(T, fx, name, score, label, prev=None, absent=None):
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    label = np.asarray(label, dtype=np.uint8)
    M, N = score.shape
    prev = np.full(M, np.nan) if prev is None else np.asarray(prev, dtype=np.float64)
    absent = np.zeros(M, dtype=np.uint8) if absent is None else np.asarray(absent, dtype=np.uint8)
    fx[f"{name}/score"], fx[f"{name}/label"], fx[f"{name}/prev"], fx[f"{name}/prev_absent"] = score, label, prev, absent
    cands = np.full((M, 200), np.nan)
    for policy in POLICIES[:3]:
        rows = []
        for m in range(M):
            row, c, _ = policy_row(T, score[m], label, policy, prev[m], bool(absent[m]))
            rows.append(row)
            line = np.full(200, np.nan)
            line[:len(c)] = c
            assert policy == POLICIES[0] or np.array_equal(line, cands[m], equal_nan=True)
            cands[m] = line
        fx[f"{name}/{policy}/exp"] = np.array(rows, dtype=np.float64)
    fx[f"{name}/cand"] = cands
    if len(np.unique(label)) < 2:
        import torch
        try:
            T.compute_youden_j_threshold(torch.zeros(N, dtype=torch.float64), torch.from_numpy(label.astype(np.int64)))
        except ValueError as e:
            fx[f"{name}/youden/error"] = np.array(str(e))
        else:
            raise AssertionError("the reference accepted one class for youden")
    else:
        fx[f"{name}/youden/exp"] = np.array([youden_row(T, score[m], label) for m in range(M)], dtype=np.float64)
    return fx[f"{name}/{POLICIES[0]}/exp"]


def separated(rng, label, runs=1):
    return survive(np.clip(0.35 * label[None, :] + rng.uniform(0.02, 0.63, (runs, len(label))), 1e-6, 1 - 1e-6))


def distinct(rng, d, n, label_rng):
    """n scores over exactly d distinct values inside (0, 1), and labels with both classes."""
    vals = survive(np.sort(rng.uniform(0.05, 0.95, d)))
    assert len(np.unique(vals)) == d
    s = np.r_[vals, rng.choice(vals, n - d)]
    rng.shuffle(s)
    label = (label_rng.random(n) < 0.3 + 0.4 * s).astype(np.uint8)
    label[:2] = (1, 0)
    return s, label


def main():
    T = reference()
    import sklearn
    from sklearn.metrics import roc_curve
    fx = {"expected_keys": np.array(EXPECTED), "policies": np.array(POLICIES), "sklearn_version": np.array(sklearn.__version__),
          "tile": np.array(TILE)}
    rng = np.random.default_rng(20250913)

    # ---- the sizes around the scan tile
    for n in SIZES:
        label = (rng.random(n) < 0.4).astype(np.uint8)
        label[:2] = (1, 0)
        cont = separated(rng, label)[0]
        rounded = survive(np.round(separated(rng, label)[0], 2))
        if n > TILE:
            srt = np.sort(rounded)[::-1]
            assert srt[TILE - 1] == srt[TILE], "no tie group across the first tile boundary"
        equal = survive(np.full(n, 0.5))
        add_case(T, fx, f"size{n}", np.stack([cont, rounded, equal]), label)

    # ---- U on both sides of the candidate budget
    for d, want in ((197, 199), (198, 200), (199, 200), (1400, 200)):
        s, label = distinct(rng, d, d + 40, rng)
        name = {197: "u199", 198: "u200", 199: "u201", 1400: "u1000"}[d]
        exp = add_case(T, fx, name, s, label)
        assert len(np.unique(np.r_[0.0, s, 1.0])) == d + 2 and exp[0, 1] == want, (name, exp[0, 1])

    # ---- scores that hold exactly 0.0 and 1.0
    n = 300
    label = (rng.random(n) < 0.5).astype(np.uint8)
    label[:2] = (1, 0)
    base = separated(rng, label, 3)
    base[0, 5], base[0, 6], base[0, 7], base[0, 8] = 0.0, 1.0, 0.0, 1.0
    base[1, 5], base[1, 6] = 0.0, 0.0
    base[2, 5], base[2, 6] = 1.0, 1.0
    add_case(T, fx, "ends01", base, label)

    # ---- separation, perfect and inverted
    n = 60
    label = (np.arange(n) % 3 == 0).astype(np.uint8)
    s = survive(rng.uniform(0.1, 0.4, n) + 0.5 * label)
    exp = add_case(T, fx, "perfect", s, label)
    assert exp[0, 3:7].tolist() == [20.0, 0.0, 40.0, 0.0]
    inv = np.stack([survive(rng.uniform(0.1, 0.4, n) + 0.5 * (1 - label)) for _ in range(2)])
    inv[1, np.argmax(inv[1])] = 1.0
    add_case(T, fx, "inverted", inv, label)
    y = fx["inverted/youden/exp"]
    assert y[0, 0] == np.nextafter(inv[0].max(), 1.0) and y[0, 3] == 0 and y[0, 4] == 0, "youden on inverted scores"
    assert y[1, 0] == 1.0 and y[1, 3] + y[1, 4] == 1

    # ---- a slope-1 run of the ROC (tied pairs of one positive and one negative, P = Nn) whose interior points are dropped: without the
    # dropping, the first maximum of J lies on an interior point that exceeds the kept one by an ulp
    found = None
    for half in range(11, 80):
        for lead in range(1, half - 8):
            run = 8
            label = np.r_[np.ones(lead), np.tile([1, 0], run), np.zeros(half - run), np.ones(half - run - lead)].astype(np.uint8)
            vals = np.sort(rng.uniform(0.05, 0.95, len(label)))[::-1]
            s = vals.copy()
            for r in range(run):
                s[lead + 2 * r + 1] = s[lead + 2 * r]
            s = survive(s)
            if len(np.unique(s)) != len(label) - run:
                continue
            fpr, tpr, thr = roc_curve(label.astype(int), s, drop_intermediate=False)
            full = thr[np.argmax(tpr - fpr)]
            fpr, tpr, thr = roc_curve(label.astype(int), s)
            if thr[np.argmax(tpr - fpr)] != full:
                found = (s, label)
                break
        if found:
            break
    assert found, "no slope-1 case in which the dropping decides"
    add_case(T, fx, "slope1", *found)

    # ---- objective ties
    label = np.array([1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0], dtype=np.uint8)   # f1 = 2/3 at tp, fp = 2, 0 and again at 4, 4
    s = survive(np.linspace(0.9, 0.1, len(label)))
    exp = add_case(T, fx, "tie_recall", s, label)
    size, rec = objective_set(T, s, label, "f1_opt_on_val")
    assert size > 1 and len(np.unique(rec)) > 1 and exp[0, 7] == rec.max() and exp[0, 0] == s[7], (size, rec, exp[0])
    label = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)      # everything positive is best: at 0.0 and at the lowest score
    s = survive(np.linspace(0.9, 0.2, len(label)))
    exp = add_case(T, fx, "tie_tau", s, label)
    size, rec = objective_set(T, s, label, "f1_opt_on_val")
    assert size > 1 and len(np.unique(rec)) == 1 and exp[0, 0] == 0.0, (size, rec, exp[0])

    # ---- one class only: previous_tau finite, NaN, absent
    n = 50
    s = np.stack([survive(rng.uniform(0.05, 0.95, n)) for _ in range(3)])
    for name, value in (("onepos", 1), ("oneneg", 0)):
        exp = add_case(T, fx, name, s, np.full(n, value, dtype=np.uint8), prev=[0.37, np.nan, np.nan], absent=[0, 0, 1])
        assert exp[:, 0].tolist() == [0.37, 0.5, 0.5] and (exp[:, 1] == 0).all() and (exp[:, 2] == 1).all()

    for name in fx:
        if name.endswith("/score") and name not in ("ends01/score", "inverted/score"):
            assert 0.0 < fx[name].min() and fx[name].max() < 1.0, name
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(fx)} arrays)")


if __name__ == "__main__":
    main()
