"""NumPy restatement of the bootstrap metrics (not a test module): what pm_boot_metrics computes, per replicate, from (score, label,
weight) after one descending sort -- the formulas of DESIGN.md "Bootstrap intervals of the test metrics".  The CPU test holds it to
the reference's values of tests/golden/boot_metrics.npz; tools/boot_metrics_bench.py times it beside the device."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boot_metrics.npz")
INTEGER_COLUMNS = (0, 1, 2, 4, 5, 6, 7)   # count, n_pos, n_neg, tp, fp, tn, fn


def load_fixture():
    return dict(np.load(GOLDEN, allow_pickle=False))


def bound(n_frames, ref):
    """|got - ref| <= 64 N 2^-53 max(1, |ref|): a sum of at most N f64 terms, a margin of 64 for the summation order and a 1-ulp log."""
    return 64.0 * n_frames * 2.0 ** -53 * np.maximum(1.0, np.abs(ref))


def assert_matches(got, ref, n_frames, what=""):
    """got / ref [..., 16]: integer-valued entries equal, the others within `bound`, non-finite reference values non-finite alike."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for k in range(16):
        g, r = got[..., k], ref[..., k]
        if k in INTEGER_COLUMNS:
            assert np.array_equal(g, r), (what, k, g, r)
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r)), (what, k, g, r)
        fin = np.isfinite(r)
        err = np.abs(g[fin] - r[fin])
        assert (err <= bound(n_frames, r[fin])).all(), (what, k, float(err.max()), float(bound(n_frames, r[fin]).min()))


def frame_weights(cluster, draws, n_clusters):
    """int64 [R, N]: how often every frame appears in every replicate."""
    out = np.empty((draws.shape[0], len(cluster)), dtype=np.int64)
    for r, d in enumerate(draws):
        out[r] = np.bincount(d[d >= 0], minlength=n_clusters)[cluster]
    return out


def replicate_metrics(score, label, loss, w, tau):
    """The 16 values for frames already in descending score order: score f64, label 0/1 int64, loss f64 per frame, w int64."""
    nan = float("nan")
    tp_cum, fp_cum = np.cumsum(w * label), np.cumsum(w * (1 - label))
    P, Nn = int(tp_cum[-1]), int(fp_cum[-1])
    n = P + Nn
    k = int(np.count_nonzero(score >= tau))
    tp, fp = (int(tp_cum[k - 1]), int(fp_cum[k - 1])) if k else (0, 0)
    tn, fn = Nn - fp, P - tp
    if n == 0:
        return [0.0, 0.0, 0.0, nan, 0.0, 0.0, 0.0, 0.0] + [nan] * 8
    end = np.r_[score[1:] != score[:-1], True]
    TP, FP = tp_cum[end], fp_cum[end]
    dTP, dFP = np.diff(np.r_[0, TP]), np.diff(np.r_[0, FP])
    live = dTP + dFP > 0
    TP, FP, dTP, dFP = TP[live], FP[live], dTP[live], dFP[live]
    auprc = float(np.sum(dTP * (TP / (TP + FP))) / P) if P else 0.0
    auroc = int(np.sum(dFP * (2 * (TP - dTP) + dTP))) / (2.0 * P * Nn) if P and Nn else nan
    recall = tp / P if P else 0.0
    spec = tn / Nn if Nn else 0.0
    precision = tp / (tp + fp) if tp + fp else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    bal = 0.5 * (recall + spec) if P and Nn else (recall if P else spec)
    den = float(P) * float(Nn) * float(tp + fp) * float(tn + fn)
    mcc = (tp * tn - fp * fn) / np.sqrt(den) if den > 0 else 0.0
    return [float(n), float(P), float(Nn), P / n, float(tp), float(fp), float(tn), float(fn), auprc, auroc, recall, precision, f1,
            bal, mcc, float(np.sum(w * loss) / n)]


def boot_metrics_numpy(score, label, tau, cluster, draws, n_clusters=None):
    """f64 [R, M, 16] as ssl4polyp_amd.metrics.bootstrap_binary_metrics returns it."""
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    label = np.asarray(label).astype(np.int64)
    cluster, draws = np.asarray(cluster), np.asarray(draws)
    M, N = score.shape
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (M,))
    C = int(n_clusters) if n_clusters is not None else int(cluster.max()) + 1
    W = frame_weights(cluster, draws, C)
    out = np.empty((draws.shape[0], M, 16))
    for m in range(M):
        order = np.argsort(-score[m], kind="stable")
        s, y = score[m][order], label[order]
        p = np.clip(s, 1e-12, 1.0 - 1e-12)
        loss = -(y * np.log(p) + (1 - y) * np.log(1 - p))
        for r in range(draws.shape[0]):
            out[r, m] = replicate_metrics(s, y, loss, W[r][order], tau[m])
    return out
