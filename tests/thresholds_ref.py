"""NumPy restatement of the threshold selection (not a test module): what pm_select_tau computes from (score, label) after one
descending sort -- DESIGN.md "Threshold selection on the device".  The CPU test holds it to the values the reference's
classification/metrics/thresholds.py returned (tests/golden/thresholds.npz); tools/select_tau_bench.py times it beside the device."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thresholds.npz")
POLICY_NAMES = ("f1_opt_on_val", "youden_on_val", "val_opt_youden", "youden")
KEYS = ("tau", "n_candidates", "degenerate", "objective", "tp", "fp", "tn", "fn", "recall", "precision", "f1", "tpr", "fpr",
        "youden_j", "n_unique", "index")
# the fixture's expected columns: everything the reference returns (tau, n_candidates, degenerate_val, the metrics dict)
EXPECTED = ("tau", "n_candidates", "degenerate", "tp", "fp", "tn", "fn", "recall", "precision", "f1", "tpr", "fpr", "youden_j")
EXPECTED_COLUMNS = [KEYS.index(k) for k in EXPECTED]
MAX_CANDIDATES = 200
EPS = 1e-12


def load_fixture():
    return dict(np.load(GOLDEN, allow_pickle=False))


def linspace_indices(U):
    """np.linspace(0, U - 1, num=200, dtype=int) for U > 200, one f64 product per index."""
    step = np.float64(U - 1) / np.float64(MAX_CANDIDATES - 1)
    idx = np.floor(np.arange(MAX_CANDIDATES, dtype=np.float64) * step).astype(np.int64)
    idx[-1] = U - 1
    return idx


def _ratio(num, den):
    return num / den if den > 0 else 0.0


def _row(tau, n_cand, degenerate, objective, tp, fp, P, Nn, n_unique, index):
    tn, fn = Nn - fp, P - tp
    rec, fpr = _ratio(tp, tp + fn), _ratio(fp, fp + tn)
    return [tau, float(n_cand), float(degenerate), objective, float(tp), float(fp), float(tn), float(fn), rec, _ratio(tp, tp + fp),
            _ratio(2 * tp, 2 * tp + fp + fn), rec, fpr, rec - fpr, n_unique, float(index)]


def select_one(score, label, policy, previous_tau=None):
    """(the 16 values in KEYS order, the candidate list) of one run."""
    nan = float("nan")
    score = np.asarray(score, dtype=np.float64)
    order = np.argsort(-score, kind="stable")
    s, y = score[order], np.asarray(label).astype(np.int64)[order]
    tp_cum, fp_cum = np.cumsum(y), np.cumsum(1 - y)
    P, Nn = int(tp_cum[-1]), int(fp_cum[-1])
    end = np.r_[s[1:] != s[:-1], True]
    ps, ptp, pfp = s[end], tp_cum[end], fp_cum[end]   # the distinct scores, descending, and the prefix counts at their group ends
    D = len(ps)
    youden = policy == "youden"
    if P == 0 or Nn == 0:
        if youden:
            return _row(nan, 0, 1, nan, 0, 0, P, Nn, nan, -1), []
        carried = previous_tau is not None and math.isfinite(previous_tau)
        tau = float(previous_tau) if carried else 0.5
        k = int(np.count_nonzero(s >= tau))
        return _row(tau, 0, 1, nan, int(tp_cum[k - 1]) if k else 0, int(fp_cum[k - 1]) if k else 0, P, Nn, nan, -2 if carried else -1), [tau]
    if not youden:
        has0, has1 = ps[-1] == 0.0, ps[0] == 1.0
        U = D + (not has0) + (not has1)
        idx = np.arange(U) if U <= MAX_CANDIDATES else linspace_indices(U)
        cand, tp, fp = np.empty(len(idx)), np.empty(len(idx), dtype=np.int64), np.empty(len(idx), dtype=np.int64)
        for k, i in enumerate(idx):
            if i == 0 and not has0:
                cand[k], tp[k], fp[k] = 0.0, P, Nn
            elif i == U - 1 and not has1:
                cand[k], tp[k], fp[k] = 1.0, 0, 0
            else:
                g = D - 1 - (i - (not has0))
                cand[k], tp[k], fp[k] = ps[g], ptp[g], pfp[g]
        rec = tp / P
        with np.errstate(invalid="ignore"):
            obj = np.where(2 * tp + fp + (P - tp) > 0, 2 * tp / (2 * tp + fp + (P - tp)), 0.0) if policy == "f1_opt_on_val" else rec - fp / Nn
        s0 = obj >= obj.max() - EPS
        s1 = s0 & (rec >= rec[s0].max() - EPS)
        k = int(np.flatnonzero(s1)[0])
        return _row(float(cand[k]), len(idx), 0, float(obj[k]), int(tp[k]), int(fp[k]), P, Nn, float(U), k), cand.tolist()
    keep = np.ones(D, dtype=bool)
    if D > 2:
        keep[1:-1] = (np.diff(pfp, 2) != 0) | (np.diff(ptp, 2) != 0)
    J = np.where(keep, ptp / P - pfp / Nn, -np.inf)
    g = int(np.argmax(J))
    n_points = int(keep.sum()) + 1
    if not J[g] > 0.0:   # the curve's first point (0, 0) at +inf
        tau = float(np.nextafter(ps[0], 1.0))
        at = ps[0] >= tau
        return _row(tau, n_points, 0, 0.0, int(ptp[0]) if at else 0, int(pfp[0]) if at else 0, P, Nn, float(D), 0), []
    return _row(float(ps[g]), n_points, 0, float(J[g]), int(ptp[g]), int(pfp[g]), P, Nn, float(D), g + 1), []


def select_numpy(score, label, policy, previous_tau=None):
    """(f64 [M, 16], f64 [M, 200] NaN-padded) as ssl4polyp_amd.metrics.select_threshold(..., return_candidates=True) returns them."""
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    M = score.shape[0]
    prev = np.full(M, np.nan) if previous_tau is None else np.broadcast_to(np.asarray(previous_tau, dtype=np.float64), (M,))
    rows, cands = np.empty((M, 16)), np.full((M, MAX_CANDIDATES), np.nan)
    for m in range(M):
        row, c = select_one(score[m], label, policy, float(prev[m]))
        rows[m] = row
        cands[m, :len(c)] = c
    return rows, cands


def assert_equal(got, want, what=""):
    """Bit-for-bit apart from NaN, which must be NaN on both sides."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, got, want)
