"""Host side of the threshold selection (ssl4polyp_amd/metrics.py, pm_select_tau's admission rules, main_finetune's flags) against
tests/golden/thresholds.npz, which holds what the reference's classification/metrics/thresholds.py returned.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import thresholds_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_KEYS = {"policy", "tau", "split", "n_candidates", "tiebreakers", "epoch", "degenerate_val", "notes", "metrics"}
METRIC_KEYS = {"tp", "fp", "tn", "fn", "recall", "precision", "f1", "tpr", "fpr", "youden_j"}


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def cases(fx):
    return sorted(k[:-len("/score")] for k in fx if k.endswith("/score"))


def test_restatement_equals_the_reference_exactly(fx):
    assert tuple(fx["expected_keys"]) == R.EXPECTED and tuple(fx["policies"]) == R.POLICY_NAMES
    checked = 0
    for name in cases(fx):
        for policy in R.POLICY_NAMES:
            rows, cand = R.select_numpy(fx[f"{name}/score"], fx[f"{name}/label"], policy, fx[f"{name}/prev"])
            if f"{name}/{policy}/exp" not in fx:   # youden on one class: the reference raises
                assert policy == "youden" and "both positive and negative" in str(fx[f"{name}/youden/error"])
                assert (rows[:, 2] == 1).all() and np.isnan(rows[:, 0]).all()
                continue
            R.assert_equal(rows[:, R.EXPECTED_COLUMNS], fx[f"{name}/{policy}/exp"], f"{name}/{policy}")
            if policy != "youden":
                R.assert_equal(cand, fx[f"{name}/cand"], f"{name}/{policy} candidates")
            checked += rows.shape[0]
    assert checked >= 4 * 3 * 5


def test_fixture_holds_the_cases_the_kernel_can_get_wrong(fx):
    tile = int(fx["tile"])
    from ssl4polyp_amd import metrics
    assert tile == metrics.SCAN_TILE
    for n in (2, tile - 1, tile, tile + 1, 3 * tile + 5):
        s = fx[f"size{n}/score"]
        assert s.shape == (3, n) and s.dtype == np.float64 and len(np.unique(s[2])) == 1
        if n > tile:   # a tie group lies across the first tile boundary of the sorted order
            srt = np.sort(s[1])[::-1]
            assert srt[tile - 1] == srt[tile]
    ncand = lambda name: fx[f"{name}/f1_opt_on_val/exp"][0, 1]
    uniq = lambda name: len(np.unique(np.r_[0.0, fx[f"{name}/score"][0], 1.0]))
    assert (uniq("u199"), ncand("u199")) == (199, 199) and (uniq("u200"), ncand("u200")) == (200, 200)
    assert (uniq("u201"), ncand("u201")) == (201, 200) and uniq("u1000") > 1000 and ncand("u1000") == 200
    e = fx["ends01/score"]
    assert {0.0, 1.0} <= set(e[0]) and 0.0 in e[1] and 1.0 not in e[1] and 1.0 in e[2] and 0.0 not in e[2]
    assert 0.0 < fx["u201/score"].min() and fx["u201/score"].max() < 1.0
    assert fx["perfect/f1_opt_on_val/exp"][0, 9] == 1.0
    inv, y = fx["inverted/score"], fx["inverted/youden/exp"]
    assert y[0, 0] == np.nextafter(inv[0].max(), 1.0) and y[0, 3] + y[0, 4] == 0 and y[1, 0] == 1.0
    for name in ("onepos", "oneneg"):
        assert np.isfinite(fx[f"{name}/prev"][0]) and np.isnan(fx[f"{name}/prev"][1:]).all() and fx[f"{name}/prev_absent"].tolist() == [0, 0, 1]
        assert fx[f"{name}/f1_opt_on_val/exp"][:, 0].tolist() == [fx[f"{name}/prev"][0], 0.5, 0.5]
    # the slope-1 run: without roc_curve's dropping the first maximum of J is another point
    s, y = fx["slope1/score"][0], fx["slope1/label"].astype(np.int64)
    order = np.argsort(-s, kind="stable")
    end = np.r_[s[order][1:] != s[order][:-1], True]
    tps, fps = np.cumsum(y[order])[end], np.cumsum(1 - y[order])[end]
    J = tps / tps[-1] - fps / fps[-1]
    assert s[order][end][np.argmax(J)] != fx["slope1/youden/exp"][0, 0] and J.max() > 0
    # objective ties: |S0| > 1, decided by recall / by the lower tau
    for name, by_recall in (("tie_recall", True), ("tie_tau", False)):
        rows, cand = R.select_numpy(fx[f"{name}/score"], fx[f"{name}/label"], "f1_opt_on_val")
        c = cand[0][~np.isnan(cand[0])]
        lab, sc = fx[f"{name}/label"].astype(np.int64), fx[f"{name}/score"][0]
        tp = np.array([(lab[sc >= t] == 1).sum() for t in c])
        fp = np.array([(lab[sc >= t] == 0).sum() for t in c])
        f1 = 2 * tp / (2 * tp + fp + (lab.sum() - tp))
        s0 = f1 >= f1.max() - 1e-12
        assert s0.sum() > 1 and (len(np.unique(tp[s0])) > 1) == by_recall


def test_linspace_identity():
    for U in range(201, 6000):
        assert np.array_equal(R.linspace_indices(U), np.linspace(0, U - 1, num=200, dtype=int)), U


def test_names_symbols_and_admission_without_a_gpu():
    import __graft_entry__ as g
    from ssl4polyp_amd import _lib, metrics
    assert "pm_threshold.hip" in g.SOURCES and g.SOURCE_FLAGS["pm_threshold.hip"] == ["-ffp-contract=off"]
    assert metrics.POLICIES == {"f1_opt_on_val": 0, "youden_on_val": 1, "val_opt_youden": 2, "youden": 3}
    assert metrics.TAU_KEYS == R.KEYS and len(metrics.TAU_KEYS) == 16
    assert metrics.format_threshold_key("Dataset", "VAL", "F1_opt_on_val") == "dataset_val_f1_opt_on_val"
    header = open(os.path.join(REPO, "include", "polypmae.h")).read()
    for name in ("pm_select_tau", "pm_select_tau_workspace"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    lib = _lib.load()
    assert lib.pm_select_tau.restype is ctypes.c_int and len(lib.pm_select_tau.argtypes) == 12
    need = ctypes.c_size_t(0)
    assert lib.pm_select_tau_workspace(15840, 30, ctypes.byref(need)) == 0 and need.value >= 15840 * 30 * 16 and need.value % 16 == 0
    assert lib.pm_select_tau_workspace(1, 1, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pm_select_tau_workspace(1 << 20, 256, ctypes.byref(need)) == 0
    for bad in ((0, 1), (1, 0), ((1 << 20) + 1, 1), (10, 257)):
        assert lib.pm_select_tau_workspace(*bad, ctypes.byref(need)) == _lib.PM_ESHAPE, bad
        assert lib.pm_select_tau(None, None, None, None, 0, None, None, *bad, None, 0, None) == _lib.PM_ESHAPE, bad
    assert lib.pm_select_tau_workspace(10, 1, None) == _lib.PM_EINVAL
    # missing buffers, a policy outside 0..3, a workspace that is too small: refused before anything touches a device
    assert lib.pm_select_tau(None, None, None, None, 0, None, None, 10, 1, None, 0, None) == _lib.PM_EINVAL
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.pm_select_tau(p, p, p, p, 4, p, None, 10, 1, p, 512, None) == _lib.PM_EINVAL
    assert lib.pm_select_tau(p, p, p, p, -1, p, None, 10, 1, p, 512, None) == _lib.PM_EINVAL
    assert lib.pm_select_tau(p, p, p, p, 0, p, None, 10, 1, p, 159, None) == _lib.PM_EINVAL
    with pytest.raises(ValueError, match="Unsupported threshold policy"):
        metrics.select_threshold(np.zeros(4), np.zeros(4), "sun_val_frozen")
    with pytest.raises(ValueError, match="Unsupported threshold policy"):
        metrics.threshold_record(np.zeros(16), "best_guess", "d/val", 0)


def test_main_finetune_threshold_flags():
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import metrics
    assert M.SELECTING_POLICIES == tuple(metrics.POLICIES) and M.FROZEN_POLICY not in metrics.POLICIES
    p = M.get_args_parser()
    a = p.parse_args(["--test_csv", "t.csv"])
    assert a.threshold_policy == "none" and a.dataset_name == "dataset" and a.threshold_from is None
    for policy in ("none", "f1_opt_on_val", "youden_on_val", "val_opt_youden", "youden", "sun_val_frozen"):
        assert p.parse_args(["--test_csv", "t.csv", "--threshold_policy", policy]).threshold_policy == policy
    b = p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "sun_val_frozen", "--threshold_from", "c.pth", "--dataset_name", "SUN"])
    assert b.threshold_from == "c.pth" and b.dataset_name == "SUN"
    with pytest.raises(SystemExit):
        p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "best_guess"])
    # refusals before anything touches a device
    with pytest.raises(SystemExit, match="num_classes 2"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "youden", "--num_classes", "3"]))
    with pytest.raises(SystemExit, match="threshold_from"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "sun_val_frozen"]))
    with pytest.raises(SystemExit, match="val_csv"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "youden"]))


def test_threshold_record_has_the_reference_keys(fx):
    from ssl4polyp_amd.metrics import TAU_KEYS, threshold_record
    rows, cand = R.select_numpy(fx["u201/score"], fx["u201/label"], "f1_opt_on_val")
    rec = threshold_record(rows[0], "F1_opt_on_val", "sun_full/val", 7, candidates=cand[0])
    exp = dict(zip(R.EXPECTED, fx["u201/f1_opt_on_val/exp"][0]))
    assert set(rec) == RECORD_KEYS | {"candidates"} and set(rec["metrics"]) == METRIC_KEYS
    assert rec["policy"] == "f1_opt_on_val" and rec["split"] == "sun_full/val" and rec["epoch"] == 7 and type(rec["epoch"]) is int
    assert rec["tau"] == exp["tau"] and type(rec["tau"]) is float and rec["n_candidates"] == 200 and type(rec["n_candidates"]) is int
    assert rec["tiebreakers"] == ["higher_recall", "lower_tau"] and rec["degenerate_val"] is False and rec["notes"] == {}
    assert rec["metrics"] == {k: exp[k] for k in METRIC_KEYS} and all(type(v) is float for v in rec["metrics"].values())
    assert rec["candidates"] == fx["u201/cand"][0].tolist() and len(rec["candidates"]) == 200
    assert set(threshold_record(rows[0], "f1_opt_on_val", "x/val", 0)) == RECORD_KEYS
    # one class only: carried forward, or the default; youden raises the reference's error
    rows, _ = R.select_numpy(fx["onepos/score"], fx["onepos/label"], "youden_on_val", fx["onepos/prev"])
    recs = [threshold_record(r, "youden_on_val", "x/val", 0) for r in rows]
    assert [r["notes"] for r in recs] == [{"carried_forward": True}, {"default_tau": 0.5}, {"default_tau": 0.5}]
    assert all(r["degenerate_val"] is True and r["n_candidates"] == 0 for r in recs) and recs[0]["tau"] == fx["onepos/prev"][0]
    rows, _ = R.select_numpy(fx["onepos/score"], fx["onepos/label"], "youden")
    with pytest.raises(ValueError, match=str(fx["onepos/youden/error"])):
        threshold_record(rows[0], "youden", "x/val", 0)
    assert len(TAU_KEYS) == rows.shape[1]
