"""pm_select_tau on the device (ssl4polyp_amd/metrics.select_threshold) against tests/golden/thresholds.npz: every expected value is
what the reference's classification/metrics/thresholds.py returned.  Everything is compared for EQUALITY: tau is one of the scores
(or 0, 1, a carried value, nextafter of a score), the counts are integers, and recall, precision, f1, fpr are each one IEEE f64
division of exact integers, youden_j one subtraction of two of them -- the derived bound is zero, not a tolerance."""
import json

import numpy as np
import pytest
import torch

import thresholds_ref as R
from pack_files import write_pack

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RECORD_KEYS = {"policy", "tau", "split", "n_candidates", "tiebreakers", "epoch", "degenerate_val", "notes", "metrics"}


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def _cases(fx):
    return sorted(k[:-len("/score")] for k in fx if k.endswith("/score"))


def _select(fx, name, policy, runs=slice(None), candidates=True):
    from ssl4polyp_amd.metrics import select_threshold
    out = select_threshold(torch.from_numpy(fx[f"{name}/score"][runs]).to(DEV), fx[f"{name}/label"], policy,
                           previous_tau=fx[f"{name}/prev"][runs], return_candidates=candidates)
    rows = out[0] if candidates else out
    assert rows.is_cuda and rows.dtype == torch.float64 and rows.shape[1] == 16
    return out


@pytest.mark.parametrize("policy", R.POLICY_NAMES)
def test_every_fixture_case_equals_the_reference(fx, policy):
    from ssl4polyp_amd import metrics
    assert metrics.SCAN_TILE == int(fx["tile"]) and metrics.TAU_KEYS == R.KEYS
    for name in _cases(fx):
        rows, cand = _select(fx, name, policy)
        rows, cand = rows.cpu().numpy(), cand.cpu().numpy()
        print(name, policy, rows[:, :8].tolist())
        if f"{name}/{policy}/exp" not in fx:   # youden on one class: no answer, and the record raises the reference's error
            assert policy == "youden" and (rows[:, 2] == 1).all() and np.isnan(rows[:, 0]).all() and np.isnan(cand).all()
            with pytest.raises(ValueError, match=str(fx[f"{name}/youden/error"])):
                metrics.threshold_record(rows[0], policy, "x/val", 0)
            continue
        R.assert_equal(rows[:, R.EXPECTED_COLUMNS], fx[f"{name}/{policy}/exp"], f"{name}/{policy}")
        want_rows, want_cand = R.select_numpy(fx[f"{name}/score"], fx[f"{name}/label"], policy, fx[f"{name}/prev"])
        R.assert_equal(rows, want_rows, f"{name}/{policy} objective, n_unique, index")   # the columns the reference does not return
        R.assert_equal(cand, fx[f"{name}/cand"] if policy != "youden" else want_cand, f"{name}/{policy} candidates")
        # previous_tau absent = NaN
        if fx[f"{name}/prev_absent"].any():
            from ssl4polyp_amd.metrics import select_threshold
            m = int(np.flatnonzero(fx[f"{name}/prev_absent"])[0])
            alone = select_threshold(fx[f"{name}/score"][m], fx[f"{name}/label"], policy).cpu().numpy()
            R.assert_equal(alone[:, R.EXPECTED_COLUMNS], fx[f"{name}/{policy}/exp"][m:m + 1], f"{name}/{policy} no previous_tau")


def test_runs_together_and_alone_same_bits(fx):
    tile = int(fx["tile"])
    for name in (f"size{3 * tile + 5}", f"size{tile + 1}", "ends01"):
        for policy in ("f1_opt_on_val", "youden_on_val", "youden"):
            rows, cand = _select(fx, name, policy)
            again, cand2 = _select(fx, name, policy)
            assert torch.equal(rows.view(torch.int64), again.view(torch.int64)) and torch.equal(cand.view(torch.int64), cand2.view(torch.int64))
            for m in range(3):
                alone, c1 = _select(fx, name, policy, runs=slice(m, m + 1))
                assert torch.equal(alone.view(torch.int64)[0], rows.view(torch.int64)[m]), (name, policy, m)
                assert torch.equal(c1.view(torch.int64)[0], cand.view(torch.int64)[m])
            assert torch.equal(_select(fx, name, policy, candidates=False).view(torch.int64), rows.view(torch.int64))


def test_tau_stays_on_the_device_and_feeds_the_bootstrap(fx):
    from ssl4polyp_amd.metrics import METRIC_KEYS, bootstrap_binary_metrics
    name = "u1000"
    score, label = fx[f"{name}/score"], fx[f"{name}/label"]
    n = score.shape[1]
    for policy in ("f1_opt_on_val", "youden"):
        rows = _select(fx, name, policy, candidates=False)
        tau = rows[:, 0]
        assert tau.is_cuda and tau.dtype == torch.float64
        out = bootstrap_binary_metrics(torch.from_numpy(score).to(DEV), label, tau, np.zeros(n, dtype=np.int32),
                                       np.zeros((1, 1), dtype=np.int32), n_clusters=1)
        got = dict(zip(METRIC_KEYS, out[0, 0].tolist()))
        assert got["tp"] + got["fp"] == (score[0] >= tau.item()).sum() and got["count"] == n
        assert [got[k] for k in ("tp", "fp", "tn", "fn")] == rows[0, 4:8].tolist()


def test_order_entries_outside_the_range_are_no_frames(fx):
    """The C entry with an `order` whose tail names no frame (-1, N, the int32 extremes): the result is that of the frames it does
    name -- nothing outside the buffers is read, and the padding is no score, no class and no ROC point."""
    import ctypes
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.metrics import TAU_KEYS
    lib = _lib.load()
    for name in ("u201", "ends01"):
        score, label = fx[f"{name}/score"][:1], fx[f"{name}/label"]
        n, pad = score.shape[1], [-1, score.shape[1], 2 ** 31 - 1, -2 ** 31, score.shape[1] + 7]
        keep = n - len(pad)
        order = np.r_[np.argsort(-score[0, :keep], kind="stable"), pad].astype(np.int32)[None]
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
             (("score", score), ("order", order), ("label", label), ("prev", np.full(1, np.nan)))}
        need = ctypes.c_size_t(0)
        assert lib.pm_select_tau_workspace(n, 1, ctypes.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        for policy in ("f1_opt_on_val", "youden_on_val", "youden"):
            out = torch.empty((1, len(TAU_KEYS)), dtype=torch.float64, device=DEV)
            cand = torch.empty((1, 200), dtype=torch.float64, device=DEV)
            st = lib.pm_select_tau(d["score"].data_ptr(), d["order"].data_ptr(), d["label"].data_ptr(), d["prev"].data_ptr(),
                                   R.POLICY_NAMES.index(policy), out.data_ptr(), cand.data_ptr(), n, 1, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream(DEV).cuda_stream)
            assert st == 0
            want, want_cand = R.select_numpy(score[:, :keep], label[:keep], policy)
            R.assert_equal(out.cpu().numpy(), want, f"{name}/{policy} padded order")
            R.assert_equal(cand.cpu().numpy(), want_cand, f"{name}/{policy} padded order, candidates")


def _log(path):
    return [json.loads(ln) for ln in open(path)]


def test_main_finetune_selects_carries_and_freezes_tau(tmp_path):
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import metrics as MX
    csv_path, roots, _, labels = write_pack(str(tmp_path / "pack"))
    (key, root), = roots.items()
    data = ["--root", f"{key}={root}", "--batch_size", "8", "--precision", "bf16", "--num_workers", "0", "--no_pin_mem", "--seed", "3"]
    common = ["--val_csv", csv_path, "--test_csv", csv_path] + data
    policy = ["--threshold_policy", "f1_opt_on_val"]
    # ---- a selecting run: val and test are the same ten files
    _, val_logits = M.run(M.get_args_parser().parse_args(common + policy + ["--output_dir", str(tmp_path / "sel"), "--metrics", "--bootstrap", "8"]))
    val, test = _log(tmp_path / "sel" / "log.txt")
    probs = MX.positive_probs(val_logits.to(DEV))
    row = MX.select_threshold(probs, labels, "f1_opt_on_val")
    assert row.is_cuda and val["val_tau"] == test["test_tau"] == row[0, 0].item()
    want = R.select_numpy(probs.cpu().numpy(), labels, "f1_opt_on_val")[0]
    R.assert_equal(row.cpu().numpy(), want, "val logits")
    rec = val["val_threshold"]
    assert set(rec) == RECORD_KEYS and rec["split"] == "dataset/val" and rec["policy"] == "f1_opt_on_val" and rec["tau"] == val["val_tau"]
    assert rec["tiebreakers"] == ["higher_recall", "lower_tau"] and rec["degenerate_val"] is False and rec["epoch"] == 0
    n_at = int((probs.cpu().numpy() >= test["test_tau"]).sum())
    assert test["test_metrics_at_tau"]["tp"] + test["test_metrics_at_tau"]["fp"] == n_at
    assert val["val_metrics_at_tau"] == test["test_metrics_at_tau"] and rec["metrics"]["tp"] == test["test_metrics_at_tau"]["tp"]
    assert set(test["test_metrics"]) == set(test["test_metrics_at_tau"]) == set(MX.METRIC_KEYS) and test["bootstrap"] == 8
    at_tau = MX.binary_metrics(probs, labels, test["test_tau"])
    assert test["test_metrics_at_tau"] == dict(zip(at_tau, M.strict(at_tau.values())))
    # ---- one epoch of training: the checkpoint holds the threshold under the reference's key
    import csv
    from pack_files import encode, frame
    out, troot = tmp_path / "train", tmp_path / "tdata"
    (troot / "img").mkdir(parents=True)
    with open(tmp_path / "train.csv", "w", newline="") as f:   # sixteen frames a training batch can be cropped from
        w = csv.writer(f)
        w.writerow(["frame_path", "label", "store_id", "variant"])
        for i in range(16):
            (troot / "img" / f"{i:02d}.jpg").write_bytes(encode(frame(64, 64, 200 + i), subsampling=2, quality=90))
            w.writerow([f"img/{i:02d}.jpg", (i // 2) % 2, "frames", "clean"])
    M.run(M.get_args_parser().parse_args(["--train_csv", str(tmp_path / "train.csv"), "--val_csv", str(tmp_path / "train.csv"), "--root",
                                          f"frames={troot}"] + data[2:] + policy +
                                         ["--output_dir", str(out), "--epochs", "1", "--finetune_mode", "head+1"]))
    epoch, = _log(out / "log.txt")
    ckpt = torch.load(str(out / "ckpts" / "finetune_e1.pth"), map_location="cpu", weights_only=False)
    name = "dataset_val_f1_opt_on_val"
    assert set(ckpt["thresholds"]) == set(ckpt["threshold_records"]) == {name}
    assert ckpt["thresholds"][name] == epoch["val_tau"] == ckpt["threshold_records"][name]["tau"]
    assert ckpt["threshold_records"][name] == epoch["val_threshold"] and epoch["val_threshold"]["epoch"] == 1
    assert "val_metrics_at_tau" not in epoch and "val_metrics" not in epoch   # they come with --metrics
    # ---- a frozen run reuses that tau
    frozen = ["--threshold_policy", "sun_val_frozen", "--threshold_from", str(out / "ckpts" / "finetune_e1.pth")]
    M.run(M.get_args_parser().parse_args(["--test_csv", csv_path] + data + frozen + ["--output_dir", str(tmp_path / "frozen"), "--metrics"]))
    test2, = _log(tmp_path / "frozen" / "log.txt")
    assert test2["test_tau"] == epoch["val_tau"] and test2["test_threshold"]["source_key"] == name
    assert test2["test_metrics_at_tau"]["tp"] + test2["test_metrics_at_tau"]["fp"] <= 10
    plain_ckpt = tmp_path / "none.pth"
    torch.save({"model_state_dict": {}}, str(plain_ckpt))
    with pytest.raises(SystemExit, match="exactly one"):
        M.run(M.get_args_parser().parse_args(["--test_csv", csv_path] + data + frozen[:3] + [str(plain_ckpt), "--output_dir", str(tmp_path / "bad")]))
    # ---- without the new flags the records are what they were
    M.run(M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "plain")]))
    val0, test0 = _log(tmp_path / "plain" / "log.txt")
    assert set(val0) == {"val_loss"} and set(test0) == {"test_loss", "test_samples"}
    assert val0["val_loss"] == val["val_loss"] and test0["test_loss"] == test["test_loss"]
