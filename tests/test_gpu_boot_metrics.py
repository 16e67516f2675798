"""pm_boot_metrics on the device (ssl4polyp_amd/metrics.py) against tests/golden/boot_metrics.npz: every expected value is what the
reference's compute_binary_metrics (scikit-learn) returned on the gathered sample of that replicate.  Integer-valued entries must be
equal, the others within 64 N 2^-53 max(1, |ref|) (boot_metrics_ref.bound: under 3e-11 at these sizes, while one mishandled tie or
weight moves a metric by at least 1 / (P Nn) > 1e-7), non-finite values must match as non-finite."""
import json

import numpy as np
import pytest
import torch

import boot_metrics_ref as B
from pack_files import write_pack

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx():
    return B.load_fixture()


def _run(fx, name, draws, runs=slice(None), score=None, tau=None, **kw):
    from ssl4polyp_amd.metrics import bootstrap_binary_metrics
    score = fx[f"{name}/score"] if score is None else score
    tau = fx[f"{name}/tau"] if tau is None else tau
    out = bootstrap_binary_metrics(torch.from_numpy(score[runs].astype(np.float64)).to(DEV), fx[f"{name}/label"], tau[runs],
                                   fx[f"{name}/cluster"], draws, **kw)
    assert out.is_cuda and out.dtype == torch.float64
    return out


def test_scan_tile_is_the_fixtures(fx):
    from ssl4polyp_amd import metrics
    assert metrics.SCAN_TILE == int(fx["tile"]) and tuple(fx["keys"]) == metrics.METRIC_KEYS


@pytest.mark.parametrize("kind", ["cont", "round", "equal"])
@pytest.mark.parametrize("offset", ["two", "T-1", "T", "T+1", "3T+5"])
def test_sizes_around_the_tile(fx, offset, kind):
    """R = 16 stratified replicates; three runs with tau below / inside / above the score range, together (M = 3) and alone (M = 1)."""
    from ssl4polyp_amd.metrics import SCAN_TILE as T
    n = {"two": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[offset]
    score, tau, ref = fx[f"size{n}/{kind}/score"], fx[f"size{n}/{kind}/tau"], fx[f"size{n}/{kind}/ref"]
    assert score.shape == (3, n) and ref.shape == (16, 3, 16)
    s64 = score.astype(np.float64)
    assert tau[0] < s64[0].min() and s64[1].min() <= tau[1] <= s64[1].max() and tau[2] > s64[2].max()
    if kind == "round" and n > T:   # a tie group lies across a tile boundary of the sorted order
        assert all(np.sort(s64[m])[::-1][T - 1] == np.sort(s64[m])[::-1][T] for m in range(3))
    draws = fx[f"size{n}/draws"]
    got = _run(fx, f"size{n}", draws, score=score, tau=tau).cpu().numpy()
    B.assert_matches(got, ref, n, f"size{n}/{kind} M=3")
    if kind == "equal":
        both = (ref[..., 1] > 0) & (ref[..., 2] > 0)
        assert both.all() and (got[..., 9] == 0.5).all()
    for m in range(3):
        alone = _run(fx, f"size{n}", draws, runs=slice(m, m + 1), score=score, tau=tau).cpu().numpy()
        B.assert_matches(alone, ref[:, m:m + 1], n, f"size{n}/{kind} M=1 run {m}")
        assert np.array_equal(alone[:, 0], got[:, m], equal_nan=True)   # a run's values do not depend on its neighbours


def test_multiplicities_above_255_and_65535(fx):
    draws, ref = fx["mult/draws"], fx["mult/ref"]
    assert (draws[0, :300] == draws[0, 0]).all() and (draws[0, 300:] == -1).all() and int(fx["a/cluster"].max()) + 1 >= 300
    assert ref[0, 0, 0] >= 300 and ref[4, 0, 0] > 65535
    got = _run(fx, "a", draws).cpu().numpy()
    B.assert_matches(got, ref, len(fx["a/label"]), "mult")


def test_per_frame_clusters_absent_classes_and_weightless_top_group(fx):
    draws, ref = fx["frame/draws"], fx["frame/ref"]
    assert draws.shape[0] == 64
    top = np.flatnonzero(fx["frame/score"][0] == fx["frame/score"][0].max())
    assert any(not np.isin(top, d).any() for d in draws) and (ref[:, 0, 1] == 0).any() and (ref[:, 0, 2] == 0).any()
    got = _run(fx, "frame", draws).cpu().numpy()
    B.assert_matches(got, ref, len(fx["frame/label"]), "frame")


def test_two_runs_37_replicates_bit_reproducible_and_chunk_independent(fx):
    from ssl4polyp_amd.metrics import bootstrap_binary_metrics, build_cluster_set, draw_cluster_samples
    for name in ("a", "b"):
        draws = fx[f"{name}/draws"]
        assert draws.shape[0] == 37
        one = _run(fx, name, draws, chunk=64)
        B.assert_matches(one.cpu().numpy(), fx[f"{name}/ref"], len(fx[f"{name}/label"]), name)
        again = _run(fx, name, draws, chunk=64)
        assert torch.equal(one.view(torch.int64), again.view(torch.int64))      # the same call twice: identical bits
        parts = _run(fx, name, draws, chunk=16)
        assert torch.equal(one.view(torch.int64), parts.view(torch.int64))      # one chunk of 37 == chunks of 16, 16, 5
    # the whole host path: rows -> clusters -> draws -> replicates, from the seed alone
    rows = [{"case_id": str(c)} for c in fx["a/case_id"]]
    cs = build_cluster_set(rows, fx["a/label"].tolist())
    draws = draw_cluster_samples([cs, build_cluster_set([{"case_id": str(c)} for c in fx["b/case_id"]], fx["b/label"].tolist())],
                                 np.random.default_rng(int(fx["ab/seed"])), 37)[0]
    got = bootstrap_binary_metrics(fx["a/score"].astype(np.float64), fx["a/label"], 0.5, cs.cluster, draws, n_clusters=cs.n_clusters)
    B.assert_matches(got.cpu().numpy(), fx["a/ref"], len(rows), "a from the seed")


def test_binary_metrics_is_the_single_evaluation(fx):
    from ssl4polyp_amd.metrics import METRIC_KEYS, binary_metrics
    n = len(fx["a/label"])
    for m in range(2):
        got = binary_metrics(fx["a/score"][m].astype(np.float64), fx["a/label"], 0.5)
        assert tuple(got) == METRIC_KEYS
        B.assert_matches(np.array(list(got.values())), fx["a/single"][m], n, f"a/single run {m}")


def test_scalar_tau_is_compared_in_f64(fx):
    """A float tau that no f32 holds, equal to one of the f64 scores: the frame at tau is predicted positive (score >= tau), as the
    reference decides against float(tau).  Rounded to f32 the threshold lies above that score and the frame's weight leaves tp or fp
    in every replicate that holds it.  Expected values: the NumPy restatement (held to the reference by the CPU test), same bound."""
    from ssl4polyp_amd.metrics import binary_metrics, bootstrap_binary_metrics
    label, cluster, draws = fx["a/label"], fx["a/cluster"], fx["a/draws"]
    n = len(label)
    score = np.clip(fx["a/score"].astype(np.float64) + np.random.default_rng(11).uniform(-2.0 ** -26, 2.0 ** -26, (2, n)), 0.0, 1.0)
    drawn = np.bincount(draws[draws >= 0], minlength=int(cluster.max()) + 1)[cluster] > 0
    up = [float(t) for t in score[0][drawn] if float(np.float32(t)) > t and 0.3 < t < 0.7]
    assert up, "no score that f32 rounds upwards"
    tau = up[0]
    assert float(np.float32(tau)) != tau and (score[0] == tau).sum() == 1
    ref = B.boot_metrics_numpy(score, label, tau, cluster, draws)
    moved = B.boot_metrics_numpy(score, label, float(np.float32(tau)), cluster, draws)
    assert (ref[:, 0, 4] + ref[:, 0, 5] != moved[:, 0, 4] + moved[:, 0, 5]).any()   # the case tells the two thresholds apart
    got = bootstrap_binary_metrics(score, label, tau, cluster, draws).cpu().numpy()
    B.assert_matches(got, ref, n, "scalar f64 tau")
    single = B.boot_metrics_numpy(score[0], label, tau, np.zeros(n, dtype=np.int32), np.zeros((1, 1), dtype=np.int32))[0, 0]
    one = binary_metrics(score[0], label, tau)
    B.assert_matches(np.array(list(one.values())), single, n, "scalar f64 tau, single")
    assert one["tp"] + one["fp"] == (score[0] >= tau).sum()


def test_main_finetune_logs_metrics_and_intervals(tmp_path):
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import metrics as MX
    csv_path, roots, _, labels = write_pack(str(tmp_path / "pack"))
    (key, root), = roots.items()
    common = ["--val_csv", csv_path, "--test_csv", csv_path, "--root", f"{key}={root}", "--batch_size", "8", "--precision", "bf16",
              "--num_workers", "0", "--no_pin_mem", "--seed", "3"]
    args = M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "out"), "--metrics", "--bootstrap", "8"])
    model, val_logits = M.run(args)
    del model
    val, test = [json.loads(ln) for ln in open(tmp_path / "out" / "log.txt")]
    assert val_logits.shape == (10, 2) and test["test_samples"] == 10 and test["bootstrap"] == 8
    want = MX.binary_metrics(MX.positive_probs(val_logits.to(DEV)), labels, 0.5)
    assert want["count"] == 10 and want["n_pos"] == 5 and np.isfinite(list(want.values())).all()
    # val and test are the same ten files through the same evaluation path: the returned logits are the test logits
    assert test["test_loss"] == val["val_loss"]
    assert val["val_metrics"] == want and test["test_metrics"] == want
    assert set(test["ci_lower"]) == set(test["ci_upper"]) == set(MX.REPORTED_KEYS) and "ci_lower" not in val
    for k in MX.REPORTED_KEYS:
        lo, hi = test["ci_lower"][k], test["ci_upper"][k]
        assert np.isfinite(lo) and np.isfinite(hi) and lo <= hi, (k, lo, hi)
    # without the flags the records are what they were
    plain = M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "plain")])
    M.run(plain)
    val0, test0 = [json.loads(ln) for ln in open(tmp_path / "plain" / "log.txt")]
    assert set(val0) == {"val_loss"} and set(test0) == {"test_loss", "test_samples"}
    assert val0["val_loss"] == val["val_loss"] and test0["test_loss"] == test["test_loss"]
    # --bootstrap alone adds the intervals and nothing else: the metrics come with --metrics
    only = M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "only"), "--bootstrap", "8"])
    M.run(only)
    val1, test1 = [json.loads(ln) for ln in open(tmp_path / "only" / "log.txt")]
    assert set(val1) == {"val_loss"} and set(test1) == {"test_loss", "test_samples", "bootstrap", "ci_lower", "ci_upper"}
    assert test1["ci_lower"] == test["ci_lower"] and test1["ci_upper"] == test["ci_upper"]
