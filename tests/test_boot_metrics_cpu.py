"""Host side of the bootstrap metrics (ssl4polyp_amd/metrics.py, pm_boot_metrics' admission rules, main_finetune's flags) against
tests/golden/boot_metrics.npz, which holds what the reference's common_metrics (build_cluster_set, sample_cluster_ids,
compute_binary_metrics over scikit-learn) returned: clusters, draws and the 16 values of every replicate.  No GPU."""
import ctypes

import numpy as np
import pytest

import boot_metrics_ref as B


@pytest.fixture(scope="module")
def fx():
    return B.load_fixture()


def _rows(fx, name):
    return [{"frame_id": str(f), "case_id": str(c)} for f, c in zip(fx[f"{name}/frame_id"], fx[f"{name}/case_id"])]


def test_build_cluster_set_equals_the_reference_clusters(fx):
    from ssl4polyp_amd.metrics import build_cluster_set
    for name in ("a", "b"):
        rows = _rows(fx, name)
        assert any(r["case_id"] == "" for r in rows)   # rows without a key are clusters of their own
        cs = build_cluster_set(rows, fx[f"{name}/label"].tolist(), "case_id", "case_id")
        assert cs.n_pos == int(fx[f"{name}/n_pos_clusters"]) and cs.n_clusters == int(fx[f"{name}/cluster"].max()) + 1
        np.testing.assert_array_equal(cs.cluster, fx[f"{name}/cluster"])
        # a missing column and a callable key follow the same rule
        np.testing.assert_array_equal(build_cluster_set([{k: v for k, v in r.items() if v != ""} for r in rows],
                                                        fx[f"{name}/label"].tolist(), lambda r: r.get("case_id"),
                                                        lambda r: r.get("case_id")).cluster, fx[f"{name}/cluster"])


def test_build_cluster_set_takes_keys_as_the_reference_does():
    """`key(record) or <own cluster>`: nothing is stripped, so blanks are a key and differ from the same name without them; only
    a false value is missing."""
    from ssl4polyp_amd.metrics import build_cluster_set
    keys = ["a", " a", "  ", "  ", "", None, "a", "a", " a", ""]
    labels = [1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    cs = build_cluster_set([{"case_id": k} for k in keys], labels)
    # positives: "a" 0, " a" 1, "  " 2 (twice), two frames of their own 3, 4; negatives: "a" 5 (twice), " a" 6, one of its own 7
    assert cs.cluster.tolist() == [0, 1, 2, 2, 3, 4, 5, 5, 6, 7] and (cs.n_pos, cs.n_neg) == (5, 3)


def test_draw_cluster_samples_equals_the_recorded_draws_of_two_interleaved_sets(fx):
    from ssl4polyp_amd.metrics import build_cluster_set, draw_cluster_samples
    sets = [build_cluster_set(_rows(fx, n), fx[f"{n}/label"].tolist()) for n in ("a", "b")]
    R = fx["a/draws"].shape[0]
    got = draw_cluster_samples(sets, np.random.default_rng(int(fx["ab/seed"])), R)
    for g, n in zip(got, ("a", "b")):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, fx[f"{n}/draws"])
    # one set alone: the first set's draws differ from the interleaved ones after replicate 0 (the generator is shared)
    alone = draw_cluster_samples(sets[0], np.random.default_rng(int(fx["ab/seed"])), R)
    np.testing.assert_array_equal(alone[0], fx["a/draws"][0])
    assert not np.array_equal(alone[1], fx["a/draws"][1])


def test_numpy_restatement_meets_the_reference(fx):
    tile = int(fx["tile"])
    sizes = (2, tile - 1, tile, tile + 1, 3 * tile + 5)
    for n in sizes:
        for kind in ("cont", "round", "equal"):
            got = B.boot_metrics_numpy(fx[f"size{n}/{kind}/score"], fx[f"size{n}/label"], fx[f"size{n}/{kind}/tau"],
                                       fx[f"size{n}/cluster"], fx[f"size{n}/draws"])
            B.assert_matches(got, fx[f"size{n}/{kind}/ref"], n, f"size{n}/{kind}")
    for name, draws, ref in (("a", "a/draws", "a/ref"), ("b", "b/draws", "b/ref"), ("a", "mult/draws", "mult/ref"),
                             ("frame", "frame/draws", "frame/ref")):
        got = B.boot_metrics_numpy(fx[f"{name}/score"], fx[f"{name}/label"], fx[f"{name}/tau"], fx[f"{name}/cluster"], fx[draws])
        B.assert_matches(got, fx[ref], len(fx[f"{name}/label"]), ref)
    n = len(fx["a/label"])
    single = B.boot_metrics_numpy(fx["a/score"], fx["a/label"], 0.5, np.zeros(n, dtype=np.int32), np.zeros((1, 1), dtype=np.int32))
    B.assert_matches(single[0], fx["a/single"], n, "a/single")
    # the fixture holds the cases the kernel can get wrong
    assert (fx["mult/ref"][:, 0, 0] > 65535).any() and np.isnan(fx["frame/ref"][:, 0, 9]).any()
    assert (fx["frame/ref"][:, 0, 1] == 0).any() and (fx["frame/ref"][:, 0, 2] == 0).any()


def test_percentile_ci_is_numpy_percentile_over_finite_replicates():
    from ssl4polyp_amd.metrics import percentile_ci
    rng = np.random.default_rng(3)
    a, b = rng.random((200, 8)), rng.random((200, 8))
    a[5, 2] = np.nan
    lo, hi = percentile_ci(a, 0.95)
    keep = np.isfinite(a[:, 2])
    p_lo, p_hi = (1.0 - 0.95) / 2.0 * 100.0, (1.0 + 0.95) / 2.0 * 100.0   # the percents as the reports compute them
    assert lo[2] == np.percentile(a[keep, 2], p_lo) and hi[2] == np.percentile(a[keep, 2], p_hi)
    assert lo[0] == np.percentile(a[:, 0], p_lo) and (lo <= hi).all()
    assert percentile_ci(a[:, 0]) == (np.percentile(a[:, 0], p_lo), np.percentile(a[:, 0], p_hi))
    dlo, dhi = percentile_ci(a, 0.95, baseline=b)   # paired delta of two runs over the same draws
    assert dlo[1] == np.percentile(a[:, 1] - b[:, 1], p_lo) and dhi[2] == np.percentile((a - b)[keep, 2], p_hi)
    assert all(np.isnan(v) for v in percentile_ci(np.full(4, np.nan)))


def test_symbols_load_and_the_workspace_query_answers_without_a_gpu():
    import __graft_entry__ as g
    from ssl4polyp_amd import _lib, metrics
    assert "pm_metrics.hip" in g.SOURCES
    lib = _lib.load()
    assert {"pm_boot_metrics", "pm_boot_metrics_workspace"} <= set(_lib.SIGNATURES)
    assert lib.pm_boot_metrics.restype is ctypes.c_int and len(lib.pm_boot_metrics.argtypes) == 16
    need = ctypes.c_size_t(0)
    N, M, R, K, C = 15840, 2, 512, 600, 600
    assert lib.pm_boot_metrics_workspace(N, M, R, K, C, ctypes.byref(need)) == 0
    assert need.value >= M * N * 20 + R * C * 4 and need.value % 16 == 0   # sorted score + loss (f64), cluster | label, the counters
    big = ctypes.c_size_t(0)
    assert lib.pm_boot_metrics_workspace(N, M, 2 * R, K, C, ctypes.byref(big)) == 0 and big.value - need.value == R * C * 4
    assert lib.pm_boot_metrics_workspace(1, 1, 1, 1, 1, ctypes.byref(need)) == 0 and need.value > 0
    assert metrics.MAX_REPLICATES_PER_CALL == 4096 and metrics.SCAN_TILE == 1024
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), ((1 << 20) + 1, 1, 1, 1, 1),
                (10, 257, 1, 1, 1), (10, 1, 4097, 1, 1), (10, 1, 1, (1 << 20) + 1, 1), (10, 1, 1, 1, (1 << 20) + 1),
                (1 << 16, 1, 1, 1 << 15, 1)):   # the last: N * K = 2^31, a replicate's weight would not fit 31 bits
        assert lib.pm_boot_metrics_workspace(*bad, ctypes.byref(need)) == _lib.PM_ESHAPE, bad
    assert lib.pm_boot_metrics_workspace((1 << 16) - 1, 1, 1, 1 << 15, 1, ctypes.byref(need)) == 0
    assert lib.pm_boot_metrics_workspace(10, 1, 1, 1, 1, None) == _lib.PM_EINVAL
    # the launch entry refuses the same shapes (and missing buffers) before it touches a device
    assert lib.pm_boot_metrics(None, None, None, None, None, None, None, 10, 1, 4097, 1, 1, 0, None, 0, None) == _lib.PM_ESHAPE
    assert lib.pm_boot_metrics(None, None, None, None, None, None, None, 10, 1, 1, 1, 1, 0, None, 0, None) == _lib.PM_EINVAL


def test_main_finetune_flags_are_off_by_default():
    from ssl4polyp_amd import main_finetune as M
    p = M.get_args_parser()
    a = p.parse_args(["--test_csv", "t.csv"])
    assert a.metrics is False and a.bootstrap == 0 and isinstance(a.bootstrap_seed, int)
    b = p.parse_args(["--test_csv", "t.csv", "--metrics", "--bootstrap", "2000", "--bootstrap_seed", "7"])
    assert b.metrics is True and b.bootstrap == 2000 and b.bootstrap_seed == 7
    with pytest.raises(SystemExit, match="num_classes 2"):   # before anything touches a device
        M.run(p.parse_args(["--test_csv", "t.csv", "--metrics", "--num_classes", "3"]))


def test_records_stay_strict_json_when_a_metric_is_undefined():
    import json
    from ssl4polyp_amd import main_finetune as M
    assert M.strict([0.25, float("nan"), float("inf"), 1.0]) == [0.25, None, None, 1.0]
    json.loads(json.dumps(M.strict([float("nan")])), parse_constant=lambda c: pytest.fail(f"bare {c} in a record"))
