"""pm_group_metrics on the device (ssl4polyp_amd/metrics.py: bootstrap_group_metrics and what is built on it) against
tests/golden/group_metrics.npz: every expected value is what the reference returned on the gathered sample of that (replicate, run,
group).  Bound per group: boot_metrics_ref.assert_matches with n = the group's number of frames (64 n 2^-53 max(1, |ref|); integer
columns equal, non-finite values non-finite alike).  Beyond the values, the equalities the design rests on are held bit for bit: a
group is the gathered-subset call, the group of every frame is the ungrouped call, neighbours and chunking change nothing."""
import csv
import json

import numpy as np
import pytest
import torch

import boot_metrics_ref as B
import group_metrics_ref as G
from pack_files import encode, frame, write_pack

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx():
    return G.load_fixture()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _sizes_groups(fx):
    from ssl4polyp_amd.metrics import GroupSet
    members = G.sizes_members(fx)
    return GroupSet.from_members([f"n{len(m)}" for m in members[:-1]] + ["all"], members), members


def _gathered(score, label, tau, cluster, draws, frames, C, **kw):
    """bootstrap_binary_metrics on the frames of one group alone, with the set's clusters and draws."""
    from ssl4polyp_amd.metrics import bootstrap_binary_metrics
    f = torch.as_tensor(np.asarray(frames, dtype=np.int64))
    return bootstrap_binary_metrics(score[:, f.to(score.device)], np.asarray(label)[frames], tau, np.asarray(cluster)[frames], draws, n_clusters=C, **kw)


@pytest.mark.parametrize("kind", G.KINDS)
def test_group_sizes_around_the_tile(fx, kind):
    """Groups of 0, 1, 2, T - 1, T, T + 1 and 3 T + 5 frames dealt at random from one set, plus the group of every frame; R = 16,
    three runs with tau below / inside / above the score range."""
    from ssl4polyp_amd.metrics import SCAN_TILE as T
    from ssl4polyp_amd.metrics import bootstrap_binary_metrics, bootstrap_group_metrics, group_member_order
    groups, members = _sizes_groups(fx)
    assert groups.sizes.tolist() == [0, 1, 2, T - 1, T, T + 1, 3 * T + 5, 6 * T + 8] and T == int(fx["tile"])
    score64, tau, ref = fx[f"sizes/{kind}/score"].astype(np.float64), fx[f"sizes/{kind}/tau"], fx[f"sizes/{kind}/ref"]
    label, cluster, draws = fx["sizes/label"], fx["sizes/cluster"], fx["sizes/draws"]
    assert ref.shape == (16, 3, 8, 16) and tau[0] < score64[0].min() and score64[1].min() <= tau[1] <= score64[1].max() and tau[2] > score64[2].max()
    score = torch.from_numpy(score64).to(DEV)
    C = int(cluster.max()) + 1
    member = group_member_order(score, groups).cpu().numpy()
    np.testing.assert_array_equal(member, G.member_order_numpy(score64, groups.entry_frame, groups.seg))
    if kind == "equal":   # a tie lies across every boundary between two non-empty segments: the last score of g = the first of g + 1
        inner = [int(s) for s in groups.seg[1:-1] if 0 < s]
        assert len(inner) == 6 and all(score64[m][member[m, s - 1]] == score64[m][member[m, s]] for m in range(3) for s in inner)
    got = bootstrap_group_metrics(score, label, tau, groups, cluster, draws)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (16, 3, 8, 16)
    G.assert_groups_match(got.cpu().numpy(), ref, groups.sizes, f"sizes/{kind}")
    assert (got[:, :, 0, :3] == 0).all() and torch.isnan(got[:, :, 0, 8:]).all() and torch.isnan(got[:, :, 0, 3]).all()   # the empty group
    # the group of every frame is the ungrouped call, bit for bit
    whole = bootstrap_binary_metrics(score, label, tau, cluster, draws, n_clusters=C)
    assert torch.equal(_bits(got[:, :, 7]), _bits(whole))
    # every group is the call on its gathered subset
    for g in range(1, 8):
        alone = _gathered(score, label, tau, cluster, draws, members[g], C)
        assert torch.equal(_bits(got[:, :, g]), _bits(alone)), (kind, g)
    # a group's values do not depend on its neighbours, nor on the other runs
    for g in (2, 5):
        solo = bootstrap_group_metrics(score, label, tau, groups.subset([g]), cluster, draws)
        assert torch.equal(_bits(solo[:, :, 0]), _bits(got[:, :, g]))
    one_run = bootstrap_group_metrics(score[1], label, tau[1], groups, cluster, draws)
    assert torch.equal(_bits(one_run[:, 0]), _bits(got[:, 1]))


def test_chunks_and_repeated_calls_give_the_same_bits(fx):
    from ssl4polyp_amd.metrics import bootstrap_group_metrics
    groups, _ = _sizes_groups(fx)
    cluster = fx["sizes/cluster"]
    C = int(cluster.max()) + 1
    draws = np.random.default_rng(5).integers(0, C, (37, C)).astype(np.int32)     # any list of clusters is a replicate
    draws[3, 10:] = -1
    score = torch.from_numpy(fx["sizes/round/score"].astype(np.float64)).to(DEV)
    args = (score, fx["sizes/label"], fx["sizes/round/tau"], groups, cluster, draws)
    one = bootstrap_group_metrics(*args, n_clusters=C, chunk=64)
    again = bootstrap_group_metrics(*args, n_clusters=C, chunk=64)
    parts = bootstrap_group_metrics(*args, n_clusters=C, chunk=16)               # 16, 16 and 5
    assert tuple(one.shape) == (37, 3, 8, 16) and torch.equal(_bits(one), _bits(again)) and torch.equal(_bits(one), _bits(parts))
    ref = G.group_metrics_numpy(score.cpu().numpy(), fx["sizes/label"], fx["sizes/round/tau"], cluster, draws[:4],
                                G.member_order_numpy(score.cpu().numpy(), groups.entry_frame, groups.seg), groups.seg, C)
    G.assert_groups_match(one[:4].cpu().numpy(), ref, groups.sizes, "37 draws")   # the restatement, held to the reference by the CPU test


def test_morphology_strata(fx):
    from ssl4polyp_amd.metrics import METRIC_KEYS, STRATA, bootstrap_group_metrics, group_metrics, morphology_groups
    morph = fx["morph/morphology"].tolist()
    score = torch.from_numpy(fx["morph/score"].astype(np.float64)).to(DEV)
    tau = fx["morph/tau"]
    assert {" Flat", "FLAT  ", "Polypoid ", "  POLYPOID", "sessile", ""} <= set(morph)
    groups = morphology_groups(morph, fx["morph/label"])
    assert groups.names == STRATA
    got = bootstrap_group_metrics(score, fx["morph/label"], tau, groups, fx["morph/cluster"], fx["morph/draws"]).cpu().numpy()
    G.assert_groups_match(got, fx["morph/boot_ref"], groups.sizes, "morph")
    # replicates 14 / 15 draw no negative and no flat / no polypoid positive: that stratum has weight zero, the others do not
    assert (got[14, :, 1, 0] == 0).all() and np.isnan(got[14, :, 1, 8:]).all() and (got[14, :, 2, 0] > 0).all()
    assert (got[15, :, 2, 0] == 0).all() and np.isnan(got[15, :, 2, 8:]).all() and (got[15, :, 1, 0] > 0).all()
    for m in range(3):   # the single evaluation: _build_morphology_strata_metrics
        single = group_metrics(score[m], fx["morph/label"], float(tau[m]), groups)
        assert tuple(single) == STRATA and all(tuple(v) == METRIC_KEYS for v in single.values())
        G.assert_groups_match(np.array([list(v.values()) for v in single.values()]), fx[f"morph/strata{m}"], groups.sizes, f"strata run {m}")
    # a split without flat positives: the stratum is left out, or (always-three form) holds the negatives alone
    label2 = fx["noflat/label"]
    omitted = morphology_groups(morph, label2)
    assert omitted.names == ("overall", "polypoid_plus_negs")
    single = group_metrics(score[0], label2, float(tau[0]), omitted)
    G.assert_groups_match(np.array([list(v.values()) for v in single.values()]), fx["noflat/strata0"], omitted.sizes, "noflat strata")
    three = morphology_groups(morph, label2, omit_empty=False)
    got2 = bootstrap_group_metrics(score, label2, tau, three, fx["noflat/cluster"], fx["noflat/draws"]).cpu().numpy()
    G.assert_groups_match(got2, fx["noflat/boot_ref"], three.sizes, "noflat")
    assert (got2[:, :, 1, 0] > 0).all() and (got2[:, :, 1, 1] == 0).all() and np.isnan(got2[:, :, 1, 9]).all() and (got2[:, :, 1, 8] == 0).all()
    assert group_metrics(score[0, :0], [], 0.5, morphology_groups([], [])) == {}


def test_perturbation_tags_and_cases(fx):
    from ssl4polyp_amd.metrics import ALL_PERTURBED, bootstrap_group_metrics, group_case_metrics, group_metrics, perturbation_groups
    rows = G.pert_rows(fx)
    groups = perturbation_groups(rows)
    assert groups.names == G.PERT_ORDER
    at = [fx["pert/ref_names"].tolist().index(n) for n in groups.names]
    label, cluster, draws, tau = fx["pert/label"], fx["pert/cluster"], fx["pert/draws"], fx["pert/tau"]
    score = torch.from_numpy(fx["pert/score"].astype(np.float64)).to(DEV)
    got = bootstrap_group_metrics(score, label, tau, groups, cluster, draws)
    G.assert_groups_match(got.cpu().numpy(), fx["pert/boot_ref"][:, :, at], groups.sizes, "pert")
    # ALL-perturbed is the union of the tags that are not clean: the call on those frames
    union = np.flatnonzero(fx["pert/tag"] != "clean")
    np.testing.assert_array_equal(groups.frames(ALL_PERTURBED), union)
    assert torch.equal(_bits(got[:, :, -1]), _bits(_gathered(score, label, tau, cluster, draws, union, int(cluster.max()) + 1)))
    assert (got[:, :, -1, 0] == got[:, :, 1:-1, 0].sum(dim=2)).all()
    for m in range(3):
        single = group_metrics(score[m], label, float(tau[m]), groups)
        assert tuple(single) == G.PERT_ORDER
        G.assert_groups_match(np.array([list(v.values()) for v in single.values()]), fx["pert/single_ref"][m][at], groups.sizes, f"per tag, run {m}")
        cases = fx["pert/case_names"].tolist()
        per = group_case_metrics(score[m], label, float(tau[m]), groups, [cases.index(r["case_id"]) for r in rows], len(cases))
        want = fx["pert/per_case"][m][at]
        assert per["count"].is_cuda and per["count"].dtype == torch.int64
        np.testing.assert_array_equal(per["count"].cpu().numpy(), want[..., 2])
        np.testing.assert_array_equal(per["recall"].cpu().numpy(), want[..., 0])
        np.testing.assert_array_equal(per["f1"].cpu().numpy(), want[..., 1])


def test_threshold_grid_f1_morph_and_curves_on_the_device(fx, tmp_path):
    from ssl4polyp_amd.metrics import export_curves, f1_morph_threshold, morphology_groups, threshold_grid_counts
    morph, label = fx["grid/morphology"].tolist(), fx["grid/label"]
    score = torch.from_numpy(fx["grid/score"].astype(np.float64)).to(DEV)
    groups = morphology_groups(morph, label)
    taus = np.linspace(0.0, 1.0, 512)
    counts = threshold_grid_counts(score, label, taus, groups)
    assert counts.is_cuda and tuple(counts.shape) == (2, 3, 512, 4)
    assert torch.equal(counts.cpu(), threshold_grid_counts(score.cpu(), label, taus, groups, device=torch.device("cpu")))
    assert (counts.sum(dim=-1) == torch.as_tensor(groups.sizes, device=DEV)[None, :, None]).all()
    for m in range(2):
        assert f1_morph_threshold(score[m], label, morph) == float(fx["grid/f1_morph_tau"][m])
        got = export_curves(tmp_path / f"stem{m}", "test", score[m], label, int(fx[f"grid/points{m}"]))
        assert open(got["roc_csv"], newline="").read() == str(fx[f"grid/roc_csv{m}"])
        assert open(got["pr_csv"], newline="").read() == str(fx[f"grid/pr_csv{m}"])


def _log(path):
    return [json.loads(ln) for ln in open(path)]


def test_main_finetune_reports_groups_selects_f1_morph_and_writes_curves(tmp_path):
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import metrics as MX
    plain_csv, roots, _, labels = write_pack(str(tmp_path / "pack"))
    (key, root), = roots.items()
    morphology = {1: "flat", 3: " Polypoid", 5: "FLAT ", 7: "polypoid", 9: "sessile"}
    rows = list(csv.DictReader(open(plain_csv, newline="")))
    for i, r in enumerate(rows):
        r["morphology"], r["case_id"] = morphology.get(i, ""), f"c{i // 2}"
    csv_path = str(tmp_path / "pack" / "groups.csv")
    with open(csv_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    data = ["--root", f"{key}={root}", "--batch_size", "8", "--precision", "bf16", "--num_workers", "0", "--no_pin_mem", "--seed", "3"]
    flags = ["--metrics", "--bootstrap", "8", "--group_metrics", "morphology", "--group_metrics", "perturbation", "--threshold_policy", "f1-morph",
             "--curve_export", "21"]
    out = tmp_path / "groups"
    _, val_logits = M.run(M.get_args_parser().parse_args(["--val_csv", csv_path, "--test_csv", csv_path] + data + flags + ["--output_dir", str(out)]))
    val, test = _log(out / "log.txt")
    probs = MX.positive_probs(val_logits.to(DEV))     # val and test are the same ten files: these are the test scores too
    # ---- the f1-morph tau, selected on val and in force on test
    tau = MX.f1_morph_threshold(probs, labels, [r["morphology"] for r in rows])
    assert tau is not None and val["val_threshold"] == {"policy": "f1-morph", "tau": tau, "split": "dataset/val", "epoch": 0, "fallback": None}
    assert val["val_tau"] == test["test_tau"] == tau
    # ---- the strata and the tags at that tau
    strata = MX.morphology_groups(rows, labels)
    assert strata.names == MX.STRATA and strata.sizes.tolist() == [10, 7, 7]
    want = MX.group_metrics(probs, labels, tau, strata)
    assert test["test_strata"] == {g: dict(zip(v, M.strict(v.values()))) for g, v in want.items()}
    assert test["test_strata"]["overall"] == test["test_metrics_at_tau"]
    tags = MX.perturbation_groups(rows)
    assert tags.names == ("clean", "bc_b1p3_c0p7", "blur_1p5", "jpeg_q=40", "occ_a0p2", "ALL-perturbed")
    block = test["test_perturbation_metrics"]
    assert set(block) == {"per_tag", "per_case"} and tuple(block["per_tag"]) == tags.names == tuple(block["per_case"])
    want = MX.group_metrics(probs, labels, tau, tags)
    assert block["per_tag"] == {g: dict(zip(v, M.strict(v.values()))) for g, v in want.items()}
    assert block["per_tag"]["clean"]["count"] == 6 and block["per_tag"]["ALL-perturbed"]["count"] == 4
    one = block["per_tag"]["blur_1p5"]                # one frame: AUROC is undefined and is written as null, not as a bare NaN
    assert one["count"] == 1 and one["auroc"] is None and "NaN" not in open(out / "log.txt").read()
    assert set(block["per_case"]["clean"]) == {"c0", "c2", "c3", "c4"} and block["per_case"]["blur_1p5"] == {"c0": {"recall": 0.0, "f1": 0.0, "count": 1.0}}
    assert all(set(v) == {"recall", "f1", "count"} for per in block["per_case"].values() for v in per.values())
    # ---- the intervals: per group and reported metric, from the draws of the overall interval
    for name, groups in (("test_strata_ci", strata), ("test_perturbation_ci", tags)):
        assert set(test[name]) == {"ci_lower", "ci_upper"}
        for side in ("ci_lower", "ci_upper"):
            assert tuple(test[name][side]) == groups.names and all(tuple(v) == MX.REPORTED_KEYS for v in test[name][side].values())
    assert test["test_strata_ci"]["ci_lower"]["overall"] == test["ci_lower"] and test["test_strata_ci"]["ci_upper"]["overall"] == test["ci_upper"]
    lo, hi = test["test_strata_ci"]["ci_lower"]["flat_plus_negs"]["recall"], test["test_strata_ci"]["ci_upper"]["flat_plus_negs"]["recall"]
    assert lo is None or lo <= hi
    # ---- the curve files
    for rec, split in ((val, "val"), (test, "test")):
        paths = rec[f"{split}_curves"]
        assert paths["grid_points"] == 21 and paths["roc_csv"] == str(out / f"curves_{split}_roc_curve.csv")
        for kind, columns in (("roc_csv", "threshold,tpr,fpr,tp,fp,tn,fn"), ("pr_csv", "threshold,precision,recall,f1,tp,fp,tn,fn")):
            lines = open(paths[kind], newline="").read().split("\r\n")
            assert lines[0] == columns and len(lines) == 23 and lines[-1] == ""
    # ---- no morphology column: f1-morph has no answer and the run falls back to Youden's J
    M.run(M.get_args_parser().parse_args(["--val_csv", plain_csv, "--test_csv", plain_csv] + data + ["--threshold_policy", "f1-morph", "--output_dir",
                                                                                                    str(tmp_path / "fallback")]))
    val1, test1 = _log(tmp_path / "fallback" / "log.txt")
    youden = MX.select_threshold(probs, labels, "youden")[0, 0].item()
    assert val1["val_threshold"] == {"policy": "f1-morph", "tau": youden, "split": "dataset/val", "epoch": 0, "fallback": "youden"}
    assert test1["test_tau"] == youden and "test_strata" not in test1 and "test_curves" not in test1
    # ---- one epoch of training: the checkpoint keeps the tau under the reference's key
    troot = tmp_path / "tdata"
    (troot / "img").mkdir(parents=True)
    with open(tmp_path / "train.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame_path", "label", "store_id", "variant", "morphology"])
        for i in range(16):
            (troot / "img" / f"{i:02d}.jpg").write_bytes(encode(frame(64, 64, 200 + i), subsampling=2, quality=90))
            w.writerow([f"img/{i:02d}.jpg", (i // 2) % 2, "frames", "clean", ("flat", "polypoid")[i % 2] if (i // 2) % 2 else ""])
    tout = tmp_path / "train"
    M.run(M.get_args_parser().parse_args(["--train_csv", str(tmp_path / "train.csv"), "--val_csv", str(tmp_path / "train.csv"), "--root",
                                          f"frames={troot}"] + data[2:] + ["--threshold_policy", "f1-morph", "--output_dir", str(tout),
                                                                            "--epochs", "1", "--finetune_mode", "head+1"]))
    epoch, = _log(tout / "log.txt")
    ckpt = torch.load(str(tout / "ckpts" / "finetune_e1.pth"), map_location="cpu", weights_only=False)
    name = "dataset_val_f1-morph"
    assert set(ckpt["thresholds"]) == set(ckpt["threshold_records"]) == {name}
    assert ckpt["thresholds"][name] == epoch["val_tau"] == epoch["val_threshold"]["tau"] and ckpt["threshold_records"][name] == epoch["val_threshold"]
    assert epoch["val_threshold"]["policy"] == "f1-morph" and epoch["val_threshold"]["epoch"] == 1 and epoch["val_threshold"]["fallback"] is None
    # ---- without the new flags the records are what they were
    M.run(M.get_args_parser().parse_args(["--val_csv", csv_path, "--test_csv", csv_path] + data + ["--output_dir", str(tmp_path / "plain")]))
    val0, test0 = _log(tmp_path / "plain" / "log.txt")
    assert set(val0) == {"val_loss"} and set(test0) == {"test_loss", "test_samples"}
    assert val0["val_loss"] == val["val_loss"] and test0["test_loss"] == test["test_loss"]
