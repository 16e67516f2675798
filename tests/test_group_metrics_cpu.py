"""Host side of the per-group metrics (ssl4polyp_amd/metrics.py: GroupSet and its builders, the entry order, the threshold grid,
f1-morph, the curve files; pm_group_metrics' admission rules; main_finetune's flags) against tests/golden/group_metrics.npz, which
holds what the reference's functions returned (tests/golden/make_group_metrics_fixture.py).  The torch plumbing runs on CPU tensors
here (device="cpu"); the kernel itself is restated in NumPy (group_metrics_ref) and held to the same values.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import boot_metrics_ref as B
import group_metrics_ref as G

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fx():
    return G.load_fixture()


def _s64(a):
    return np.asarray(a).astype(np.float64)


def test_numpy_restatement_meets_the_reference(fx):
    members = G.sizes_members(fx)
    ef, seg = G.layout(members)
    assert [len(m) for m in members[:-1]] == fx["sizes/group_sizes"].tolist() and int(fx["tile"]) == 1024
    for kind in G.KINDS:
        score = _s64(fx[f"sizes/{kind}/score"])
        member = G.member_order_numpy(score, ef, seg)
        got = G.group_metrics_numpy(score, fx["sizes/label"], fx[f"sizes/{kind}/tau"], fx["sizes/cluster"], fx["sizes/draws"], member, seg)
        G.assert_groups_match(got, fx[f"sizes/{kind}/ref"], [len(m) for m in members], f"sizes/{kind}")
    ref = fx["sizes/cont/ref"]
    assert (ref[:, :, 0, 0] == 0).all() and np.isnan(ref[:, :, 0, 8:]).all()      # the empty group: the n == 0 row
    assert (ref[:, :, 1, 0] == 0).any() and (ref[:, :, 1, 0] > 0).any()           # one frame: drawn in some replicates only
    for name in ("morph", "noflat"):
        from ssl4polyp_amd.metrics import morphology_groups
        groups = morphology_groups(fx["morph/morphology"].tolist(), fx[f"{name}/label"], omit_empty=False)
        score = _s64(fx["morph/score"])
        member = G.member_order_numpy(score, groups.entry_frame, groups.seg)
        got = G.group_metrics_numpy(score, fx[f"{name}/label"], fx["morph/tau"], fx[f"{name}/cluster"], fx[f"{name}/draws"], member, groups.seg)
        G.assert_groups_match(got, fx[f"{name}/boot_ref"], groups.sizes, name)


def test_restated_kernel_clamps_offsets_and_ignores_entries_that_name_no_frame(fx):
    """pm_group_metrics' answer to wrong tables (no test sends them to a device): offsets are clamped to [0, E], start >= end is an
    empty group, an entry outside [0, N) weighs nothing -- here on the restatement, which states the same rules."""
    members = G.sizes_members(fx)[1:4]
    ef, seg = G.layout(members)
    score = _s64(fx["sizes/cont/score"])[:1]
    args = (score, fx["sizes/label"], fx["sizes/cont/tau"][:1], fx["sizes/cluster"], fx["sizes/draws"][:4])
    member = G.member_order_numpy(score, ef, seg)
    good = G.group_metrics_numpy(*args, member, seg)
    E = len(ef)
    wide = G.group_metrics_numpy(*args, member, np.array([-5, seg[1], seg[2], E + 100]))
    assert np.array_equal(wide, good, equal_nan=True)
    back = G.group_metrics_numpy(*args, member, np.array([0, seg[2], seg[1], E]))        # group 1 runs backwards: empty
    assert (back[:, :, 1, 0] == 0).all() and np.isnan(back[:, :, 1, 8:]).all() and np.array_equal(back[:, :, 0], G.group_metrics_numpy(
        *args, member, np.array([0, seg[2], seg[2], E]))[:, :, 0], equal_nan=True)
    holes = member.copy()
    holes[0, seg[3] - 7:seg[3]] = (-1, -2, 1 << 30, len(fx["sizes/label"]), -1, -1, -1)
    kept = np.setdiff1d(members[2], member[0, seg[3] - 7:seg[3]])
    ef2, seg2 = G.layout([kept])
    alone = G.group_metrics_numpy(*args, G.member_order_numpy(score, ef2, seg2), seg2)
    got = G.group_metrics_numpy(*args, holes, seg)
    for k in B.INTEGER_COLUMNS:
        assert np.array_equal(got[:, :, 2, k], alone[:, :, 0, k])
    assert np.array_equal(got[:, :, :2], good[:, :, :2], equal_nan=True)


def test_morphology_groups_are_the_reference_strata(fx):
    from ssl4polyp_amd.metrics import STRATA, GroupSet, morphology_groups
    morph, y = fx["morph/morphology"].tolist(), fx["morph/label"]
    assert {" Flat", "FLAT  ", "Polypoid ", "  POLYPOID", "sessile", "", "  "} <= set(morph)     # spellings, a third morphology, none
    groups = morphology_groups(morph, y)
    assert groups.names == STRATA == ("overall", "flat_plus_negs", "polypoid_plus_negs")
    assert isinstance(groups, GroupSet) and groups.entry_frame.dtype == np.int32 and groups.seg.dtype == np.int32
    norm = np.array([m.strip().lower() for m in morph])
    want = [np.arange(len(y)), np.flatnonzero((y == 0) | ((y == 1) & (norm == "flat"))), np.flatnonzero((y == 0) | ((y == 1) & (norm == "polypoid")))]
    for g, frames in enumerate(want):
        np.testing.assert_array_equal(groups.frames(g), frames)
    np.testing.assert_array_equal(groups.seg, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert len(np.intersect1d(groups.frames(1), groups.frames(2))) == int((y == 0).sum())          # the strata share every negative
    assert (norm[(y == 0)] == "flat").any()                                                        # a negative's value does not matter
    # rows (dicts) and None values are taken alike
    rows = [{"morphology": (m if m != "" else None)} for m in morph]
    again = morphology_groups(rows, y.tolist())
    np.testing.assert_array_equal(again.entry_frame, groups.entry_frame)
    # single evaluation per stratum: the reference's _build_morphology_strata_metrics
    for m in range(3):
        score = _s64(fx["morph/score"][m])
        member = G.member_order_numpy(score, groups.entry_frame, groups.seg)
        got = G.group_metrics_numpy(score, y, fx["morph/tau"][m], np.zeros(len(y), dtype=np.int32), np.zeros((1, 1), dtype=np.int32), member, groups.seg)
        G.assert_groups_match(got[0, 0], fx[f"morph/strata{m}"], groups.sizes, f"strata run {m}")
    # a split without flat positives: omitted as test() omits it, kept (without positives) in the always-three form
    y2 = fx["noflat/label"]
    assert morphology_groups(morph, y2).names == tuple(fx["noflat/strata_names"].tolist()) == ("overall", "polypoid_plus_negs")
    three = morphology_groups(morph, y2, omit_empty=False)
    assert three.names == STRATA and (y2[three.frames(1)] == 0).all() and len(three.frames(1)) == int((y2 == 0).sum())
    assert morphology_groups([], []).names == () and len(morphology_groups([], [])) == 0
    with pytest.raises(ValueError, match="one morphology value per frame"):
        morphology_groups(morph[:-1], y)


def test_perturbation_tags_and_their_order_of_report(fx):
    from ssl4polyp_amd.metrics import ALL_PERTURBED, perturbation_groups, perturbation_tag
    rows, expected = G.typed_rows(fx)
    assert len(rows) == len(expected) >= 15 and None in expected
    for row, want in zip(rows, expected):
        assert perturbation_tag(row) == want, (row, want)
    assert perturbation_tag("not a row") is None
    rows = G.pert_rows(fx)
    tags = [perturbation_tag(r) or "clean" for r in rows]
    assert tags == fx["pert/tag"].tolist() and perturbation_tag(rows[0]) is None      # a row without any tag is clean
    groups = perturbation_groups(rows)
    assert groups.names == G.PERT_ORDER and groups.names[0] == "clean" and groups.names[-1] == ALL_PERTURBED
    assert sorted(groups.names[:-1]) == fx["pert/ref_names"].tolist()[:-1] != list(groups.names[:-1])   # not the alphabetical order
    tags = np.array(tags)
    for name in groups.names[:-1]:
        np.testing.assert_array_equal(groups.frames(name), np.flatnonzero(tags == name))
    np.testing.assert_array_equal(groups.frames(ALL_PERTURBED), np.flatnonzero(tags != "clean"))
    assert int(groups.seg[-1]) == len(rows) + int((tags != "clean").sum())              # E: every frame once, the perturbed twice
    clean_only = perturbation_groups([{"variant": "clean"}, {}, {"jpeg_q": "-1"}])
    assert clean_only.names == ("clean",) and clean_only.sizes.tolist() == [3]


def test_group_set_checks_its_layout():
    from ssl4polyp_amd.metrics import GroupSet
    g = GroupSet.from_members(("a", "b", "c"), [[3, 1], [], np.array([True, False, True, True])])
    assert g.entry_frame.tolist() == [1, 3, 0, 2, 3] and g.seg.tolist() == [0, 2, 2, 5] and g.sizes.tolist() == [2, 0, 3]
    assert g.subset(["c", "a"]).names == ("c", "a") and g.subset(["c", "a"]).seg.tolist() == [0, 3, 5]
    for names, ef, seg in ((("a",), [0, 1], [0, 1]), (("a",), [0, 1], [1, 2]), (("a", "b"), [0, 1], [0, 2, 1]), (("a", "a"), [0], [0, 1, 1])):
        with pytest.raises(ValueError):
            GroupSet(names, ef, seg)


def test_member_order_is_group_then_descending_score_then_frame(fx):
    from ssl4polyp_amd.metrics import GroupSet, group_member_order
    members = G.sizes_members(fx)
    groups = GroupSet.from_members([f"g{i}" for i in range(len(members))], members)
    ef, seg = G.layout(members)
    np.testing.assert_array_equal(groups.entry_frame, ef)
    np.testing.assert_array_equal(groups.seg, seg)
    for kind in G.KINDS:
        score = _s64(fx[f"sizes/{kind}/score"])
        got = group_member_order(torch.from_numpy(score), groups).numpy()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, G.member_order_numpy(score, ef, seg))
        for a, b, frames in zip(seg[:-1], seg[1:], members):     # a segment is the stable descending sort of the gathered subset
            sub = np.argsort(-score[1][frames], kind="stable")
            np.testing.assert_array_equal(got[1, a:b], frames[sub])
    with pytest.raises(ValueError, match="frames"):
        group_member_order(torch.zeros(1, 3, dtype=torch.float64), GroupSet(("a",), [0, 3], [0, 2]))


def test_threshold_grid_counts_are_exact(fx):
    from ssl4polyp_amd.metrics import morphology_groups, threshold_grid_counts
    y = fx["morph/label"]
    groups = morphology_groups(fx["morph/morphology"].tolist(), y, omit_empty=False)
    score = _s64(fx["morph/score"])
    taus = np.concatenate([np.linspace(0, 1, 17), score[1][:5], [-1.0, 2.0]])      # grid points, taus AT a score, outside the range
    got = threshold_grid_counts(torch.from_numpy(score), y, taus, groups, device=CPU)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 3, len(taus), 4)
    for m in range(3):
        for g in range(3):
            f = groups.frames(g)
            for k, t in enumerate(taus):
                p = score[m][f] >= t
                want = [int((p & (y[f] == 1)).sum()), int((p & (y[f] == 0)).sum()), int((~p & (y[f] == 0)).sum()), int((~p & (y[f] == 1)).sum())]
                assert got[m, g, k].tolist() == want, (m, g, t)
    whole = threshold_grid_counts(score[0], y, taus, device=CPU)
    assert torch.equal(whole[0, 0], got[0, 0])


def test_f1_morph_threshold_is_the_reference_tau(fx):
    from ssl4polyp_amd.metrics import f1_morph_threshold
    morph, y = fx["morph/morphology"].tolist(), fx["morph/label"]
    for m in range(3):
        assert f1_morph_threshold(_s64(fx["morph/score"][m]), y, morph, device=CPU) == float(fx["morph/f1_morph_tau"][m])
    assert f1_morph_threshold(_s64(fx["morph/score"][0]), y, morph, grid_points=64, device=CPU) == float(fx["morph/f1_morph_tau_64"])
    for m in range(2):
        got = f1_morph_threshold(torch.from_numpy(_s64(fx["grid/score"][m])), fx["grid/label"], fx["grid/morphology"].tolist(), device=CPU)
        assert got == float(fx["grid/f1_morph_tau"][m]) and 0.0 < got < 1.0
    # None where the reference gives none: no flat positive, a length mismatch, no frames
    assert f1_morph_threshold(_s64(fx["morph/score"][0]), fx["noflat/label"], morph, device=CPU) is None
    assert f1_morph_threshold(_s64(fx["morph/score"][0]), y, morph[:-1], device=CPU) is None
    assert f1_morph_threshold(np.zeros(0), np.zeros(0), [], device=CPU) is None


def test_curve_files_are_the_reference_text(fx, tmp_path):
    from ssl4polyp_amd.metrics import curve_rows, export_curves
    for m in range(2):
        got = export_curves(tmp_path / "sub" / f"stem{m}", "test", _s64(fx["grid/score"][m]), fx["grid/label"], int(fx[f"grid/points{m}"]), device=CPU)
        assert got["grid_points"] == int(fx[f"grid/points{m}"]) and got["roc_csv"].endswith(f"stem{m}_test_roc_curve.csv")
        assert got["pr_csv"].endswith(f"stem{m}_test_pr_curve.csv")
        assert open(got["roc_csv"], newline="").read() == str(fx[f"grid/roc_csv{m}"])
        assert open(got["pr_csv"], newline="").read() == str(fx[f"grid/pr_csv{m}"])
    neg = export_curves(tmp_path / "neg", "val", _s64(fx["grid/neg_score"]), np.zeros(2, dtype=np.int64), 3, device=CPU)
    assert open(neg["roc_csv"], newline="").read() == str(fx["grid/neg_roc_csv"]) and ",," in str(fx["grid/neg_pr_csv"])   # empty cells
    assert open(neg["pr_csv"], newline="").read() == str(fx["grid/neg_pr_csv"])
    roc, pr = curve_rows(_s64(fx["grid/neg_score"]), np.zeros(2, dtype=np.int64), 3, device=CPU)
    assert roc[1] == {"threshold": 0.5, "tpr": None, "fpr": 0.5, "tp": 0, "fp": 1, "tn": 1, "fn": 0} and pr[1]["f1"] is None
    for bad in (dict(grid_points=1), dict(grid_points=None)):
        with pytest.raises(ValueError, match="two grid points"):
            curve_rows(np.zeros(2), np.zeros(2), device=CPU, **bad)
    with pytest.raises(ValueError, match="no samples"):
        curve_rows(np.zeros(0), np.zeros(0), device=CPU)


def test_group_case_metrics_are_the_reference_values(fx):
    from ssl4polyp_amd.metrics import group_case_metrics, perturbation_groups
    rows = G.pert_rows(fx)
    groups = perturbation_groups(rows)
    cases = fx["pert/case_names"].tolist()
    index = [cases.index(r["case_id"]) for r in rows]
    at = [fx["pert/ref_names"].tolist().index(n) for n in groups.names]
    for m in range(3):
        got = group_case_metrics(_s64(fx["pert/score"][m]), fx["pert/label"], float(fx["pert/tau"][m]), groups, index, len(cases), device=CPU)
        want = fx["pert/per_case"][m][at]
        assert got["count"].dtype == torch.int64 and tuple(got["recall"].shape) == (len(groups), len(cases))
        np.testing.assert_array_equal(got["count"].numpy(), want[..., 2])
        np.testing.assert_array_equal(got["recall"].numpy(), want[..., 0])     # one division of two integers: the same bits
        np.testing.assert_array_equal(got["f1"].numpy(), want[..., 1])
    assert (want[..., 0] == 0).any() and (want[..., 0] == 1).any() and ((want[..., 1] > 0) & (want[..., 1] < 1)).any()
    extra = group_case_metrics(_s64(fx["pert/score"][0]), fx["pert/label"], 0.5, groups, index, len(cases) + 1, device=CPU)
    assert (extra["count"][:, -1] == 0).all() and (extra["recall"][:, -1] == 0).all()


def test_names_symbols_and_admission_without_a_gpu():
    import __graft_entry__ as g
    from ssl4polyp_amd import _lib, metrics
    assert "pm_metrics.hip" in g.SOURCES and _lib.ABI_VERSION == 16
    lib = _lib.load()
    assert {"pm_group_metrics", "pm_group_metrics_workspace"} <= set(_lib.SIGNATURES)
    assert lib.pm_group_metrics.restype is ctypes.c_int and len(lib.pm_group_metrics.argtypes) == 19
    need, boot = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N, M, E, Gn, R, K, C = 15840, 2, 30690, 17, 512, 60, 60
    assert lib.pm_group_metrics_workspace(N, M, E, Gn, R, K, C, ctypes.byref(need)) == 0
    assert need.value >= M * E * 20 + R * C * 4 and need.value % 16 == 0       # the view is per entry: score + loss (f64), cluster | label
    assert lib.pm_boot_metrics_workspace(E, M, R, K, C, ctypes.byref(boot)) == 0 and boot.value == need.value
    big = ctypes.c_size_t(0)
    assert lib.pm_group_metrics_workspace(N, M, E, Gn, 2 * R, K, C, ctypes.byref(big)) == 0 and big.value - need.value == R * C * 4
    assert lib.pm_group_metrics_workspace(1, 1, 1, 1, 1, 1, 1, ctypes.byref(need)) == 0 and need.value > 0
    assert metrics.MAX_GROUP_ENTRIES == 1 << 22 and metrics.MAX_GROUPS == 1 << 16
    for bad in ((0, 1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1, 1), (1, 1, 1, 0, 1, 1, 1), (1, 1, 1, 1, 0, 1, 1),
                (1, 1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 1, 1, 0), (1, 1, -3, 1, 1, 1, 1),
                ((1 << 20) + 1, 1, 1, 1, 1, 1, 1), (10, 257, 1, 1, 1, 1, 1), (10, 1, (1 << 22) + 1, 1, 1, 1, 1), (10, 1, 1, (1 << 16) + 1, 1, 1, 1),
                (10, 1, 1, 1, 4097, 1, 1), (10, 1, 1, 1, 1, (1 << 20) + 1, 1), (10, 1, 1, 1, 1, 1, (1 << 20) + 1),
                (10, 1, 1 << 16, 1, 1, 1 << 15, 1),              # E * K = 2^31: a segment's weight would not fit 31 bits
                (10, 256, 10, 1 << 16, 4096, 1, 1)):             # R * M * G = 2^36: more workgroups than one launch holds
        assert lib.pm_group_metrics_workspace(*bad, ctypes.byref(need)) == _lib.PM_ESHAPE, bad
    assert lib.pm_group_metrics_workspace(10, 1, (1 << 16) - 1, 1, 1, 1 << 15, 1, ctypes.byref(need)) == 0
    assert lib.pm_group_metrics_workspace(10, 128, 10, 1 << 12, 4095, 1, 1, ctypes.byref(need)) == 0       # R * M * G just below 2^31
    assert lib.pm_group_metrics_workspace(10, 1, 1, 1, 1, 1, 1, None) == _lib.PM_EINVAL
    # the launch entry refuses the same shapes, missing buffers, a short workspace and bad alignment before it touches a device
    none = (None,) * 8
    assert lib.pm_group_metrics(*none, 10, 1, 10, (1 << 16) + 1, 1, 1, 1, 0, None, 0, None) == _lib.PM_ESHAPE
    assert lib.pm_group_metrics(*none, 10, 1, 10, 1, 1, 1, 1, 0, None, 0, None) == _lib.PM_EINVAL
    buf = (ctypes.c_double * 64)()
    at = ctypes.addressof(buf)
    at += (-at) % 16
    ptrs = (at,) * 8
    assert lib.pm_group_metrics_workspace(4, 1, 4, 1, 1, 1, 1, ctypes.byref(need)) == 0 and need.value <= 256
    assert lib.pm_group_metrics(*ptrs, 4, 1, 4, 1, 1, 1, 1, 0, at, need.value - 1, None) == _lib.PM_EINVAL
    assert lib.pm_group_metrics(*ptrs, 4, 1, 4, 1, 1, 1, 1, 0, at + 8, need.value, None) == _lib.PM_EALIGN
    assert lib.pm_group_metrics(at + 4, *ptrs[1:], 4, 1, 4, 1, 1, 1, 1, 0, at, need.value, None) == _lib.PM_EALIGN
    assert lib.pm_group_metrics(at, at + 2, *ptrs[2:], 4, 1, 4, 1, 1, 1, 1, 0, at, need.value, None) == _lib.PM_EALIGN


def test_main_finetune_group_flags():
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import metrics as MX
    p = M.get_args_parser()
    a = p.parse_args(["--test_csv", "t.csv"])
    assert a.group_metrics == [] and a.curve_export == 0 and a.threshold_policy == "none"
    b = p.parse_args(["--test_csv", "t.csv", "--group_metrics", "morphology", "--group_metrics", "perturbation", "--curve_export", "200",
                      "--threshold_policy", "f1-morph"])
    assert b.group_metrics == ["morphology", "perturbation"] and b.curve_export == 200 and b.threshold_policy == "f1-morph"
    assert M.MORPH_POLICY == MX.F1_MORPH_POLICY == "f1-morph" and M.MORPH_POLICY not in M.SELECTING_POLICIES and M.MORPH_POLICY not in MX.POLICIES
    assert M.SELECTING_POLICIES == tuple(MX.POLICIES) and M.GROUP_KINDS == ("morphology", "perturbation")
    assert MX.format_threshold_key("SUN", "val", M.MORPH_POLICY) == "sun_val_f1-morph"
    with pytest.raises(SystemExit):
        p.parse_args(["--test_csv", "t.csv", "--group_metrics", "colour"])
    # refusals before anything touches a device
    with pytest.raises(SystemExit, match="num_classes 2"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--group_metrics", "morphology", "--num_classes", "3"]))
    with pytest.raises(SystemExit, match="two grid points"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--curve_export", "1"]))
    with pytest.raises(SystemExit, match="num_classes 2"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--curve_export", "10", "--num_classes", "3"]))
    with pytest.raises(SystemExit, match="num_classes 2"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "f1-morph", "--num_classes", "3"]))
    with pytest.raises(SystemExit, match="needs --val_csv"):
        M.run(p.parse_args(["--test_csv", "t.csv", "--threshold_policy", "f1-morph"]))
