"""NumPy restatement of the per-group bootstrap metrics (not a test module): what pm_group_metrics computes from the entry list --
`member` [M, E], `seg` [G + 1] -- with boot_metrics_ref.replicate_metrics as the scan of one segment, the kernel's clamping of the
offsets and its weight zero for an entry that names no frame.  The CPU test holds it to the reference's values of
tests/golden/group_metrics.npz; tools/group_metrics_bench.py reads the fixture's shapes through it."""
import json
import os

import numpy as np

import boot_metrics_ref as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_metrics.npz")
KINDS = ("cont", "round", "equal")
PERT_COLUMNS = ("perturbation_id", "blur_sigma", "jpeg_q", "brightness", "contrast", "bbox_area_frac", "variant")
# the order in which the reference's test() reports the tags of the fixture's `pert` set (train_classification.py:5272-5291,
# :5449-5457): clean, then by component name, numeric values before textual ones and by value (3 before 10, 5 before 40), then the union
PERT_ORDER = ("clean", "bbox_area_frac=0.2", "blur_sigma=1.5", "blur_sigma=3", "blur_sigma=10", "blur_sigma=abc",
              "brightness=1.3|contrast=0.7", "custom", "jpeg_q=5", "jpeg_q=40", "odd_variant", "ALL-perturbed")


def load_fixture():
    return dict(np.load(GOLDEN, allow_pickle=False))


def pert_rows(fx):
    rows = [dict(zip(PERT_COLUMNS, values)) for values in zip(*(fx[f"pert/col/{c}"].tolist() for c in PERT_COLUMNS))]
    for row, case in zip(rows, fx["pert/case_id"].tolist()):
        row["case_id"] = case
    return rows


def typed_rows(fx):
    return json.loads(str(fx["tags/typed_rows"])), json.loads(str(fx["tags/typed_expected"]))


def sizes_members(fx):
    """The frames of the eight groups of the `sizes` set: the seven dealt ones (sizes 0, 1, 2, T - 1, T, T + 1, 3 T + 5), then all."""
    of = fx["sizes/group_of_frame"]
    return [np.flatnonzero(of == g) for g in range(len(fx["sizes/group_sizes"]))] + [np.arange(len(of))]


def layout(members):
    """(entry_frame int32 [E], seg int32 [G + 1]) of index lists: group after group, frames ascending."""
    members = [np.sort(np.asarray(m, dtype=np.int64)) for m in members]
    seg = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    return (np.concatenate(members) if members else np.zeros(0)).astype(np.int32), seg


def member_order_numpy(score, entry_frame, seg):
    """int32 [M, E]: per run and segment the group's frames by descending score, equal scores in ascending frame order."""
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    out = np.empty((score.shape[0], len(entry_frame)), dtype=np.int32)
    for m in range(score.shape[0]):
        for a, b in zip(seg[:-1], seg[1:]):
            frames = np.asarray(entry_frame[a:b], dtype=np.int64)
            out[m, a:b] = frames[np.argsort(-score[m][frames], kind="stable")]
    return out


def group_metrics_numpy(score, label, tau, cluster, draws, member, seg, n_clusters=None):
    """f64 [R, M, G, 16] as pm_group_metrics writes it."""
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    label = np.asarray(label).astype(np.int64)
    cluster, draws, member = np.asarray(cluster), np.asarray(draws), np.atleast_2d(np.asarray(member))
    M, N = score.shape
    E, G = member.shape[1], len(seg) - 1
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (M,))
    C = int(n_clusters) if n_clusters is not None else int(cluster.max()) + 1
    W = B.frame_weights(cluster, draws, C)
    bounds = np.clip(np.asarray(seg, dtype=np.int64), 0, E)            # the kernel's clamp
    out = np.empty((draws.shape[0], M, G, 16))
    for m in range(M):
        valid = (member[m] >= 0) & (member[m] < N)                       # an entry that names no frame: weight zero
        frame = np.where(valid, member[m], 0).astype(np.int64)
        s_all, y_all = np.where(valid, score[m][frame], 0.0), label[frame]
        p = np.clip(s_all, 1e-12, 1.0 - 1e-12)
        loss_all = np.where(valid, -(y_all * np.log(p) + (1 - y_all) * np.log(1 - p)), 0.0)
        for g in range(G):
            a, b = int(bounds[g]), int(bounds[g + 1])
            b = max(a, b)                                                # start >= end: empty
            for r in range(draws.shape[0]):
                if a == b:
                    out[r, m, g] = [0.0, 0.0, 0.0, np.nan, 0.0, 0.0, 0.0, 0.0] + [np.nan] * 8
                    continue
                w = np.where(valid[a:b], W[r][frame[a:b]], 0)
                out[r, m, g] = B.replicate_metrics(s_all[a:b], y_all[a:b], loss_all[a:b], w, tau[m])
    return out


def assert_groups_match(got, ref, sizes, what=""):
    """got / ref [..., G, 16]: every group under boot_metrics_ref.assert_matches with n = that group's number of frames."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.shape[-2] == len(sizes), (what, got.shape, ref.shape, len(sizes))
    for g, n in enumerate(sizes):
        B.assert_matches(got[..., g, :], ref[..., g, :], max(int(n), 1), f"{what} group {g}")
