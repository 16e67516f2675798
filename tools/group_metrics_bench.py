"""Timing of the per-group bootstrap metrics: one metrics.bootstrap_group_metrics call against the loop of one
metrics.bootstrap_binary_metrics call per group on its gathered subset -- the only way to a group's interval without pm_group_metrics
(needs the GPU; no test gates on these numbers).  Generated scores, R = 2000 replicates, M = 2 runs, two shapes of the reference's
packs: sun_test_perturbations (15 840 frames = 16 tags x 990, 30 cases, G = 17 with ALL-perturbed, E = 30 690 entries, 60 clusters)
and sun_morphology (990 frames = 495 negatives + 330 polypoid + 165 flat, 3 strata).  Both sides take tensors that already lie on
the device (the loop's subsets are gathered before the clock starts, which favours the loop) and include their sorts, chunks and
workspace.  Device events around --calls calls after warm-up, the window repeated --repeats times, the median reported; the two
sides alternate inside a repeat.  The tool also checks that both give the same bits.  Writes profiles/group_metrics.json and prints it.

    python tools/group_metrics_bench.py [--replicates 2000] [--calls 10] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def perturbation_pack(rng):
    """Rows of 990 source frames (30 cases of 33) under 16 tags: clean + 15 perturbations."""
    tags = [{"variant": "clean"}] + [{"blur_sigma": str(s), "variant": "blur"} for s in (1, 2, 3, 4, 5)] + \
           [{"jpeg_q": str(q), "variant": "jpeg"} for q in (10, 20, 40, 60, 80)] + \
           [{"brightness": str(b), "contrast": str(c), "variant": "bc"} for b, c in ((0.7, 0.7), (0.7, 1.3), (1.3, 0.7), (1.3, 1.3))] + \
           [{"bbox_area_frac": "0.2", "variant": "occ"}]
    source_label = rng.random(990) < 0.4
    source_label[::33], source_label[1::33] = True, False      # every case holds both classes: 60 clusters
    rows, labels = [], []
    for tag in tags:
        for i in range(990):
            rows.append({"case_id": f"case{i // 33:02d}", **tag})
            labels.append(int(source_label[i]))
    return rows, np.array(labels, dtype=np.uint8)


def morphology_pack(rng):
    labels = np.array([0] * 495 + [1] * 495, dtype=np.uint8)
    morph = [""] * 495 + ["polypoid"] * 330 + ["flat"] * 165
    rows = [{"case_id": f"case{int(c)}", "morphology": m} for c, m in zip(rng.integers(0, 80, 990), morph)]
    return rows, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "group_metrics.json"))
    args = ap.parse_args()
    import torch
    from ssl4polyp_amd import metrics as MX
    dev = torch.device("cuda", 0)
    R = args.replicates
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "replicates": R, "runs": 2,
              "calls": args.calls, "chunk": MX.CHUNK,
              "note": "grouped = one bootstrap_group_metrics call; loop = one bootstrap_binary_metrics call per group on a subset gathered "
                      "on the device beforehand; ms per evaluation of all groups, median of the windows", "shapes": []}
    for name, pack, build in (("sun_test_perturbations", perturbation_pack, MX.perturbation_groups),
                              ("sun_morphology", morphology_pack, lambda rows, labels: MX.morphology_groups(rows, labels))):
        rng = np.random.default_rng(len(name))
        rows, labels = pack(rng)
        n = len(rows)
        groups = build(rows) if build is MX.perturbation_groups else build(rows, labels)
        score = np.clip(0.35 * labels[None, :] + rng.uniform(0.02, 0.63, (2, n)), 0.0, 1.0).astype(np.float32).astype(np.float64)
        cs = MX.build_cluster_set(rows, labels.tolist())
        draws = MX.draw_cluster_samples(cs, np.random.default_rng(1), R)
        d = {k: torch.as_tensor(v).to(dev) for k, v in (("score", score), ("label", labels), ("cluster", cs.cluster), ("draws", draws))}
        subsets = []
        for g in range(len(groups)):
            f = torch.from_numpy(groups.frames(g).astype(np.int64)).to(dev)
            subsets.append((d["score"][:, f].contiguous(), d["label"][f].contiguous(), d["cluster"][f].contiguous()))

        def grouped():
            return MX.bootstrap_group_metrics(d["score"], d["label"], 0.5, groups, d["cluster"], d["draws"], n_clusters=cs.n_clusters)

        def loop():
            return torch.stack([MX.bootstrap_binary_metrics(s, y, 0.5, c, d["draws"], n_clusters=cs.n_clusters) for s, y, c in subsets], dim=2)

        for _ in range(2):
            a, b = grouped(), loop()
        torch.cuda.synchronize()
        same = bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
        windows = {"grouped": [], "loop": []}
        for _ in range(args.repeats):
            for side, fn in (("grouped", grouped), ("loop", loop)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.calls):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                windows[side].append(t0.elapsed_time(t1) / args.calls)
        med = {k: float(np.median(v)) for k, v in windows.items()}
        rec = {"shape": name, "frames": n, "groups": len(groups), "entries": int(groups.seg[-1]), "clusters": cs.n_clusters,
               "same_bits": same, "grouped_ms": round(med["grouped"], 3), "loop_ms": round(med["loop"], 3),
               "grouped_ms_windows": [round(w, 3) for w in windows["grouped"]], "loop_ms_windows": [round(w, 3) for w in windows["loop"]],
               "loop_over_grouped": round(med["loop"] / med["grouped"], 2)}
        result["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
