"""Timing of the bootstrap metrics on the device against a NumPy restatement of the same replicates on this host (needs the GPU;
no test gates on these numbers).  Generated scores, R = 2000 replicates, M = 2 runs, N = 6 600 and 15 840 frames in ~12-frame
cases per label: device events around 10 calls of metrics.bootstrap_binary_metrics after warm-up (sort, chunks and workspace
included), the window repeated --repeats times so that the spread is known (the median is reported), and the wall time of
tests/boot_metrics_ref.boot_metrics_numpy on one core over the first --host-replicates replicates only: the host's figures for all R
(host_numpy_s_for_all_replicates, host_over_device) are that time scaled by R / host_replicates, not measured, and the file says so
(host_replicates).  `device` is the name the runtime gives the card, which may be a generic one; `arch` is its ISA (gfx950 on an
MI355X).  Writes profiles/boot_metrics.json and prints it.

    python tools/boot_metrics_bench.py [--replicates 2000] [--calls 10] [--repeats 5] [--host-replicates 100] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def generated(n, seed):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.4).astype(np.uint8)
    rows = [{"case_id": f"case{int(c)}"} for c in rng.integers(0, max(2, n // 12), n)]
    score = np.clip(0.35 * labels[None, :] + rng.uniform(0.02, 0.63, (2, n)), 0.0, 1.0).astype(np.float32).astype(np.float64)
    return rows, labels, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[6600, 15840])
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-replicates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "boot_metrics.json"))
    args = ap.parse_args()
    import torch
    from boot_metrics_ref import assert_matches, boot_metrics_numpy
    from ssl4polyp_amd import metrics as MX
    dev = torch.device("cuda", 0)
    R = args.replicates
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "replicates": R,
              "host_replicates": min(args.host_replicates, R),
              "note": "host_numpy_s_for_all_replicates and host_over_device are scaled from host_replicates timed replicates",
              "runs": 2, "calls": args.calls, "chunk": MX.CHUNK, "sizes": []}
    for n in args.sizes:
        rows, labels, score = generated(n, n)
        cs = MX.build_cluster_set(rows, labels.tolist())
        t0 = time.perf_counter()
        draws = MX.draw_cluster_samples(cs, np.random.default_rng(1), R)
        draw_s = time.perf_counter() - t0
        d = {k: torch.as_tensor(v).to(dev) for k, v in (("score", score), ("label", labels), ("cluster", cs.cluster), ("draws", draws))}

        def call():
            return MX.bootstrap_binary_metrics(d["score"], d["label"], 0.5, d["cluster"], d["draws"], n_clusters=cs.n_clusters)
        call()
        call()
        torch.cuda.synchronize()
        windows = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                out = call()
            b.record()
            torch.cuda.synchronize()
            windows.append(a.elapsed_time(b) / args.calls)
        device_ms = float(np.median(windows))
        h = min(args.host_replicates, R)
        t0 = time.perf_counter()
        host = boot_metrics_numpy(score, labels, 0.5, cs.cluster, draws[:h], cs.n_clusters)
        host_s = time.perf_counter() - t0
        assert_matches(out[:h].cpu().numpy(), host, n, f"N={n}")   # restatement against restatement: the same bound as the tests
        rec = {"frames": n, "clusters": cs.n_clusters, "device_ms_per_call": round(device_ms, 3),
               "device_ms_per_call_windows": [round(w, 3) for w in windows],
               "device_us_per_replicate": round(device_ms * 1e3 / R, 3), "host_numpy_ms_per_replicate": round(host_s * 1e3 / h, 3),
               "host_numpy_s_for_all_replicates": round(host_s / h * R, 2), "host_draws_s": round(draw_s, 3),
               "host_over_device": round(host_s / h * R * 1e3 / device_ms, 1)}
        result["sizes"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
