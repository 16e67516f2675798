"""Timing of the threshold selection on the device beside the NumPy restatement of the same selection on this host (needs the GPU;
no test gates on these numbers).  Generated scores (sigmoid-like f64, continuous: nearly every score is a distinct value, so the
candidate list is the 200-of-U one), N = 6 600 and 15 840 frames, M = 1 and 30 runs, policies f1_opt_on_val and youden: device
events around --calls calls of metrics.select_threshold after warm-up (the sort, the workspace and the launch included, nothing read
back inside the window), the window repeated --repeats times so that the spread is known (the median is reported), and the wall time
of tests/thresholds_ref.select_numpy on one core for the same M runs (measured in full, once).  Before timing, the device rows are
checked equal to the restatement's.  `device` is the name the runtime gives the card, which may be a generic one; `arch` is its ISA
(gfx950 on an MI355X).  Writes profiles/select_tau.json and prints it.

    python tools/select_tau_bench.py [--calls 200] [--repeats 5] [--out FILE]
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


def generated(n, runs, seed):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.4).astype(np.uint8)
    score = 1.0 / (1.0 + np.exp(-(1.5 * (2.0 * labels[None, :] - 1.0) + rng.normal(0.0, 2.0, (runs, n)))))
    return labels, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[6600, 15840])
    ap.add_argument("--runs", type=int, nargs="*", default=[1, 30])
    ap.add_argument("--policies", nargs="*", default=["f1_opt_on_val", "youden"])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "select_tau.json"))
    args = ap.parse_args()
    import torch
    from thresholds_ref import assert_equal, select_numpy
    from ssl4polyp_amd import metrics as MX
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "calls": args.calls,
              "repeats": args.repeats, "note": "device_ms_per_call: sort + one pm_select_tau launch, median of the windows; "
                                               "host_numpy_ms: tests/thresholds_ref.select_numpy on one core, measured once",
              "cases": []}
    for n in args.sizes:
        for runs in args.runs:
            labels, score = generated(n, runs, n + runs)
            d_score, d_label = torch.from_numpy(score).to(dev), torch.from_numpy(labels).to(dev)
            for policy in args.policies:
                t0 = time.perf_counter()
                host_rows, _ = select_numpy(score, labels, policy)
                host_ms = (time.perf_counter() - t0) * 1e3
                out = MX.select_threshold(d_score, d_label, policy)
                assert_equal(out.cpu().numpy(), host_rows, f"N={n} M={runs} {policy}")
                MX.select_threshold(d_score, d_label, policy)
                torch.cuda.synchronize()
                windows = []
                for _ in range(args.repeats):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.calls):
                        out = MX.select_threshold(d_score, d_label, policy)
                    b.record()
                    torch.cuda.synchronize()
                    windows.append(a.elapsed_time(b) / args.calls)
                device_ms = float(np.median(windows))
                rec = {"frames": n, "runs": runs, "policy": policy, "n_unique": host_rows[:, 14].tolist()[:3],
                       "device_ms_per_call": round(device_ms, 4), "device_ms_per_call_windows": [round(w, 4) for w in windows],
                       "host_numpy_ms": round(host_ms, 3), "host_over_device": round(host_ms / device_ms, 1)}
                result["cases"].append(rec)
                print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
