"""Stand-alone time of pm_layernorm_bwd (ln_bwd_kernel + its reduce launch) with HIP events, optionally beside a parent build.

    python tools/ln_bwd_bench.py [--parent DIR] [--shapes M,D ...] [--precision bf16] [--calls 20] [--windows 5]

One JSON line per shape: microseconds per call (the median of `--windows` windows of `--calls` back-to-back calls, every window
listed), the algorithmic GB/s of that median (dy + x + dres in, dx + dx_act out), and with --parent DIR (a checkout of the commit
to compare with, its library built: DIR/ssl4polyp_amd/lib/libpolypmae.so, or the library file itself) the same for the parent's
library in the same process, windows alternating, plus whether dx / dx_act and the three column sums are bit-identical to the
parent's (they are as long as both builds bound the grid alike; another bound is another association of the sums).  The default
shapes are the ViT-B/16 fine-tune step at bs 64 and 32 and the MAE decoder at bs 256.

A stand-alone figure says what the kernel can do with the whole device; inside the step it shares the CUs with the weight
gradients, and only the in-step A/B (profiles/README.md) decides a default."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--shapes", nargs="*", default=["12608,768", "6304,768", "50432,512"])
    ap.add_argument("--precision", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import torch
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import Kernels, _ptr, _stream

    k = Kernels(args.precision)
    libs = {"new": k.lib}
    if args.parent:
        path = args.parent if args.parent.endswith(".so") else os.path.join(args.parent, "ssl4polyp_amd", "lib", "libpolypmae.so")
        libs["parent"] = ctypes.CDLL(path)
        libs["parent"].pm_layernorm_bwd.restype = ctypes.c_int
        libs["parent"].pm_layernorm_bwd.argtypes = _lib.SIGNATURES["pm_layernorm_bwd"]
    dev = torch.device("cuda:0")
    for shape in args.shapes:
        M, D = (int(v) for v in shape.split(","))
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(M, D, generator=g) * 2 + 0.5).to(dev)
        gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
        beta = torch.zeros(D, device=dev)
        dy = torch.randn(M, D, generator=g).to(dev).to(k.act_dtype)
        dres = torch.randn(M, D, generator=g).to(dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        k.layernorm_fwd(x, gamma, beta, torch.empty(M, D, dtype=k.act_dtype, device=dev), mean, rstd, M, D)
        ws = torch.empty(int(k.lib.pm_workspace_bytes(_lib.WS_LAYERNORM_BWD, M, D)), dtype=torch.uint8, device=dev)
        out = {n: dict(dx=torch.empty(M, D, device=dev), dx_act=torch.empty(M, D, dtype=k.act_dtype, device=dev),
                       sums=[torch.zeros(D, device=dev) for _ in range(3)]) for n in libs}

        def call(n):
            o = out[n]
            _lib.check(libs[n].pm_layernorm_bwd(_ptr(dy), k.act, _ptr(x), D, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres), D,
                                                _ptr(o["dx"]), D, _ptr(o["dx_act"]), k.act, _ptr(o["sums"][0]), _ptr(o["sums"][1]),
                                                _ptr(o["sums"][2]), M, D, _ptr(ws), ws.numel(), _stream()), "pm_layernorm_bwd")

        rec = {"M": M, "D": D, "precision": args.precision, "calls": args.calls}
        for n in libs:  # one call each on zeroed sums: the results to compare
            call(n)
        torch.cuda.synchronize()
        if "parent" in libs:
            rec["dx_equals_parent"] = bool(torch.equal(out["new"]["dx"], out["parent"]["dx"]))
            rec["dx_act_equals_parent"] = bool(torch.equal(out["new"]["dx_act"], out["parent"]["dx_act"]))
            rec["sums_equal_parent"] = [bool(torch.equal(a, b)) for a, b in zip(out["new"]["sums"], out["parent"]["sums"])]
            rec["sums_max_rel_to_parent"] = [float(((a - b).abs().max() / b.abs().max()).item())
                                             for a, b in zip(out["new"]["sums"], out["parent"]["sums"])]
        for n in libs:
            for _ in range(5):
                call(n)
        times = {n: [] for n in libs}
        for _ in range(args.windows):
            for n in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    call(n)
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        act_b = 4 if args.precision == "fp32" else 2
        for n in libs:
            med = statistics.median(times[n])
            rec[f"{n}_us"] = round(med, 2)
            rec[f"{n}_us_windows"] = [round(t, 2) for t in times[n]]
            rec[f"{n}_gb_per_s"] = round(M * D * (act_b + 4 + 4 + 4 + act_b) / med / 1e3, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
