"""Stand-alone time of the ViT-B/16 optimizer update (HIP events): pm_adamw_tick + pm_adamw_dev per segment, and one
pm_adamw_segments call at each grid bound when the library has it.

    python tools/adamw_bench.py [--lib PATH] [--calls 30] [--bounds 0 64 128 256 512 1024 2048]

The 17 segments of the fine-tune step: three vector ranges, the patch embedding, twelve blocks of 7 077 888 matrix elements, the
head; f32 p / g / m / v and a bf16 shadow, 30 B per parameter, 2.57 GB per update.  --lib: another build of the library (the
parent commit's, for a before / after in two processes).  One line per way of launching: microseconds per update and TB/s.

A stand-alone figure says what the kernel can do with the whole device; beside the next forward the update shares HBM with it, and
only the step rate (profiles/README.md, "AdamW footprint") chooses the bound."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [152064, 122112, 64, 589824] + [7077888] * 12 + [1536]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--bounds", type=int, nargs="*", default=[0, 64, 128, 256, 512, 1024, 2048])
    args = ap.parse_args()
    import torch
    from ssl4polyp_amd import _lib
    path = args.lib or _lib.LIB_PATH
    lib = ctypes.CDLL(path)
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.pm_adamw_dev.argtypes = [P, P, P, P, P, I, L, P, P]
    lib.pm_adamw_tick.argtypes = [P, I, P]
    tot, dev = sum(SIZES), "cuda:0"
    p, g, m, v = (torch.randn(tot, device=dev) * 0.02 for _ in range(4))
    v.abs_()
    sh = torch.zeros(tot, device=dev, dtype=torch.bfloat16)
    hyper = torch.zeros(1, 16, device=dev)
    hyper[0, :6] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0])
    st = torch.cuda.current_stream().cuda_stream
    offs = [sum(SIZES[:i]) for i in range(len(SIZES))]
    ptrs = [(p.data_ptr() + 4 * o, g.data_ptr() + 4 * o, m.data_ptr() + 4 * o, v.data_ptr() + 4 * o, sh.data_ptr() + 2 * o) for o in offs]

    def per_segment():
        lib.pm_adamw_tick(hyper.data_ptr(), 1, st)
        for a, n in zip(ptrs, SIZES):
            lib.pm_adamw_dev(*a, _lib.PM_BF16, n, hyper.data_ptr(), st)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.calls * 1e3

    def line(what, us):
        print(f"{what}: {us:.1f} us per update, {tot * 30 / us / 1e6:.2f} TB/s")

    print(f"{path}: {len(SIZES)} segments, {tot * 30 / 1e9:.2f} GB per update")
    line("pm_adamw_tick + pm_adamw_dev per segment", timed(per_segment))
    if hasattr(lib, "pm_adamw_segments"):
        lib.pm_adamw_segments.argtypes = [P, I, P, I, P, P, I]
        segs = (_lib.AdamwSegment * len(SIZES))(*[_lib.AdamwSegment(*a, _lib.PM_BF16, n, hyper.data_ptr(), None)
                                                   for a, n in zip(ptrs, SIZES)])
        for bound in args.bounds:
            line(f"pm_adamw_segments, max_blocks {bound}", timed(lambda: lib.pm_adamw_segments(segs, len(SIZES), hyper.data_ptr(), 1, None, st, bound)))


if __name__ == "__main__":
    main()
