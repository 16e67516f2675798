"""Timing of the pack input path (needs the GPU; bench.py measures the training step, this measures what feeds it).

    python tools/pack_input_bench.py stage [--sizes 576x720 1080x1240 1080x1920] [--batch-size 64] [--calls 10]
    python tools/pack_input_bench.py e2e --pack DIR [--files 2000] [--size 1080x1240] [--batch-size 64] [--num-workers 14]

stage: the first stage of the transform alone on generated q90 4:2:0 batches (tools/jpeg_decode_bench.py's generator): the two-step
path -- DeviceJpegDecoder, then DeviceAugmenter.resize of the decoded RaggedFrames -- against DeviceJpegDecoder.resized_crop, in one
process on the same device arrays, alternating; ms per call from device events over `--calls` calls after warm-up, the peak device
memory of each path above what the batch itself holds, and whether the bytes agree.  One JSON line per size.  For the per-kernel
split run it under `rocprofv3 --kernel-trace --stats -- python tools/pack_input_bench.py stage ...` in a run of its own.

e2e: writes (once) a pack of `--files` generated frames + a CSV under --pack, then times train.evaluate_cls over
packs.device_pack_loaders for decode = host / device / device + fused_decode: img/s of the second pass (workers alive, buffers
grown).  One JSON line per mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpeg_decode_bench import encode, sin_noise, timed  # noqa: E402


def _size(s):
    h, w = s.lower().split("x")
    return int(h), int(w)


def _write_one(job):
    d, s, h, w = job
    with open(os.path.join(d, f"{s:05d}.jpg"), "wb") as f:
        f.write(encode(sin_noise(h, w, s)))


def stage(args):
    import torch
    from ssl4polyp_amd import jpeg
    from ssl4polyp_amd.data import DeviceAugmenter, DeviceJpegDecoder
    dev = torch.device("cuda", 0)
    for name in args.sizes:
        h, w = _size(name)
        files = [encode(sin_noise(h, w, s)) for s in range(args.batch_size)]
        jb = jpeg.JpegBatch.from_bytes(files)
        d = jb.to(dev)
        boxes = np.zeros((len(files), 4), dtype=np.int32)
        boxes[:, 2:] = jb.meta["hw"]
        rec = {"frames": name, "files": len(files), "compressed_MB": round(sum(map(len, files)) / 1e6, 2), "out": args.out,
               "decoded_MB": round(jb.meta["nbytes"] / 1e6, 1)}
        results = {}
        for path in ("two_step", "fused"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            dec, aug = DeviceJpegDecoder(dev), DeviceAugmenter(dev, size=args.out)
            if path == "two_step":
                fn = lambda dec=dec, aug=aug: aug.resize(dec(d))
            else:
                fn = lambda dec=dec: dec.resized_crop(d, boxes, args.out, False)
            ms = [round(timed(fn, args.calls, torch), 3)]
            results[path] = (fn, ms)
            rec[path + "_peak_MB"] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)
            rec[path + "_out"] = fn().clone()
        for path, (fn, ms) in results.items():   # once more, alternating: the spread
            ms.append(round(timed(fn, args.calls, torch), 3))
            rec[path + "_ms"] = ms
        rec["equal_bytes"] = bool(torch.equal(rec.pop("two_step_out"), rec.pop("fused_out")))
        print(json.dumps(rec), flush=True)
        del fn, results, rec, dec, aug   # (whatever holds a decoder: freed before the next size's baseline is read)


def e2e(args):
    import csv

    import torch
    h, w = _size(args.size)
    d = os.path.join(args.pack, "frames")
    csv_path = os.path.join(args.pack, "test.csv")
    if not os.path.exists(csv_path):
        os.makedirs(d, exist_ok=True)
        import concurrent.futures
        with concurrent.futures.ProcessPoolExecutor(args.jobs) as ex:
            list(ex.map(_write_one, [(d, s, h, w) for s in range(args.files)], chunksize=16))
        with open(csv_path, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(["frame_path", "label", "store_id", "variant"])
            for s in range(args.files):
                wr.writerow([f"{s:05d}.jpg", s % 2, "frames", "clean"])
    import ssl4polyp_amd as A
    from ssl4polyp_amd.packs import device_pack_loaders, read_pack_csv
    from ssl4polyp_amd.train import evaluate_cls
    dev = torch.device("cuda", 0)
    split = read_pack_csv(csv_path, {"frames": d})
    torch.manual_seed(0)
    model = A.get_MAE_backbone(None, True, 2, False, None, precision=args.precision).to(dev)
    ref = None
    for mode, decode, fused in (("host", "host", False), ("device", "device", False), ("device_fused", "device", True)):
        if mode not in args.modes:
            continue
        loaders, _ = device_pack_loaders({"test": split}, dev, args.batch_size, decode=decode, num_workers=args.num_workers,
                                         fused_decode=fused)
        rates = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logits, targets = evaluate_cls(model, loaders["test"], dev)
            rates.append(round(len(targets) / (time.perf_counter() - t0), 1))
        rec = {"mode": mode, "frames": args.size, "files": len(targets), "batch_size": args.batch_size, "num_workers": args.num_workers,
               "precision": args.precision, "img_per_s_first_pass": rates[0], "img_per_s": rates[1],
               "peak_device_MB": round(torch.cuda.max_memory_allocated(dev) / 1e6, 1)}
        if ref is None:
            ref = logits
        rec["equal_logits"] = bool(torch.equal(logits, ref))
        print(json.dumps(rec), flush=True)
        del loaders


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stage")
    s.add_argument("--sizes", nargs="*", default=["576x720", "1080x1240", "1080x1920"], help="H x W (SUN frames are 1240 wide, 1080 high)")
    s.add_argument("--batch-size", type=int, default=64)
    s.add_argument("--calls", type=int, default=10)
    s.add_argument("--out", type=int, default=224)
    e = sub.add_parser("e2e")
    e.add_argument("--pack", required=True)
    e.add_argument("--files", type=int, default=2000)
    e.add_argument("--size", default="1080x1240")
    e.add_argument("--batch-size", type=int, default=64)
    e.add_argument("--num-workers", type=int, default=14)
    e.add_argument("--jobs", type=int, default=14, help="processes that write the pack")
    e.add_argument("--precision", default="bf16")
    e.add_argument("--modes", nargs="*", default=["host", "device", "device_fused"])
    args = ap.parse_args()
    (stage if args.cmd == "stage" else e2e)(args)


if __name__ == "__main__":
    main()
