"""Timing of the device JPEG decoder on generated batches of 64 (needs the GPU; bench.py measures the training step, this
measures the decode alone).  Per batch it prints one JSON line: compressed MB, subsequences, packing files/s on one core, decode
ms per call (device events around 10 calls after warm-up) for mode="parallel" and mode="interval", and the counters.

    python tools/jpeg_decode_bench.py [--batches NAME ...] [--parent DIR] [--sync-rounds N ...] [--calls 10]
    python tools/jpeg_decode_bench.py --write-folder DIR --files 2000      # the mixed folder for main_pretrain --data_path

--parent DIR: a checkout of the commit to compare with, its library built (DIR/ssl4polyp_amd/lib/libpolypmae.so).  Its
pm_jpeg_decode is called on the same device tensors, alternating with this tree's decoder and twice, so that the spread of the old
time is known; every decoded batch is compared with its bytes.  Its packer (DIR/ssl4polyp_amd/jpeg.py) is timed beside this one.
For the per-kernel times run this script under `rocprofv3 --kernel-trace --stats -- python tools/jpeg_decode_bench.py ...`
in a run of its own.  POLYPMAE_LIB / --subseq-bytes select a side build with another subsequence size."""
import argparse
import ctypes
import importlib.util
import io
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

_BASE = {}


def sin_noise(h, w, seed, sigma=6.0):
    """sinusoids (one base per size) + per-seed Gaussian noise"""
    if (h, w) not in _BASE:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        _BASE[(h, w)] = np.stack([127 + 90 * np.sin(xx / (17 + 5 * c) + yy / (23 - 3 * c) + c) for c in range(3)], -1)
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.clip(_BASE[(h, w)] + rng.normal(0, sigma, (h, w, 3)).astype(np.float32), 0, 255).astype(np.uint8)


def endo_like(h, w, seed):
    """a textured disc on a black frame with a flat box"""
    img = sin_noise(h, w, seed, 4.0)
    yy, xx = np.mgrid[0:h, 0:w]
    img[((yy - h / 2) ** 2 / (h * 0.48) ** 2 + (xx - w * 0.55) ** 2 / (w * 0.42) ** 2) > 1] = 0
    img[int(h * .7):int(h * .95), int(w * .02):int(w * .18)] = (0, 140, 60)
    return img


def encode(arr, optimize=False):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=90, subsampling=2, optimize=optimize)
    return b.getvalue()


MIX = ((576, 720), (1080, 1920), (480, 640), (531, 611))
BATCHES = {
    "576x720": lambda n: [encode(sin_noise(576, 720, s)) for s in range(n)],
    "576x720_optimize": lambda n: [encode(sin_noise(576, 720, s), True) for s in range(n)],
    "1080x1920": lambda n: [encode(sin_noise(1080, 1920, s)) for s in range(n)],
    "mixed": lambda n: [encode(sin_noise(*MIX[s % 4], s)) for s in range(n)],
    "endoscopy_like": lambda n: [encode(endo_like(576, 720, s)) for s in range(n)],
}


def _write_one(job):
    d, s = job
    with open(os.path.join(d, f"{s:05d}.jpg"), "wb") as f:
        f.write(encode(sin_noise(*MIX[s % 4], s)))


def pack_rate(from_bytes, files, min_seconds=1.0):
    from_bytes(files[:2])
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_seconds:
        from_bytes(files)
        n += len(files)
    return n / (time.perf_counter() - t0)


def timed(fn, calls, torch):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", default=list(BATCHES), choices=list(BATCHES))
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--sync-rounds", type=int, nargs="*", default=[2])
    ap.add_argument("--subseq-bytes", type=int, default=None, help="with POLYPMAE_LIB naming a library built with the same value")
    ap.add_argument("--no-interval", action="store_true", help="skip mode='interval' (slow)")
    ap.add_argument("--write-folder", default=None)
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--jobs", type=int, default=8, help="processes that write the folder")
    args = ap.parse_args()
    if args.write_folder:
        d = os.path.join(args.write_folder, "unlabelled")
        os.makedirs(d, exist_ok=True)
        import concurrent.futures
        with concurrent.futures.ProcessPoolExecutor(args.jobs) as ex:
            list(ex.map(_write_one, [(d, s) for s in range(args.files)], chunksize=16))
        return
    import torch
    from ssl4polyp_amd import jpeg
    from ssl4polyp_amd.data import DeviceJpegDecoder
    if args.subseq_bytes:
        jpeg.SUBSEQ_BYTES = args.subseq_bytes
    dev = torch.device("cuda", 0)
    parent_lib = parent_jpeg = None
    if args.parent:
        parent_lib = ctypes.CDLL(os.path.join(args.parent, "ssl4polyp_amd", "lib", "libpolypmae.so"))
        parent_lib.pm_jpeg_decode.restype = ctypes.c_int
        from ssl4polyp_amd._lib import SIGNATURES
        parent_lib.pm_jpeg_decode.argtypes = SIGNATURES["pm_jpeg_decode"]
        spec = importlib.util.spec_from_file_location("parent_jpeg", os.path.join(args.parent, "ssl4polyp_amd", "jpeg.py"))
        parent_jpeg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent_jpeg)
    for name in args.batches:
        files = BATCHES[name](args.batch_size)
        jb = jpeg.JpegBatch.from_bytes(files)
        rec = {"batch": name, "files": len(files), "compressed_MB": round(sum(map(len, files)) / 1e6, 2),
               "subseq_bytes": jpeg.SUBSEQ_BYTES, "subsequences": jb.meta["n_subseq"], "huffman_tables": jb.huff.shape[0],
               "pack_files_per_s": round(pack_rate(jpeg.JpegBatch.from_bytes, files), 1)}
        if parent_jpeg is not None:
            rec["parent_pack_files_per_s"] = round(pack_rate(parent_jpeg.JpegBatch.from_bytes, files), 1)
        d = jb.to(dev)
        want = None
        if parent_lib is not None:
            m, t = jb.meta, d.t
            coef = torch.empty(m["blocks"] * 64, dtype=torch.int16, device=dev)
            planes = torch.empty(m["blocks"] * 64, dtype=torch.uint8, device=dev)
            out = torch.empty(m["nbytes"], dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def parent_call():
                rc = parent_lib.pm_jpeg_decode(t["entropy"].data_ptr(), t["entropy"].numel(), t["intervals"].data_ptr(),
                                               t["intervals"].shape[0], t["frames"].data_ptr(), t["frames"].shape[0],
                                               t["huff"].data_ptr(), t["huff"].shape[0], t["quant"].data_ptr(), t["quant"].shape[0],
                                               None, 0, None, 0, coef.data_ptr(), planes.data_ptr(), m["blocks"], m["pixels"],
                                               out.data_ptr(), m["nbytes"], st)
                assert rc == 0, rc
            rec["parent_ms"] = [round(timed(parent_call, args.calls, torch), 3)]
            want = out.clone()
        for r in args.sync_rounds:
            dec = DeviceJpegDecoder(dev, mode="parallel", sync_rounds=r)
            rec[f"parallel_ms_rounds{r}"] = round(timed(lambda: dec(d), args.calls, torch), 3)
            rec[f"stats_rounds{r}"] = dec.stats()
            got = dec(d).data
            torch.cuda.synchronize()
            if want is not None:
                rec[f"equals_parent_rounds{r}"] = bool(torch.equal(got, want))
        if parent_lib is not None:
            rec["parent_ms"].append(round(timed(parent_call, args.calls, torch), 3))
        if not args.no_interval:
            dec = DeviceJpegDecoder(dev, mode="interval")
            rec["interval_ms"] = round(timed(lambda: dec(d), args.calls, torch), 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
