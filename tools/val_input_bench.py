"""The validation input of the MAE recipes on the device (HIP events and wall clock around a synchronise).

    python tools/val_input_bench.py --kernel [--batch 64] [--calls 50]                     # (a) the Resize + CenterCrop call alone
    python tools/val_input_bench.py --passes [--files 4096] [--workers 14] [--batch 64]    # (b) whole validation passes
    python tools/val_input_bench.py --kernel --passes --out profiles/val_input.json

(a) DeviceAugmenter.resize_center_crop(resize 256, crop 224) over B ragged noise frames of 576 x 720 and of 1080 x 1350: us per
    call (median, min, max of 5 windows of `calls` calls) and the bytes the algorithm moves per second -- the source region the
    window's taps read, the u8 temporary written and read once, the output written -- counted from the shapes below.
(b) A folder of `files` baseline JPEGs (quality 90, 4:2:0; half 576 x 720, half 1080 x 1350; eight pictures per size encoded with
    Pillow and written under many names) is made in a temporary directory; then, in one process, the three inputs of
    mae_recipe.build_val_loader alternate `rounds` times over a ViT-B/16 probe in bf16: host (Pillow in the workers),
    --val_transform device, --val_transform device --decode device.  Each pass is
    train.evaluate_probe over the whole folder, wall clock around its closing read-back, workers already running (a first pass
    per loader is not timed).  Beside them: the evaluation forward alone on a resident batch, img/s."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(576, 720), (1080, 1350)]
RESIZE, CROP = 256, 224


def span(in_size: int, out_size: int, first: int, count: int) -> int:
    """How many source lines the bicubic taps of the outputs first .. first + count - 1 read (Resample.c precompute_coeffs)."""
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    lo = max(int((first + 0.5) * scale - support + 0.5), 0)
    hi = min(int((first + count - 0.5) * scale + support + 0.5), in_size)
    return hi - lo


def events_us(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def kernel(torch, batch, calls):
    import numpy as np
    from ssl4polyp_amd.data import DeviceAugmenter, RaggedFrames, center_crop_windows
    dev = torch.device("cuda", 0)
    aug = DeviceAugmenter(dev, size=CROP)
    out = {}
    for h, w in SIZES:
        rng = np.random.default_rng(h)
        frames = RaggedFrames.from_frames([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(batch)]).to(dev)
        nh, nw, top, left = (int(v) for v in center_crop_windows([(h, w)], RESIZE, CROP)[0])
        rows, cols = span(h, nh, top, CROP), span(w, nw, left, CROP)
        nbytes = batch * 3 * (rows * cols + 2 * rows * CROP + CROP * CROP)
        fn = lambda: aug.resize_center_crop(frames, RESIZE)   # noqa: E731
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = sorted(events_us(torch, fn, calls) for _ in range(5))
        out[f"{h}x{w}"] = {"batch": batch, "us_median": us[2], "us_min": us[0], "us_max": us[4], "source_rows": rows, "source_cols": cols,
                           "bytes": nbytes, "TB_per_s_median": nbytes / us[2] / 1e6, "frames_per_s_median": batch / us[2] * 1e6}
        print(f"resize_center_crop B={batch} {h}x{w}: median {us[2]:.1f} us (min {us[0]:.1f}, max {us[4]:.1f}) of 5 x {calls} calls; "
              f"{nbytes / 1e6:.1f} MB moved, {nbytes / us[2] / 1e6:.3f} TB/s; {batch / us[2] * 1e6:.0f} frames/s")
    return out


def write_folder(root, files, variants=8):
    """`files` JPEGs under root/val/class{0..3}, the sizes alternating; `variants` distinct pictures per size are encoded once and
    written under many names (decoding and resizing cost the same whatever the name)."""
    import io
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:1080, 0:1350]
    encoded = {}
    for s, (h, w) in enumerate(SIZES):
        for v in range(variants):
            base = 110 + 60 * np.sin(yy[:h, :w] / (9.0 + v)) + 50 * np.cos(xx[:h, :w] / (11.0 + 2 * v))
            img = np.clip(base[..., None] + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=90, subsampling=2)
            encoded[(s, v)] = buf.getvalue()
    for c in range(4):
        os.makedirs(os.path.join(root, "val", f"class{c}"), exist_ok=True)
    for i in range(files):
        with open(os.path.join(root, "val", f"class{i % 4}", f"{i:05d}.jpg"), "wb") as fh:
            fh.write(encoded[(i % 2, (i // 2) % variants)])


def passes(torch, files, workers, batch, rounds):
    from ssl4polyp_amd import mae_recipe, models_vit
    from ssl4polyp_amd.train import evaluate_probe
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models_vit.vit_base_patch16(num_classes=4, precision="bf16")
    torch.nn.init.trunc_normal_(model.head.weight, std=0.01)
    models_vit.add_probe_head(model).to(dev).eval()
    modes = {"host": dict(val_transform="host", decode="host"), "val_transform_device": dict(val_transform="device", decode="host"),
             "val_transform_device_decode_device": dict(val_transform="device", decode="device")}
    out = {"files": files, "workers": workers, "batch": batch, "sizes": SIZES, "img_per_s": {k: [] for k in modes}}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.time()
        write_folder(root, files)
        print(f"wrote {files} JPEGs in {time.time() - t0:.1f} s")
        inputs, records = {}, {}
        for name, mode in modes.items():
            args = types.SimpleNamespace(data_path=root, batch_size=batch, num_workers=workers, pin_mem=True, **mode)
            inputs[name] = mae_recipe.build_val_loader(args, dev, CROP)
            records[name] = evaluate_probe(model, inputs[name][0], dev, inputs[name][1])   # (starts the workers; not timed)
        assert all(r == records["host"] for r in records.values()), "the three inputs must give the same record"
        for _ in range(rounds):
            for name, (loader, prepare) in inputs.items():
                torch.cuda.synchronize()
                t0 = time.time()
                evaluate_probe(model, loader, dev, prepare)   # (ends in a read-back: the device is done)
                out["img_per_s"][name].append(files / (time.time() - t0))
        del inputs
    imgs = torch.randn(batch, 3, CROP, CROP, device=dev)
    with torch.no_grad():
        for _ in range(3):
            model(imgs)
        torch.cuda.synchronize()
        fwd = sorted(events_us(torch, lambda: model(imgs), 20) for _ in range(5))
    out["forward_resident_img_per_s"] = batch / fwd[2] * 1e6
    out["img_per_s_median"] = {k: statistics.median(v) for k, v in out["img_per_s"].items()}
    for k, v in out["img_per_s"].items():
        print(f"validation pass, {k}: median {statistics.median(v):.0f} img/s of {[round(x) for x in v]}")
    print(f"evaluation forward on a resident batch of {batch}: {out['forward_resident_img_per_s']:.0f} img/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="frames per call / per batch (default 64)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=14)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("val_input_bench: no GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "host": os.uname().nodename, "resize": RESIZE, "crop": CROP}
    if args.kernel:
        result["kernel"] = kernel(torch, args.batch or 64, args.calls)
    if args.passes:
        result["passes"] = passes(torch, args.files, args.workers, args.batch or 64, args.rounds)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
