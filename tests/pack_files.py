"""The ten-file test batch of the pack-input and fused-decode tests (not a test module): eight baseline JPEGs that jpeg.parse_jpeg
sends to the device path -- every sampling, odd sizes, the replication and the smallest fancy-upsampled widths, grey, own Huffman
tables -- and two files the packer decodes on the host (a progressive JPEG, a PNG)."""
import io
import os

import numpy as np


def frame(H, W, seed):
    """(the `_frame` pattern of tests/test_gpu_ragged_input.py)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / (7.0 + seed) + c) * np.cos(yy / 11.0 - c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 20, (H, W, 3)), 0, 255).astype(np.uint8)


# (H, W), extension, Image.save arguments, grey
SPECS = (
    ((37, 53), "jpg", dict(subsampling=2, quality=90), False),                  # 0 odd size: last chroma row / column clamps
    ((5, 3), "jpg", dict(subsampling=2, quality=90), False),                    # 1 downsampled width 2: replication
    ((6, 5), "jpg", dict(subsampling=2, quality=90), False),                    # 2 downsampled width 3: smallest fancy-upsampled
    ((4, 4), "jpg", dict(subsampling=1, quality=90), False),                    # 3 h2v1 replication
    ((33, 17), "jpg", dict(subsampling=1, quality=75), False),                  # 4 h2v1 fancy, not a multiple of the MCU
    ((16, 16), "jpg", dict(subsampling=0, quality=95), False),                  # 5 no upsampling
    ((40, 40), "jpg", dict(quality=90), True),                                  # 6 grey
    ((160, 200), "jpg", dict(subsampling=2, quality=90, optimize=True), False),  # 7 several MCU rows, own Huffman tables
    ((48, 64), "jpg", dict(progressive=True, quality=90), False),               # 8 host fallback
    ((30, 20), "png", dict(), False),                                           # 9 host fallback
)
FALLBACK = [8, 9]
SIZES = [s[0] for s in SPECS]


def encode(arr, ext="jpg", grey=False, **save):
    from PIL import Image
    img = Image.fromarray(arr)
    if grey:
        img = img.convert("L")
    buf = io.BytesIO()
    img.save(buf, format="JPEG" if ext == "jpg" else "PNG", **save)
    return buf.getvalue()


def make_files(seed=100):
    """[(file name, bytes)] of the ten files."""
    return [(f"f{i:02d}.{ext}", encode(frame(H, W, seed + i), ext, grey, **save)) for i, ((H, W), ext, save, grey) in enumerate(SPECS)]


def pil_rgb(data):
    from PIL import Image
    return Image.open(io.BytesIO(data)).convert("RGB")


def pil_resized(data, S, box=None, bicubic=False):
    """Pillow's [crop((l, t, l + w, t + h)).]resize((S, S)) of the file, uint8 [S, S, 3]."""
    from PIL import Image
    img = pil_rgb(data)
    if box is not None:
        t, l, h, w = (int(v) for v in box)
        img = img.crop((l, t, l + w, t + h))
    return np.asarray(img.resize((S, S), Image.BICUBIC if bicubic else Image.BILINEAR))


ROW_VARIANTS = ("blur_1p5", "clean", "bc_b1p3_c0p7", "occ_a0p2", "jpeg_q40")
CSV_COLUMNS = ("dataset", "frame_id", "frame_path", "label", "store_id", "variant", "jpeg_q")


def write_pack(root, files=None, root_key="store"):
    """The files under <root>/frames, and <root>/pack.csv whose frame_path values go through the roots map {root_key: <root>/frames}.
    Returns (csv path, roots map, [file bytes], [labels])."""
    import csv
    files = files if files is not None else make_files()
    os.makedirs(os.path.join(root, "frames", "img"))
    labels = []
    path = os.path.join(root, "pack.csv")
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
        w.writeheader()
        for i, (name, data) in enumerate(files):
            with open(os.path.join(root, "frames", "img", name), "wb") as out:
                out.write(data)
            variant = ROW_VARIANTS[i] if i < len(ROW_VARIANTS) else "clean"
            labels.append(i % 2)
            w.writerow({"dataset": "TEST", "frame_id": f"case/{name}", "frame_path": f"{root_key}/img/{name}", "label": i % 2,
                        "store_id": "elsewhere", "variant": variant, "jpeg_q": 40 if variant == "jpeg_q40" else -1})
    return path, {root_key: os.path.join(root, "frames")}, [d for _, d in files], labels
