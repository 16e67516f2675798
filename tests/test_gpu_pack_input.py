"""The pack input path on the device (packs.device_pack_loaders over data.DevicePrefetcher, main_finetune.run): a ten-file pack of
mixed sizes and formats with Exp-5 style rows, every image against Pillow's resize of the FILE followed by the oracle's stages,
bit for bit; evaluate_cls and a short fine-tune over it."""
import json
import os

import numpy as np
import pytest
import torch

from pack_files import encode, frame, pil_resized, write_pack

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    from ssl4polyp_amd.packs import read_pack_csv
    root = str(tmp_path_factory.mktemp("pack"))
    csv_path, roots, files, labels = write_pack(root)
    paths, lab, rows = read_pack_csv(csv_path, roots)
    assert lab == labels == [0, 1] * 5
    return (paths, lab, rows), files


@pytest.fixture(scope="module")
def resized(pack):
    """Pillow's Resize((224, 224)) of every file: computed once, never modified."""
    x = np.stack([pil_resized(f, 224) for f in pack[1]])
    x.setflags(write=False)
    return x


def _perturbed(resized, rows):
    from oracle import augment_ref as R
    from ssl4polyp_amd import data as D
    out = []
    for img, row in zip(resized, rows):
        plan = D.perturbation_plan(row)
        if plan[0] == "blur":
            img = R.pil_gaussian_blur(img, plan[1])
        elif plan[0] == "bc":
            img = R.brightness_contrast(img, plan[1], plan[2])
        elif plan[0] == "occ":
            img = R.occlude(img, D.occlusion_rect(plan[1], plan[2], 224, 224))
        elif plan[0] == "jpeg":
            img = R.jpeg_roundtrip(img, plan[1])
        out.append(img)
    return np.stack(out)


@pytest.fixture(scope="module")
def eval_images(pack, resized):
    """(perturbations on, perturbations off) f32 [10, 3, 224, 224] on the host, from the oracle."""
    from oracle.input_ref import to_tensor_normalize
    from ssl4polyp_amd import data as D
    rows = pack[0][2]
    assert [D.perturbation_plan(r)[0] for r in rows] == ["blur", "none", "bc", "occ", "jpeg"] + ["none"] * 5
    return to_tensor_normalize(torch.from_numpy(_perturbed(resized, rows))), to_tensor_normalize(torch.from_numpy(np.array(resized)))


def _loaders(pack, decode, split="test", perturb=True, **kw):
    from ssl4polyp_amd.packs import device_pack_loaders
    loaders, sampler = device_pack_loaders({split: pack[0]}, DEV, 4, decode=decode, num_workers=0, pin_memory=False,
                                           perturbation_splits=("test",) if perturb else (), **kw)
    return loaders[split], sampler


@pytest.mark.parametrize("decode,fused", [("host", False), ("device", False), ("device", True)])
def test_eval_loader_equals_pillow_then_the_oracle(pack, eval_images, decode, fused):
    (paths, labels, rows), _ = pack
    for perturb, want in ((True, eval_images[0]), (False, eval_images[1])):
        ld, sampler = _loaders(pack, decode, perturb=perturb, fused_decode=fused)
        assert sampler is None and len(ld) == 3
        got = [(x.clone(), y, r) for x, y, r in ld]
        assert [x.shape[0] for x, _, _ in got] == [4, 4, 2]
        assert all(x.is_cuda and x.dtype == torch.float32 and not y.is_cuda and y.dtype == torch.int64 for x, y, _ in got)
        assert torch.cat([y for _, y, _ in got]).tolist() == labels       # on the host, in CSV order
        assert [r for _, _, rs in got for r in rs] == rows
        x = torch.cat([x for x, _, _ in got]).cpu()
        assert torch.equal(x, want), (perturb, [int((x[b] != want[b]).sum()) for b in range(10)])
    # a val split named in no perturbation list is the plain transform
    ld, _ = _loaders(pack, decode, split="val", perturb=True, fused_decode=fused)
    assert torch.equal(torch.cat([x.clone() for x, _, _ in ld]).cpu(), eval_images[1])


@pytest.mark.parametrize("decode", ["host", "device"])
def test_train_loader_equals_the_oracle_in_sampler_order(pack, resized, decode):
    from oracle import augment_ref as R
    from oracle.input_ref import to_tensor_normalize
    from ssl4polyp_amd.data import draw_train_params
    (paths, labels, rows), _ = pack
    ld, sampler = _loaders(pack, decode, split="train", seed=6)
    assert isinstance(sampler, torch.utils.data.RandomSampler) and len(ld) == 2     # drop_last: 4 + 4 of 10
    g = torch.Generator().manual_seed(6)   # seed + rank: a copy of the prefetcher's generator
    got = [(x.clone(), y.clone(), r) for x, y, r in ld]
    seen = []
    for x, y, rs in got:
        idx = [rows.index(r) for r in rs]
        seen += idx
        assert y.is_cuda and y.cpu().tolist() == [labels[i] for i in idx]
        p = draw_train_params(len(idx), g)
        want = to_tensor_normalize(torch.from_numpy(R.train_augment(np.stack([resized[i] for i in idx]), p)))
        assert torch.equal(x.cpu(), want), idx
    assert len(set(seen)) == 8 and seen != sorted(seen)


def test_perturber_batches_decodes_a_jpeg_batch(pack, eval_images):
    """DevicePerturber.batches over a plain pack_loader of compressed files: the JpegBatch branch, its decoder kept across batches."""
    from ssl4polyp_amd.data import DevicePerturber
    from ssl4polyp_amd.packs import PackFrames, pack_loader
    (paths, labels, rows), _ = pack
    pt = DevicePerturber(DEV)
    assert pt._decoder is None
    ld = pack_loader(PackFrames(paths, labels, rows, decode="device"), 4, "test", num_workers=0, pin_memory=False)
    got = [(x.clone(), y, r) for x, y, r in pt.batches(ld)]
    dec = pt._decoder
    assert dec is not None and [x.shape[0] for x, _, _ in got] == [4, 4, 2]
    assert torch.equal(torch.cat([x for x, _, _ in got]).cpu(), eval_images[0])
    assert torch.cat([y for _, y, _ in got]).cpu().tolist() == labels and [r for _, _, rs in got for r in rs] == rows
    list(pt.batches(ld))
    assert pt._decoder is dec


def test_top_block_tables_are_built_before_the_forward_forks(monkeypatch):
    """The cls-row index tables of a new workspace (BlockStack.top_compact: filled by launches on the main stream) must be enqueued
    before the forward hands half of the batch to its second stream, whose gather reads them.  Seen from the host: the tables exist
    when the forward asks for that stream.  (Without this order the first training step of main_finetune read stale indices.)"""
    import ssl4polyp_amd as A
    torch.manual_seed(1)
    vm = A.get_MAE_backbone(None, True, 2, False, None, precision="bf16").to(DEV)
    rt = vm._rt
    rt.ensure(DEV)
    k = rt.k
    seen, made = [], []
    get_ws, aux_stream = rt.get_ws, k.aux_stream

    def spy_ws(*a, **kw):
        ws = get_ws(*a, **kw)
        made.append(ws)
        return ws

    def spy_aux(*a, **kw):
        seen.append(made[-1]._top_c is not None)
        return aux_stream(*a, **kw)
    monkeypatch.setattr(k, "SPLIT_FORWARD", 2)   # (the defaults, whatever the environment's A/B switches say)
    monkeypatch.setattr(k, "SPARSE_TOP", True)
    monkeypatch.setattr(rt, "get_ws", spy_ws)
    monkeypatch.setattr(k, "aux_stream", spy_aux)
    with torch.no_grad():
        logits = vm(torch.randn(8, 3, 224, 224, device=DEV))
    torch.cuda.synchronize()
    assert len(made) == 1 and made[0]._top_c is not None and seen and all(seen)
    assert torch.isfinite(logits).all()


def test_evaluate_cls_over_the_pack_loader(pack, eval_images):
    import ssl4polyp_amd as A
    from ssl4polyp_amd.train import evaluate_cls
    (paths, labels, rows), _ = pack
    torch.manual_seed(0)
    model = A.get_MAE_backbone(None, True, 2, False, None, precision="fp32").to(DEV)
    lab = torch.tensor(labels)
    plain = [(eval_images[0][i:i + 4].to(DEV), lab[i:i + 4]) for i in (0, 4, 8)]
    want_lg, want_tg = evaluate_cls(model, plain, DEV)
    ld, _ = _loaders(pack, "device")
    lg, tg = evaluate_cls(model, ld, DEV)
    assert lg.shape == (10, 2) and torch.equal(lg, want_lg) and torch.equal(tg, want_tg) and tg.tolist() == labels


def test_main_finetune_runs_the_same_training_from_every_decode_path(tmp_path):
    import csv
    from ssl4polyp_amd import main_finetune as M
    root = tmp_path / "data"
    (root / "img").mkdir(parents=True)
    with open(tmp_path / "train.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame_path", "label", "store_id", "variant"])
        for i in range(16):
            H, W = ((96, 128), (130, 70), (64, 64))[i % 3]
            (root / "img" / f"{i:02d}.jpg").write_bytes(encode(frame(H, W, 200 + i), subsampling=2, quality=90))
            w.writerow([f"img/{i:02d}.jpg", (i // 2) % 2, "frames", "clean"])
    runs = {}
    for name, extra in (("host", ["--decode", "host"]), ("device", ["--decode", "device"]),
                        ("fused", ["--decode", "device", "--fused_decode"])):
        out = tmp_path / name
        args = M.get_args_parser().parse_args(
            ["--train_csv", str(tmp_path / "train.csv"), "--val_csv", str(tmp_path / "train.csv"), "--root", f"frames={root}",
             "--batch_size", "8", "--epochs", "2", "--finetune_mode", "head+1", "--precision", "bf16", "--num_workers", "0",
             "--no_pin_mem", "--output_dir", str(out), "--seed", "3", "--log_every", "1"] + extra)
        model, val_logits = M.run(args)
        log = [json.loads(ln) for ln in open(out / "log.txt")]
        assert [r["epoch"] for r in log] == [0, 1] and all(k in log[0] for k in ("train_loss", "lr", "samples_per_sec", "val_loss"))
        assert all(np.isfinite(r["train_loss"]) and np.isfinite(r["val_loss"]) for r in log)
        assert (out / "ckpts" / "finetune_e2.pth").exists() and (out / "ckpts" / "last.pth").exists()
        assert val_logits.shape == (16, 2) and not val_logits.is_cuda
        runs[name] = ([r["train_loss"] for r in log], val_logits)
        del model
    for name in ("device", "fused"):
        assert runs[name][0] == runs["host"][0], (name, runs[name][0], runs["host"][0])
        assert torch.equal(runs[name][1], runs["host"][1]), name
