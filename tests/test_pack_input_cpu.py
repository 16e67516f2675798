"""Host side of the pack input path (ssl4polyp_amd/packs.py, main_finetune's parser): the CSV reader against a fixture the
reference's own load_split + resolve_paths made (tests/golden/make_pack_paths_fixture.py), the dataset and its two collates
against Pillow / the packers they wrap, and the loader semantics of create_classification_dataloaders.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from pack_files import FALLBACK, make_files, pil_rgb, write_pack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_paths.json")


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_read_pack_csv_resolves_paths_as_the_reference_does(tmp_path):
    from ssl4polyp_amd.packs import read_pack_csv
    fx = json.load(open(GOLDEN))
    root = str(tmp_path)
    here = lambda s: s.replace("<ROOT>", root)
    csv_path = tmp_path / "split.csv"
    csv_path.write_text(fx["csv"])
    roots = {k: here(v) for k, v in fx["roots"].items()}
    want = [here(p) for p in fx["paths"]]
    assert len(want) == 12 and sum(p.startswith(root) for p in want) == 9   # all three cases of the rule are in the fixture
    for p in want:   # relative paths resolve against the working directory
        _touch(p if os.path.isabs(p) else os.path.join(root, p))
    cwd = os.getcwd()
    os.chdir(root)
    try:
        paths, labels, rows = read_pack_csv(csv_path, roots)
    finally:
        os.chdir(cwd)
    assert paths == want
    assert labels == fx["labels"] and all(isinstance(v, int) for v in labels)
    assert rows == fx["rows"] and all(type(r) is dict for r in rows)   # plain dicts of strings, exactly as read
    # without a map every path stays as written
    os.chdir(root)
    try:
        for rel in [r["frame_path"] for r in fx["rows"]]:
            _touch(os.path.join(root, rel))
        assert read_pack_csv(csv_path)[0] == [r["frame_path"] for r in fx["rows"]]
    finally:
        os.chdir(cwd)


def test_read_pack_csv_errors(tmp_path):
    from ssl4polyp_amd.packs import read_pack_csv
    p = tmp_path / "a.csv"
    p.write_text("frame_id,variant\nx,clean\n")
    with pytest.raises(ValueError, match=r"\['frame_path', 'label'\]"):
        read_pack_csv(p)
    p.write_text("frame_path,variant\nx,clean\n")
    with pytest.raises(ValueError, match=r"\['label'\]"):
        read_pack_csv(p)
    _touch(str(tmp_path / "x.jpg"))
    p.write_text(f"frame_path,label\n{tmp_path}/x.jpg,1\n{tmp_path}/x.jpg,\n")
    with pytest.raises(ValueError, match="[Ee]mpty label"):
        read_pack_csv(p)
    p.write_text(f"frame_path,label\n{tmp_path}/x.jpg,1\n{tmp_path}/missing.jpg,0\n")
    with pytest.raises(FileNotFoundError, match="missing.jpg"):
        read_pack_csv(p)


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    from ssl4polyp_amd.packs import read_pack_csv
    root = str(tmp_path_factory.mktemp("pack"))
    csv_path, roots, files, labels = write_pack(root)
    return read_pack_csv(csv_path, roots), files, labels


def test_pack_frames_and_collates(pack):
    from ssl4polyp_amd.data import RaggedFrames
    from ssl4polyp_amd.jpeg import JpegBatch
    from ssl4polyp_amd.packs import PackFrames, pack_jpeg_collate, pack_ragged_collate
    (paths, labels, rows), files, want_labels = pack
    assert labels == want_labels and all(os.path.isabs(p) for p in paths)
    host = PackFrames(paths, labels, rows)
    dev = PackFrames(paths, labels, rows, decode="device")
    assert len(host) == len(dev) == 10
    frame, label, row = host[3]
    assert np.array_equal(frame, np.asarray(pil_rgb(files[3]))) and label == 1 and row == rows[3]
    assert dev[9] == (files[9], 1, rows[9])
    x, lab, meta = pack_ragged_collate([host[i] for i in range(10)])
    want = RaggedFrames.from_frames([np.asarray(pil_rgb(f)) for f in files])
    assert isinstance(x, RaggedFrames) and torch.equal(x.data, want.data) and torch.equal(x.offset, want.offset) and torch.equal(x.hw, want.hw)
    assert lab.dtype == torch.int64 and lab.tolist() == want_labels and isinstance(meta, list) and meta == rows
    y, lab, meta = pack_jpeg_collate([dev[i] for i in range(10)])
    wantj = JpegBatch.from_bytes(files)
    assert isinstance(y, JpegBatch) and y.meta["fallback"] == FALLBACK and y.meta["n_subseq"] > 0
    assert set(y.t) == set(wantj.t) and all(torch.equal(y.t[k], wantj.t[k]) for k in wantj.t)
    assert lab.tolist() == want_labels and meta == rows
    # unlabelled: (frame, row) items, (batch, rows) batches -- and no mixing
    free = PackFrames(paths, None, rows)
    assert len(free[0]) == 2 and free[0][1] == rows[0]
    x2, meta2 = pack_ragged_collate([free[0], free[1]])
    assert len(x2) == 2 and meta2 == rows[:2]
    for collate, ds, un in ((pack_ragged_collate, host, free), (pack_jpeg_collate, dev, PackFrames(paths, None, rows, decode="device"))):
        with pytest.raises(ValueError, match="Mixed batch"):
            collate([ds[0], un[1]])
        with pytest.raises(ValueError):
            collate([un[0], ds[1]])
    with pytest.raises(ValueError, match="empty label"):
        PackFrames(paths, [1] * 9 + [""], rows)


def _order(loader):
    return [int(r["frame_id"][-6:-4]) for batch in loader for r in batch[-1]]


def test_pack_loader_semantics(pack):
    from ssl4polyp_amd.packs import PackFrames, pack_loader
    (paths, labels, rows), files, _ = pack
    ds = PackFrames(paths, labels, rows)
    kw = dict(num_workers=0, pin_memory=False)
    # train: shuffled, complete up to drop_last, a new order per epoch, the same run for the same seed
    a = pack_loader(ds, 4, "train", seed=3, **kw)
    assert len(a) == 2 and a.drop_last
    e0, e1 = _order(a), _order(a)
    assert len(e0) == 8 and len(set(e0)) == 8 and e0 != e1
    b = pack_loader(ds, 4, "train", seed=3, **kw)
    assert [_order(b), _order(b)] == [e0, e1]
    assert _order(pack_loader(ds, 4, "train", seed=4, **kw)) != e0
    assert len(pack_loader(ds, 4, "train", drop_last=False, **kw)) == 3
    # drop_last is switched off when the dataset, or a replica's share, is smaller than the batch
    small = pack_loader(ds, 16, "train", **kw)
    assert not small.drop_last and len(small) == 1 and sorted(_order(small)) == list(range(10))
    rep = pack_loader(ds, 4, "train", world=4, rank=1, seed=0, **kw)   # 10 // 4 = 2 < 4
    assert isinstance(rep.sampler, torch.utils.data.DistributedSampler) and not rep.drop_last and not rep.sampler.drop_last
    assert rep.sampler.shuffle and rep.sampler.seed == 0 and len(rep) == 1
    rep2 = pack_loader(ds, 4, "train", world=2, rank=0, seed=5, **kw)   # 10 // 2 = 5 >= 4: kept
    assert rep2.drop_last and rep2.sampler.drop_last and rep2.sampler.seed == 5 and len(rep2) == 1
    with pytest.raises(RuntimeError, match="zero batches"):
        pack_loader(PackFrames([], [], []), 4, "train", **kw)
    # val / test: sequential and complete
    for stage in ("val", "test"):
        v = pack_loader(ds, 4, stage, **kw)
        assert not v.drop_last and [len(b[0]) for b in v] == [4, 4, 2] and _order(v) == list(range(10))
        assert torch.cat([b[1] for b in v]).tolist() == labels
    with pytest.raises(ValueError):
        pack_loader(ds, 4, "eval", **kw)


def test_pack_loader_with_spawned_workers(pack):
    from ssl4polyp_amd.jpeg import JpegBatch
    from ssl4polyp_amd.packs import PackFrames, pack_loader
    (paths, labels, rows), files, _ = pack
    v = pack_loader(PackFrames(paths, labels, rows, decode="device"), 4, "val", num_workers=2, pin_memory=False)
    assert v.multiprocessing_context.get_start_method() == "spawn" and v.persistent_workers
    batches = list(v)
    assert [len(b[0]) for b in batches] == [4, 4, 2] and all(isinstance(b[0], JpegBatch) for b in batches)
    want = JpegBatch.from_bytes(files[4:8])
    assert all(torch.equal(batches[1][0].t[k], want.t[k]) for k in want.t)
    assert [r for b in batches for r in b[2]] == rows and torch.cat([b[1] for b in batches]).tolist() == labels
    del batches, v


def test_main_finetune_parser(capsys):
    from ssl4polyp_amd import main_finetune as M
    p = M.get_args_parser()
    flags = {s for a in p._actions for s in a.option_strings}
    for f in ("--train_csv", "--val_csv", "--test_csv", "--root", "--batch_size", "--epochs", "--lr", "--weight_decay", "--warmup_epochs",
              "--finetune_mode", "--mae_checkpoint", "--precision", "--decode", "--fused_decode", "--num_workers", "--perturb_test",
              "--output_dir", "--seed", "--log_every"):
        assert f in flags, f
    a = p.parse_args(["--train_csv", "t.csv", "--root", "sun=/data/sun", "--root", "pg=/data/pg", "--finetune_mode", "head+1"])
    assert a.decode == "host" and not a.fused_decode and not a.perturb_test and a.root == ["sun=/data/sun", "pg=/data/pg"]
    assert M.parse_roots(a.root) == {"sun": "/data/sun", "pg": "/data/pg"}
    with pytest.raises(SystemExit):
        p.parse_args(["--finetune_mode", "some"])
    with pytest.raises(SystemExit, match="no data"):   # before anything touches a device
        M.run(p.parse_args([]))
    with pytest.raises(SystemExit, match="KEY=PATH"):
        M.parse_roots(["nokey"])
    from ssl4polyp_amd import main_pretrain
    assert main_pretrain.get_args_parser().parse_args([]).fused_decode is False
    for mod in (main_pretrain, M):   # both refuse a fused decode that would silently run on the host
        with pytest.raises(SystemExit, match="--decode device"):
            mod.run(mod.get_args_parser().parse_args(["--fused_decode"] + (["--train_csv", "t.csv"] if mod is M else [])))
