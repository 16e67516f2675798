"""Generator of tests/golden/pack_paths.json -- the path rule of a pack split, as the REFERENCE applies it.

Writes a 12-row split CSV into a temporary directory, reads it with the reference's own ssl4polyp.configs.manifests.load_split and
resolves it with its resolve_paths (configs/manifests.py:302-347) against a roots map whose roots live under a placeholder
directory.  The rows cover the three cases of the rule: the first path component is a key of the map; it is not, and the row's
`store_id` (then its `dataset`) is; nothing maps and the path stays as written.  Only data is stored: the CSV text, the roots map
relative to the placeholder root, and the resolved paths relative to it (tests/test_pack_input_cpu.py replays them through
ssl4polyp_amd.packs.read_pack_csv).

    SSL4POLYP_REFERENCE=<reference checkout> python tests/golden/make_pack_paths_fixture.py
"""
import csv
import json
import os
import sys
import tempfile
from pathlib import Path

OUT = Path(__file__).with_name("pack_paths.json")
PLACEHOLDER = "<ROOT>"
COLUMNS = ("dataset", "frame_path", "label", "store_id", "variant")
ROOTS = {"sun": "stores/sun_frames", "polypgen_store": "stores/polypgen", "KVASIR": "stores/by_dataset/kvasir"}
ROWS = (
    # 1: the first component is a key of the map -> replaced
    ("SUN", "sun/case1/a.jpg", 1, "sun", "clean"),
    ("SUN", "sun/case1/b.jpg", 0, "", "clean"),
    ("OTHER", "sun/deep/er/c.jpg", 1, "polypgen_store", "blur_1p5"),   # (the first component wins over store_id)
    ("SUN", "sun/d.jpg", 0, "unknown", "clean"),
    # 2a: not a key; store_id is -> prefixed
    ("PolypGen", "images/e.jpg", 1, "polypgen_store", "clean"),
    ("KVASIR", "seq/1/f.jpg", 0, "polypgen_store", "jpeg_q40"),        # (store_id before dataset)
    ("X", "g.jpg", 1, "sun", "clean"),
    # 2b: neither the component nor store_id; dataset is -> prefixed
    ("KVASIR", "images/h.jpg", 0, "", "clean"),
    ("KVASIR", "i.jpg", 1, "nowhere", "occ_a0p2"),
    # 3: nothing maps -> as written
    ("X", "plain/j.jpg", 0, "", "clean"),
    ("", "k.jpg", 1, "nowhere", "clean"),
    ("Y", "plain/deep/l.jpg", 0, "nowhere", "bc_b1p3_c0p7"),
)


def main():
    ref = os.environ.get("SSL4POLYP_REFERENCE")
    if not ref:
        raise SystemExit("set SSL4POLYP_REFERENCE to the reference checkout")
    sys.path.insert(0, str(Path(ref) / "src"))
    from ssl4polyp.configs import manifests as M
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        csv_path = root / "split.csv"
        with open(csv_path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(COLUMNS)
            w.writerows(ROWS)
        roots_map = {k: str(root / v) for k, v in ROOTS.items()}
        rows = M.load_split(csv_path)
        paths = M.resolve_paths(rows, roots_map, sample=0)   # (existence is not part of the rule)
        rel = []
        for p in paths:
            p = Path(p)
            rel.append(PLACEHOLDER + "/" + p.relative_to(root).as_posix() if p.is_absolute() else p.as_posix())
        record = {"csv": csv_path.read_text(), "roots": {k: PLACEHOLDER + "/" + v for k, v in ROOTS.items()}, "paths": rel,
                  "labels": [int(r["label"]) for r in rows], "rows": [dict(r) for r in rows]}
    OUT.write_text(json.dumps(record, indent=1) + "\n")
    print(f"wrote {OUT} ({len(rel)} rows)")


if __name__ == "__main__":
    main()
