"""Writes tests/golden/attention_plan.json: what pm_attention_plan answers for the shapes test_attention_dispatch_table reads
(tests/test_host_cpu.py).  Needs the built library, no GPU.   usage: python tests/golden/make_attention_plan.py"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ssl4polyp_amd import _lib  # noqa: E402

NS = (1, 3, 17, 32, 33, 50, 64, 65, 70, 96, 97, 100, 130, 192, 193, 197, 224, 225, 257, 288)
DTYPES = (("bf16", _lib.PM_BF16), ("fp16", _lib.PM_F16), ("fp32", _lib.PM_F32))


def row(lib, backward, B, N, H, dh, dtype):
    info = _lib.AttentionPlanInfo()
    st = lib.pm_attention_plan(backward, B, N, H, dh, dtype, ctypes.byref(info))
    plan = None if st else {"family": info.family, "nt": info.nt, "ct": info.ct, "grid": info.grid, "launches": info.launches,
                            "lds_bytes": list(info.lds_bytes)}
    return {"backward": backward, "B": B, "N": N, "H": H, "dh": dh, "dtype": dtype, "status": st, "plan": plan}


def main():
    lib = _lib.load()
    rows = [row(lib, bwd, 64, N, 12, dh, dt) for bwd in (0, 1) for _, dt in DTYPES for dh in (32, 64, 80) for N in NS]
    rows += [row(lib, 0, B, 197, H, 64, _lib.PM_BF16) for B, H in ((1, 6), (64, 4), (257, 1), (37, 7), (64, 12), (256, 12))]  # B H = 6 .. 3072
    rows += [row(lib, bwd, B, N, 12, dh, dt) for bwd in (0, 1)
             for B, N, dh, dt in ((64, 289, 64, _lib.PM_BF16), (64, 197, 48, _lib.PM_BF16), (64, 197, 64, 7), (0, 197, 64, _lib.PM_BF16))]
    with open(os.path.join(HERE, "attention_plan.json"), "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
