"""CPU-side checks of the product's host logic (no GPU compute): the C-ABI library loads and exports every
symbol include/polypmae.h declares, the drop-in modules reproduce the reference's state-dict surface and
seeded initialisation, the flat parameter storage aliases correctly, and the product refuses to run
without the HIP path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "polypmae.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    return g.LIB


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built)
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/polypmae.h but not exported"
    from ssl4polyp_amd import _lib
    assert set(_lib.SIGNATURES) | {"pm_strerror", "pm_abi_version", "pm_gemm_workspace_bytes", "pm_workspace_bytes",
                                   "pm_wgrad_group_workspace_bytes", "pm_aug_resized_crop_workspace_bytes"} == set(names)
    handle = _lib.load()
    assert handle.pm_abi_version() == _lib.ABI_VERSION == 16
    # nothing undeclared leaves the library: every exported pm_* symbol is in the header (diagnostic hooks included)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("pm_")}
    assert exported == set(names), exported ^ set(names)
    # workspace queries answer without a GPU: the split-K slabs of the ViT-B fc1 weight gradient on half of the CUs
    opts = _lib.GemmOpts(128, 0)
    assert handle.pm_gemm_workspace_bytes(1, 1, _lib.PM_BF16, 3072, 768, 12608, ctypes.byref(opts)) == 3 * 3072 * 768 * 4
    assert handle.pm_gemm_workspace_bytes(0, 0, _lib.PM_BF16, 12608, 768, 768, None) == 0
    assert handle.pm_workspace_bytes(_lib.WS_LAYERNORM_BWD, 12608, 768) == 1024 * 3 * 768 * 4
    assert handle.pm_strerror(-2).decode() == "unsupported shape"
    # grouped weight gradients: a ViT-B block (108 tiles) needs no slabs, the MAE decoder block at K = 50 432 tokens is cut
    # into 4 k-slices (f32 partials + the partial row sums of the two bias gradients); a short K is not sliced
    def group(dims, biased):
        arr = (_lib.WgradItem * len(dims))()
        for j, (o, i) in enumerate(dims):
            arr[j] = _lib.WgradItem(64, o, 64, i, 64, i, o, i, 0, 64 if j in biased else None)  # (addresses are only checked)
        return arr
    enc = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    dec = [(512, 2048), (2048, 512), (512, 512), (1536, 512)]
    assert handle.pm_wgrad_group_workspace_bytes(group(enc, ()), 4, 12608, _lib.PM_BF16) == 0
    assert handle.pm_wgrad_group_workspace_bytes(group(dec, (1, 3)), 4, 50432, _lib.PM_BF16) == \
        4 * 4 * sum(o * i for o, i in dec) + 4 * 4 * (2048 + 1536)
    assert handle.pm_wgrad_group_workspace_bytes(group(dec, ()), 4, 2112, _lib.PM_BF16) == 0


def _gemm_plan(handle, a_kmajor, b_kmajor, in_dtype, has_bias, c_dtype, epilogue, M, N, K, max_blocks=0, variant=0, ws_bytes=0,
               ldc_is_n=1):
    """pm_gemm_plan -> (status, (family, cfg, tile_m, tile_n, split_k, band, ws_bytes))."""
    from ssl4polyp_amd import _lib
    opts, info = _lib.GemmOpts(max_blocks, variant), _lib.GemmPlanInfo()
    st = handle.pm_gemm_plan(a_kmajor, b_kmajor, in_dtype, has_bias, c_dtype, ldc_is_n, epilogue, M, N, K, ws_bytes, ctypes.byref(opts),
                             ctypes.byref(info))
    return st, (info.family, info.cfg, info.tile_m, info.tile_n, info.split_k, info.band, info.ws_bytes)


def test_gemm_dispatch_table(built):
    """Which kernel every GEMM of the shipped workloads runs on (pm_gemm_plan), against tests/golden/gemm_plan.json: the table the
    dispatcher gave when its rules were gathered into plan_gemm, before the unreachable variants were deleted.  Rows: the four
    forward GEMMs, the four dgrads and the four split-K weight gradients (max_blocks = 128, unlimited scratch) of ViT-B/16
    fine-tuning at bs = 64 (bf16 and f32), MAE ViT-B at bs = 256 and bs = 64 (encoder and 512-wide decoder), ViT-L/16 and ViT-H/14."""
    import json
    from ssl4polyp_amd import _lib
    handle = _lib.load()
    BF16, F32 = _lib.PM_BF16, _lib.PM_F32
    rows = json.load(open(os.path.join(REPO, "tests", "golden", "gemm_plan.json")))
    assert len(rows) == 136
    by_name = {}
    for r in rows:
        ws = (1 << 62) if r["unlimited_ws"] else 0
        st, plan = _gemm_plan(handle, r["a_kmajor"], r["b_kmajor"], r["in_dtype"], r["has_bias"], r["c_dtype"], r["epilogue"],
                              r["M"], r["N"], r["K"], r["max_blocks"], 0, ws)
        want = tuple(r["plan"][f] for f in ("family", "cfg", "tile_m", "tile_n", "split_k", "band", "ws_bytes"))
        assert st == 0 and plan == want, (r["name"], st, plan, want)
        by_name[r["name"]] = plan
        if r["unlimited_ws"]:  # the workspace query is the same plan
            opts = _lib.GemmOpts(r["max_blocks"], 0)
            assert handle.pm_gemm_workspace_bytes(1, 1, r["in_dtype"], r["M"], r["N"], r["K"], ctypes.byref(opts)) == plan[6], r["name"]
        else:
            assert handle.pm_gemm_workspace_bytes(r["a_kmajor"], r["b_kmajor"], r["in_dtype"], r["M"], r["N"], r["K"], None) == plan[6] == 0
    # rows derived by hand from the rules: (family, cfg, tile_m, tile_n), band where stated
    RING, LDS128 = _lib.GEMM_RING, _lib.GEMM_LDS128
    for name, want in {
            "vitb_cls_bs64.qkv.M6304": (RING, 8, 256, 256, 1, 6), "vitb_cls_bs64.proj.M6304": (RING, 26, 192, 256),
            "vitb_cls_bs64.fc2.M6304": (RING, 26, 192, 256), "vitb_cls_bs64.fc1_gelu.M6304": (RING, 8, 256, 256),
            "vitb_cls_bs64.dfc2_dgelu.M12608": (RING, 8, 256, 256, 1, 6), "vitb_cls_bs64.dfc1.M12608": (RING, 24, 256, 256),
            "vitb_cls_bs64.dproj.M12608": (RING, 24, 256, 256), "vitb_cls_bs64.dqkv.M12608": (RING, 24, 256, 256),
            "mae_vitb_bs64_enc.qkv.M3200": (LDS128, 0, 128, 128), "mae_vitb_bs64_enc.fc1_gelu.M3200": (RING, 8, 256, 256),
            "mae_vitb_bs64_dec.qkv.M12608": (RING, 10, 192, 256), "mae_vitb_bs64_dec.proj.M12608": (LDS128, 0, 128, 128),
            "mae_vitb_bs256_dec.proj.M50432": (RING, 24, 256, 256), "mae_vitb_bs256_dec.fc2.M50432": (RING, 24, 256, 256)}.items():
        assert by_name[name][:len(want)] == want, (name, by_name[name])
    # the shapes of test_gemm_large_tile_paths (tests/test_gpu_ops.py): at M = 4000 the few-tiles rule sends N = 768 to the
    # 128 x 128 kernel, N = 2304 stays on ring cfg 8
    E = _lib
    assert _gemm_plan(handle, 0, 0, BF16, 1, F32, E.EPI_RESIDUAL, 4000, 768, 3072)[1][:2] == (LDS128, 0)
    assert _gemm_plan(handle, 0, 0, BF16, 1, BF16, E.EPI_STORE, 4000, 2304, 768)[1][:4] == (RING, 8, 256, 256)
    assert _gemm_plan(handle, 0, 0, BF16, 1, BF16, E.EPI_GELU, 4000, 1536, 512)[1][:2] == (LDS128, 0)
    assert _gemm_plan(handle, 0, 1, BF16, 0, BF16, E.EPI_STORE, 4000, 768, 2304)[1][:2] == (LDS128, 0)
    assert _gemm_plan(handle, 0, 1, BF16, 0, BF16, E.EPI_DGELU, 4000, 3072, 768)[1][:2] == (RING, 8)
    # ... and its k-major-A shapes cover both weight-gradient tiles
    WG = _lib.GEMM_RING_WGRAD
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_STORE, 520, 136, 4096, 128, 0, 1 << 62)[1][:4] == (WG, 0, 256, 128)
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_STORE, 2304, 768, 4032, 128, 0, 1 << 62)[1][:4] == (WG, 0, 256, 256)
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_ACCUM, 768, 3072, 8192, 128, 0, 1 << 62)[1][:4] == (WG, 0, 256, 256)
    # the override names shipped kernels only: every (cfg, W layout) pair of the table is accepted and obeyed ...
    shipped = {(8, 0), (8, 1), (9, 0), (10, 0), (24, 0), (24, 1), (25, 0), (26, 0)}
    for cfg in range(2, 64):
        for wk in (0, 1):
            st, plan = _gemm_plan(handle, 0, wk, BF16, 0, BF16, E.EPI_STORE, 1031, 264, 64, 0, cfg)
            if (cfg, wk) in shipped:
                assert st == 0 and plan[:4] == (RING, cfg, 192 if cfg in (10, 26) else 256, 256), (cfg, wk, st, plan)
            else:  # ... removed values (6, 12, 13, 40, ...) and unshipped pairs (cfg 9 with k-major W) are refused
                assert st == _lib.PM_EINVAL, (cfg, wk, st)
    assert _gemm_plan(handle, 0, 0, BF16, 0, BF16, E.EPI_STORE, 1031, 264, 64, 0, 1)[1][:2] == (LDS128, 0)
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_STORE, 2304, 768, 4032, 128, 1 << 6, 1 << 62)[1][:4] == (WG, 0, 256, 128)
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_STORE, 520, 136, 4096, 128, 2 << 6, 1 << 62)[1][:4] == (WG, 0, 256, 256)
    assert _gemm_plan(handle, 1, 1, BF16, 0, F32, E.EPI_STORE, 2304, 768, 4032, 128, 3 << 6, 1 << 62)[0] == _lib.PM_EINVAL
    assert _gemm_plan(handle, 0, 0, BF16, 0, BF16, E.EPI_STORE, 1031, 264, 64, 0, 256)[0] == _lib.PM_EINVAL
    # refusals that need no pointer keep their status
    assert _gemm_plan(handle, 0, 0, BF16, 0, BF16, E.EPI_STORE, 0, 264, 64)[0] == _lib.PM_ESHAPE
    assert _gemm_plan(handle, 0, 0, BF16, 0, BF16, E.EPI_STORE, 128, 264, 36)[0] == _lib.PM_EALIGN
    assert _gemm_plan(handle, 0, 0, BF16, 0, BF16, E.EPI_RESIDUAL, 128, 264, 64)[0] == _lib.PM_EINVAL  # f32 residual stream only


def test_gemm_case_table_reaches_every_plan(built):
    """tests/gemm_cases.py (what tests/test_gpu_gemm_edges.py runs and tests/test_gemm_ref_cpu.py emulates) against pm_gemm_plan: each
    case plans to the family / cfg / tile / k-slices / band it claims, and the table reaches every combination the plan can name --
    every family with every operand type and layout pair the launcher dispatches for it, every ring configuration with each W layout
    it is built for (found by asking the plan for every variant value, so a new cfg without cases fails here), both weight-gradient
    tiles, one slice / ragged slices / the cap of 16, band 0 and band 6, the 8-wide and the 4-wide stores of a 16-bit C by both
    triggers, and each epilogue on each family that accepts it."""
    import gemm_cases as G
    from ssl4polyp_amd import _lib
    handle = _lib.load()
    DT = {"bf16": _lib.PM_BF16, "fp16": _lib.PM_F16, "fp32": _lib.PM_F32}
    EPI = {"store": _lib.EPI_STORE, "gelu": _lib.EPI_GELU, "resid": _lib.EPI_RESIDUAL, "dgelu": _lib.EPI_DGELU, "accum": _lib.EPI_ACCUM}
    FAM = {_lib.GEMM_GENERIC: "generic", _lib.GEMM_LDS128: "lds128", _lib.GEMM_RING: "ring", _lib.GEMM_RING_WGRAD: "wgrad"}
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)
    for c in G.CASES:
        st, plan = _gemm_plan(handle, int(G.a_kmajor(c)), int(G.b_kmajor(c)), DT[c.in_dt], int(c.bias), DT[c.c_dt], EPI[c.epi], c.M,
                              c.N, c.K, c.max_blocks, c.variant, G.ws_bytes(c), int(c.pc == 0))
        assert st == 0, (G.case_id(c), st)
        assert (FAM[plan[0]], plan[1], (plan[2], plan[3]), plan[4], plan[5]) == (c.family, c.cfg, c.tile, c.split, c.band), \
            (G.case_id(c), plan)
        if c.split > 1:
            assert plan[6] == c.split * c.M * c.N * 4 <= G.ws_bytes(c), (G.case_id(c), plan)

    def reached(family, *fields):
        return {tuple(getattr(c, f) if isinstance(f, str) else f(c) for f in fields) for c in G.CASES if c.family == family}
    # the two 128 x 128 kernels: PM_DISPATCH_ACT x with_layouts, and every epilogue with every C type the plan accepts for it
    small = {(lay, dt, epi, c_dt) for lay in G.LAYOUTS for dt in G.DTYPES for epi in G.EPILOGUES for c_dt in G.c_dtypes(dt, epi)}
    for fam in ("generic", "lds128"):
        assert reached(fam, "layout", "in_dt", "epi", "c_dt") >= small, (fam, small - reached(fam, "layout", "in_dt", "epi", "c_dt"))
        for lay in G.LAYOUTS:   # per layout and operand type: 1, 2 and 3 k-steps, the ragged pair of tiles and the 4-column problem
            for dt in G.DTYPES:
                sel = [c for c in G.CASES if (c.family, c.layout, c.in_dt, c.split, c.ws) == (fam, lay, dt, 1, 0)]
                ke = 64 if dt != "fp32" else 32
                assert {-(-c.K // ke) for c in sel} == {1, 2, 3} and {c.M > 128 and c.N > 128 for c in sel} == {True, False}
                assert any(c.pa for c in sel) and any(c.pb for c in sel) and any(c.pc for c in sel)
    assert min(c.K for c in G.CASES if c.family == "generic" and c.in_dt != "fp32") == 8      # less than one k-step
    assert any(c.N == 4 for c in G.CASES if c.family == "lds128") and any(c.N == 4 for c in G.CASES if c.family == "generic")
    # split-K behind the LDS-DMA kernel: ragged slices and the fall-back to one slice, STORE and ACCUM, every operand type
    for dt in G.DTYPES:
        for epi in ("store", "accum"):
            sel = [c for c in G.CASES if (c.family, c.in_dt, c.epi) == ("lds128", dt, epi) and c.ws]
            nk = lambda c: c.K // (64 if dt != "fp32" else 32)
            assert {c.split for c in sel if nk(c) % -(-nk(c) // c.split)} == {2, 5}          # the last slice is shorter
            assert any(c.split == 1 and 0 < c.ws < 2 * c.M * c.N * 4 for c in sel)           # no slab fits: one slice
    # ring: what the plan accepts as a forced variant is what RING_PAIRS mirrors, with the W layouts it is built for
    from test_gpu_ops import RING_PAIRS
    nameable = set()
    for cfg in range(2, 64):
        for wk in (0, 1):
            if _gemm_plan(handle, 0, wk, _lib.PM_BF16, 0, _lib.PM_BF16, _lib.EPI_STORE, 1031, 264, 64, 0, cfg)[0] == 0:
                nameable.add((cfg, "nn" if wk else "nt"))
    assert {cfg for cfg, _ in nameable} == set(RING_PAIRS) - {1}
    assert nameable == {(cfg, lay) for cfg, pairs in RING_PAIRS.items() if cfg != 1 for lay, _ in pairs}
    assert reached("ring", "cfg", "layout", "in_dt") == {(cfg, lay, dt) for cfg, lay in nameable for dt in ("bf16", "fp16")}
    assert reached("ring", "cfg", "layout", "epi") == {(cfg, lay, epi) for cfg, ps in RING_PAIRS.items() if cfg != 1 for lay, epi in ps}
    for cfg, pairs in RING_PAIRS.items():
        if cfg == 1:
            continue
        sel = [c for c in G.CASES if c.family == "ring" and c.cfg == cfg]
        assert {c.K for c in sel} == {64, 128, 192, 320} and {c.band for c in sel} == {0, 6}
        assert any(c.pa == 8 for c in sel) and any(c.pb for c in sel)
        for lay, epi in pairs:
            if epi not in ("store", "gelu", "dgelu"):
                continue
            for dt in ("bf16", "fp16"):   # a 16-bit C: 16-byte stores, and the 4-wide fallback by N & 7 and by ldc & 7
                widths = {(G.store_width(c), c.N % 8 != 0, c.pc % 8 != 0) for c in sel if (c.layout, c.epi, c.in_dt) == (lay, epi, dt)}
                want = {(8, False, False), (4, False, True)} | ({(4, True, False)} if lay == "nt" else set())  # (k-major W: N % 8 == 0)
                assert widths >= want, (cfg, lay, epi, dt, widths)
    # ring weight gradients: both tiles, forced and chosen; one slice, even slices, ragged slices, a lowered split, the cap
    for dt in ("bf16", "fp16"):
        for epi in ("store", "accum"):
            sel = [c for c in G.CASES if (c.family, c.in_dt, c.epi) == ("wgrad", dt, epi)]
            assert {(c.variant >> 6, c.tile) for c in sel} >= {(1, (256, 128)), (2, (256, 256)), (0, (256, 128)), (0, (256, 256))}
            for tile in ((256, 128), (256, 256)):
                assert {c.split for c in sel if c.tile == tile} >= {4} and {c.M for c in sel if c.tile == tile} == {264, 520}
            assert {c.split for c in sel} == {1, 2, 4, 16}
            assert any(c.split == 2 and 0 < c.ws < 4 * c.M * c.N * 4 for c in sel)                     # lowered by the workspace
            assert any(c.split > 1 and (c.K // 32) % -(-(c.K // 32) // c.split) for c in sel)          # a ragged last slice
            assert any(c.split == 16 and (c.K // 32) // 16 > 16 for c in sel)                          # the cap, not the k-step rule
    assert set(FAM.values()) == {c.family for c in G.CASES}


def _attention_plan(handle, backward, B, N, H, dh, dtype):
    """pm_attention_plan -> (status, (family, nt, ct, grid, launches, lds bytes of launch 0, of launch 1))."""
    from ssl4polyp_amd import _lib
    info = _lib.AttentionPlanInfo()
    st = handle.pm_attention_plan(backward, B, N, H, dh, dtype, ctypes.byref(info))
    return st, (info.family, info.nt, info.ct, info.grid, info.launches, info.lds_bytes[0], info.lds_bytes[1])


def test_attention_dispatch_table(built):
    """What pm_attention_fwd / pm_attention_bwd launch for a shape (pm_attention_plan), against tests/golden/attention_plan.json:
    the table the dispatcher gave when its rules were gathered into plan_attention, before the kernels and switches it cannot
    name were deleted.  Rows: (B, H) = (64, 12) at 20 sequence lengths x dh 32 / 64 / 80 x bf16 / fp16 / fp32, forward and
    backward; the persistent forward's grid at B H = 6 .. 3072; the refusals."""
    import json
    from ssl4polyp_amd import _lib
    handle = _lib.load()
    BF16, F16, F32 = _lib.PM_BF16, _lib.PM_F16, _lib.PM_F32
    HEAD, PERSISTENT, SPLIT, FUSED = _lib.ATTN_FWD_HEAD, _lib.ATTN_FWD_PERSISTENT, _lib.ATTN_BWD_SPLIT, _lib.ATTN_BWD_FUSED
    rows = json.load(open(os.path.join(REPO, "tests", "golden", "attention_plan.json")))
    assert len(rows) == 360 + 6 + 8
    for r in rows:
        st, plan = _attention_plan(handle, r["backward"], r["B"], r["N"], r["H"], r["dh"], r["dtype"])
        assert st == r["status"], (r, st)
        if st == 0:
            want = tuple(r["plan"][f] for f in ("family", "nt", "ct", "grid", "launches")) + tuple(r["plan"]["lds_bytes"])
            assert plan == want, (r, plan)
    assert {(r["B"] * r["H"]) for r in rows[360:366]} == {6, 256, 257, 259, 768, 3072}
    assert [r["status"] for r in rows[366:]] == [_lib.PM_ESHAPE, _lib.PM_ESHAPE, _lib.PM_EINVAL, _lib.PM_ESHAPE] * 2
    # rows derived by hand from the rules
    plan = lambda *a: _attention_plan(handle, *a)
    for half in (BF16, F16):
        # forward, dh 64, N 193..224: persistent, [K0 | V0 | K1 | V1 | Q] of 7 x 32 rows of 128 B; rounds = ceil(BH / 256),
        # grid = ceil(BH / rounds)
        for (B, H), grid in (((64, 12), 256), ((257, 1), 129), ((37, 7), 130), ((1, 6), 6)):
            for N in (193, 197, 224):
                assert plan(0, B, N, H, 64, half) == (0, (PERSISTENT, 7, 7, grid, 1, 143360, 0)), (B, H, N)
        assert 5 * 7 * 32 * 64 * 2 == 143360
        assert plan(0, 64, 192, 12, 64, half)[1][0] == plan(0, 64, 225, 12, 64, half)[1][0] == HEAD
        assert plan(0, 64, 197, 12, 32, half) == (0, (HEAD, 7, 7, 768, 1, 28672, 0))
        assert plan(0, 64, 100, 12, 64, half)[1][:2] == (HEAD, 7)  # the seven-tile instantiation serves 65 <= N <= 192 too
        assert plan(1, 64, 197, 12, 64, half) == (0, (FUSED, 7, 7, 768, 1, 116480, 0))
        assert plan(1, 64, 257, 12, 64, half) == (0, (FUSED, 9, 9, 768, 1, 149760, 0))
        assert plan(1, 64, 65, 12, 80, half) == (0, (SPLIT, 3, 3, 768, 2, 49152, 49920))
    assert plan(0, 64, 257, 12, 80, F32) == (0, (HEAD, 9, 3, 768, 1, 73728, 0))
    assert plan(1, 64, 197, 12, 64, F32) == (0, (SPLIT, 7, 7, 768, 2, 114688, 116480))
    for dt in (BF16, F16, F32):
        assert plan(0, 64, 65, 12, 80, dt)[1][:2] == (HEAD, 3)
        for bwd in (0, 1):  # the instantiated tile counts
            for dh, ladder in ((32, (1, 2, 7, 9)), (64, (1, 2, 7, 9)), (80, (3, 9))):
                got = {N: plan(bwd, 64, N, 12, dh, dt)[1][1] for N in range(1, 289)}
                assert sorted(set(got.values())) == list(ladder)
                assert all(32 * nt >= N for N, nt in got.items())
                if dh != 80:
                    assert (got[32], got[33], got[64], got[65], got[224], got[225]) == (1, 2, 2, 7, 7, 9)
                else:
                    assert (got[96], got[97]) == (3, 9)


def test_attention_case_table_reaches_every_instantiation(built):
    """tests/attention_cases.py (what tests/test_gpu_attention_edges.py runs, in every precision, forward and backward) against
    pm_attention_plan: every (family, dh, tile count, 16-bit / f32) the plan can name for some N = 1..288 is the plan of some case;
    the persistent forward walks 1, 2 and 3 heads per workgroup; the chunked configuration (ct < nt) is reached, with a whole
    chunk of padding."""
    from attention_cases import CASES
    from ssl4polyp_amd import _lib
    handle = _lib.load()
    dtypes = {"bf16": _lib.PM_BF16, "fp16": _lib.PM_F16, "fp32": _lib.PM_F32}

    def plans(B, N, H, dh):
        for prec, dt in dtypes.items():
            for bwd in (0, 1):
                st, plan = _attention_plan(handle, bwd, B, N, H, dh, dt)
                assert st == 0, (bwd, B, N, H, dh, prec)
                yield prec, plan

    key = lambda prec, plan, dh: (plan[0], dh, plan[1], prec != "fp32")
    nameable = {key(prec, plan, dh) for dh in (32, 64, 80) for N in range(1, 289) for prec, plan in plans(64, N, 12, dh)}
    assert len(nameable) == 2 * (2 * (4 + 4 + 2)) + 1   # forward + backward, 16-bit + f32, the ladders; the persistent forward
    reached, walks, chunked = set(), set(), set()
    for B, N, H, dh in CASES:
        for prec, plan in plans(B, N, H, dh):
            reached.add(key(prec, plan, dh))
            if plan[0] == _lib.ATTN_FWD_PERSISTENT:
                walks.add(-(-B * H // plan[3]))
            if plan[2] < plan[1]:
                chunked.add((plan[0], N, -(-N // (32 * plan[2]))))   # (family, N, chunks that hold a real row)
    assert reached == nameable, sorted(nameable - reached)
    assert walks == {1, 2, 3}
    # f32, dh 80, nine tiles in chunks of three: N = 97 has one real row in the second chunk and a whole chunk of padding behind
    # it, N = 193 one real row in the third chunk and two whole tiles of padding
    for fam in (_lib.ATTN_FWD_HEAD, _lib.ATTN_BWD_SPLIT):
        assert {c for f, _, c in chunked if f == fam} == {2, 3}, chunked
        assert (fam, 97, 2) in chunked and (fam, 193, 3) in chunked


def test_no_cpu_fallback():
    import ssl4polyp_amd as A
    from ssl4polyp_amd._lib import PolypMaeError
    m = A.MaskedAutoencoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, decoder_embed_dim=32,
                               decoder_depth=1, decoder_num_heads=1)
    with pytest.raises(PolypMaeError):
        m(torch.zeros(1, 3, 32, 32))


def test_custom_ops_are_registered_without_a_cpu_kernel():
    """The HIP kernels are exposed as torch custom ops (torch.ops.polypmae.*, ssl4polyp_amd/ops.py); nothing is registered
    for the CPU backend, so a CPU tensor fails in the dispatcher -- no eager fallback can be reached through the ops."""
    from ssl4polyp_amd import ops
    for n in ops.OP_NAMES:
        assert hasattr(torch.ops.polypmae, n), n
    with pytest.raises(NotImplementedError):
        torch.ops.polypmae.attention(torch.zeros(1, 4, 96), 2)
    with pytest.raises(NotImplementedError):
        torch.ops.polypmae.layernorm(torch.zeros(2, 8), torch.ones(8), torch.zeros(8))


def test_product_does_not_import_oracle():
    for root, _, files in os.walk(os.path.join(REPO, "ssl4polyp_amd")):
        for fn in files:
            if fn.endswith(".py"):
                src = open(os.path.join(root, fn)).read()
                assert "oracle" not in src, f"{fn} mentions the oracle"


def test_seeded_init_matches_reference(golden):
    """Same torch seed => same initial weights as the reference constructor (models_mae.py:65-93)."""
    import ssl4polyp_amd as A
    from oracle import vit_mae_ref as O
    fx = golden("tiny_mae.npz")
    cfg = O.VIT_TINY
    torch.manual_seed(11)
    m = A.MaskedAutoencoderViT(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim, depth=cfg.depth,
                               num_heads=cfg.num_heads, decoder_embed_dim=cfg.decoder_embed_dim,
                               decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads, mlp_ratio=4)
    checked = 0
    for n, p in m.named_parameters():
        if p.ndim >= 2 and n not in ("cls_token", "mask_token"):
            np.testing.assert_array_equal(p.detach().numpy(), fx["w/" + n], err_msg=n)
            checked += 1
    assert checked > 10


def test_state_dict_surface(golden):
    import ssl4polyp_amd as A
    fx = golden("tiny_cls.npz")
    vm = A.ViT_from_MAE(None, True, 2, False, None, embed_dim=64, depth=2, num_heads=2, out_token="cls")
    assert set(vm.state_dict()) == {k[len("mae/w/"):] for k in fx if k.startswith("mae/w/")}
    assert vm.head is True and hasattr(vm, "lin_head") and hasattr(vm, "blocks") and vm.frozen is False
    va = A.VisionTransformer_from_Any(True, 2, False, None, 64, 2, 2, "cls", False)
    assert set(va.state_dict()) == {k[len("any/w/"):] for k in fx if k.startswith("any/w/")}
    assert isinstance(va.head, torch.nn.Identity) and va.pos_embed.requires_grad
    mae = A.mae_vit_base_patch16()
    n_params = sum(p.numel() for p in mae.parameters())
    assert n_params == 111907840  # tests/golden/meta.json: reference mae_vit_base_patch16
    assert not mae.pos_embed.requires_grad and not mae.decoder_pos_embed.requires_grad
    # finetune.py:49-91 contract: head module discovery + block tail
    assert isinstance(vm.blocks, torch.nn.ModuleList) and len(list(vm.lin_head.parameters())) == 2


def test_flat_storage_aliasing_cpu():
    import ssl4polyp_amd as A
    from ssl4polyp_amd.flat import FlatParams
    m = A.ViT_from_MAE(None, True, 2, False, None, embed_dim=64, depth=2, num_heads=2, out_token="cls")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    f = FlatParams(m, torch.bfloat16)
    assert not f.bound(torch.device("cpu"))
    f.materialize(torch.device("cpu"))
    assert f.bound(torch.device("cpu"))
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n])
        assert p.data_ptr() == f.param_view(n).data_ptr()
        assert not f.grad_is_flat(n)
    with torch.no_grad():
        m.lin_head.weight.add_(1.0)
    assert torch.equal(f.param_view("lin_head.weight"), before["lin_head.weight"] + 1.0)
    assert f.shadow_stale()
    f.mark_shadow_fresh()
    assert not f.shadow_stale()
    m.lin_head.weight.grad = f.grad_view("lin_head.weight")
    assert f.grad_is_flat("lin_head.weight")
    # vec / mat split: 1-D params, tokens and positional tables live in `vec`
    regions = dict(zip(f.names, f.region))
    assert regions["cls_token"] == "vec" and regions["pos_embed"] == "vec" and regions["blocks.0.norm1.weight"] == "vec"
    assert regions["blocks.0.attn.qkv.weight"] == "mat" and regions["patch_embed.proj.weight"] == "mat"
    # moving the module invalidates the binding
    m.to(torch.float64)
    assert not f.bound(torch.device("cpu"))


def test_philox_restatement_against_random123_known_answers():
    """oracle/noise_ref.py (the CPU restatement pm_mae_noise is checked against on the GPU) on the known-answer vectors of the
    Random123 distribution (kat_vectors: philox4x32 10 rounds)."""
    from oracle.noise_ref import mae_noise, philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(ctr, key)
        assert tuple(int(x) for x in got) == want
    x = mae_noise(1000, 1234, 7)
    assert x.dtype.name == "float32" and x.min() >= 0.0 and x.max() < 1.0 and abs(x.mean() - 0.5) < 0.05
    assert not (mae_noise(1000, 1234, 8) == x).all() and (mae_noise(997, 1234, 7) == x[:997]).all()


def test_module_patchify_helpers_match_the_reference_fixture(golden):
    """MaskedAutoencoderViT.patchify / unpatchify (models_mae.py:95-121; pure data movement, off the hot path, CPU-capable) against
    the reference-generated index-ramp fixture that pins the pixel order."""
    import numpy as np
    import torch
    import ssl4polyp_amd as A
    fx = golden("tables.npz")
    m = A.MaskedAutoencoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                               decoder_num_heads=1)
    ramp = torch.arange(2 * 3 * 32 * 32, dtype=torch.float32).reshape(2, 3, 32, 32)
    np.testing.assert_array_equal(m.patchify(ramp).numpy(), fx["patchify_ramp"])
    np.testing.assert_array_equal(m.unpatchify(torch.from_numpy(fx["patchify_ramp"])).numpy(), fx["unpatchify_ramp"])


def test_stack_workspace_declares_its_state():
    """What BlockStack keeps on a workspace between calls exists from construction on, as instance attributes (bench.py reads
    `_bwd_descs` through the instance dictionary); building one needs neither the library nor a GPU."""
    from ssl4polyp_amd.engine import StackGeom, StackWorkspace
    ws = StackWorkspace(StackGeom(64, 2, 2, 256), 2, 5, torch.float32, torch.device("cpu"), True)
    assert ws._fwd_descs == {} and ws._bwd_descs == {} and ws._top_c is None and ws._deferred_join == [] and ws.cls_top is False
    assert {"_fwd_descs", "_bwd_descs", "_top_c", "_deferred_join", "cls_top"} <= set(vars(ws))


def test_scratch_arena_grows_per_key_and_never_shrinks():
    """engine.ScratchArena, as Kernels keys it by stream: distinct keys get distinct buffers, a smaller request returns the same
    buffer, a larger one a larger buffer and a new generation, nothing shrinks, and no buffer is below 64 KiB."""
    from ssl4polyp_amd.engine import ScratchArena
    a, cpu = ScratchArena(), torch.device("cpu")
    assert a.generation == 0
    b1, b2 = a.get(1, 100, cpu), a.get(2, 100, cpu)
    assert b1.data_ptr() != b2.data_ptr() and b1.dtype == torch.uint8
    assert b1.numel() == b2.numel() == 1 << 16 == ScratchArena.FLOOR and a.generation == 2
    assert a.get(1, 0, cpu) is b1 and a.get(1, 1 << 16, cpu) is b1 and a.get(2, 7, cpu) is b2 and a.generation == 2
    big = a.get(1, (1 << 16) + 1, cpu)
    assert big is not b1 and big.numel() >= (1 << 16) + 1 and a.generation == 3
    assert a.get(1, 5, cpu) is big and a.get(1, 1 << 16, cpu) is big and a.generation == 3   # nothing ever shrinks
    assert a.get(2, 100, cpu) is b2                                                          # and key 2 was left alone
    sizes = []
    for n in (10, 1 << 20, 3, 1 << 18, (1 << 20) + 8):
        sizes.append(a.get(3, n, cpu).numel())
    assert sizes == sorted(sizes) and sizes[0] == 1 << 16 and sizes[-1] >= (1 << 20) + 8 and a.generation == 6
