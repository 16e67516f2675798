"""The GEMM cases of tests/test_gpu_gemm_edges.py and tests/test_gemm_ref_cpu.py (not a test module): the smallest shapes that reach
every kernel family, ring configuration, layout pair, operand / output type, epilogue, store width, split and tile order the
dispatcher can name.  tests/test_host_cpu.py::test_gemm_case_table_reaches_every_plan holds each case to the plan it claims
(pm_gemm_plan) and the table to completeness.

A case: family, forced pm_gemm_opts.variant (0 = heuristics), layout as tests/test_gpu_ops.py names it (first letter t: A k-major
[K][M]; second letter n: B k-major [K][N] -- "nt" forward, "nn" dgrad, "tn" weight gradient, "tt" A k-major alone), operand type, C
type, epilogue, M, N, K, padding of lda / ldb / ldc in elements, bias given, workspace bytes (0 none, -1 sixteen slabs = every split
fits), pm_gemm_opts.max_blocks, and the claimed plan: k-slices, ring cfg, tile, band.

Ring (M >= 1024, K % 64 == 0, 16-bit): M = 1031 is a ragged last tile of 7 rows at 256 and of 71 rows at 192.  K = 64, 128, 192, 320
are 2, 4, 6 and 10 ring stages of 32 elements (a forward / dgrad K is a multiple of 64, so the stage count is always even: the odd
counts of the k-loops' prologue / tail branches are reached by the weight gradients, 2112 / 32 = 66 and 16448 / 32 = 514 stages cut
into slices of 17, 15, 33 and 19).  N = 264: the 8-wide 16-byte stores of a 16-bit C, last tile 8 columns wide; N = 260: the 4-wide
fallback through N & 7, last tile 4 columns wide (k-normal W only: a k-major W needs N % 8 == 0); N = 264 with ldc = 268: the
4-wide fallback through ldc & 7; N = 1800: 8 tile columns = a band of 6 and one of 2."""
from collections import namedtuple

from test_gpu_ops import RING_PAIRS  # the mirror of kRingCfgs: {cfg: [(W layout, epilogue)]}; key 1 = the 128 x 128 kernels

Case = namedtuple("Case", "family variant layout in_dt c_dt epi M N K pa pb pc bias ws max_blocks split cfg tile band")
DTYPES = ("bf16", "fp16", "fp32")
EPILOGUES = ("store", "gelu", "resid", "dgelu", "accum")
LAYOUTS = ("nt", "nn", "tn", "tt")
RING_TILE_M = {8: 256, 9: 256, 10: 192, 24: 256, 25: 256, 26: 192}
WGRAD_TILE = {1: (256, 128), 2: (256, 256)}  # pm_gemm_opts.variant bits 6-7


def a_kmajor(c):
    return c.layout[0] == "t"


def b_kmajor(c):
    return c.layout[1] == "n"


def c_dtypes(in_dt, epi):
    """The C types the plan accepts for this operand type and epilogue."""
    if epi in ("resid", "accum"):
        return ("fp32",)
    return ("fp32", in_dt) if in_dt != "fp32" else ("fp32", "bf16", "fp16")


def store_width(c):
    """Columns per store of a ring epilogue into a 16-bit C (the condition of both epilogue styles in pm_gemm.hip); None elsewhere."""
    if c.family != "ring" or c.c_dt == "fp32":
        return None
    return 8 if c.N % 8 == 0 and (c.N + c.pc) % 8 == 0 else 4


def ws_bytes(c):
    return 16 * c.M * c.N * 4 if c.ws < 0 else c.ws


def case_id(c):
    pad = "".join(f"+{n}{v}" for n, v in (("a", c.pa), ("b", c.pb), ("c", c.pc)) if v)
    return (f"{c.family}{c.variant or ''}-{c.layout}-{c.in_dt}>{c.c_dt}-{c.epi}-{c.M}x{c.N}x{c.K}{pad}"
            f"{'-ws' + str(c.ws) if c.ws else ''}{'-mb' + str(c.max_blocks) if c.max_blocks else ''}")


def _ring():
    out = []
    for cfg, pairs in RING_PAIRS.items():
        if cfg == 1:
            continue
        for pi, (layout, epi) in enumerate(pairs):
            for dt in ("bf16", "fp16"):
                c_dt = dt if epi in ("store", "gelu", "dgelu") else "fp32"
                bias = layout == "nt" and epi in ("store", "gelu", "resid")

                def add(N, K, pa=0, pb=0, pc=0):
                    out.append(Case("ring", cfg, layout, dt, c_dt, epi, 1031, N, K, pa, pb, pc, bias, 0, 0, 1, cfg,
                                    (RING_TILE_M[cfg], 256), 6 if N > 6 * 256 else 0))
                add(264, 64)
                add(260 if layout == "nt" else 264, 128)
                add(264, 192, pc=4)
                add(264, 320, pa=8 if pi == 0 else 0, pb=8 if pi == len(pairs) - 1 else 0)
                add(1800, 64)
    return out


def _small(family):
    """The two 128 x 128 kernels: (129, 132) = ragged tiles in both directions, (34, 4) = N - 4 == 0 (a k-major operand needs its
    row count to be a chunk multiple: 136 / 40 and, for a 16-bit k-major B, 136 / 8); K = 1, 2, 3 k-steps (LDS-DMA kernel: 128
    bytes of k per step) or K = 8 mod 64 (16-bit) / 4 mod 32 (f32) for the generic kernel, K = 8 / 4 being less than one step."""
    out = []
    for layout in LAYOUTS:
        akm, bkm = layout[0] == "t", layout[1] == "n"
        for dt in DTYPES:
            ke, epc = (64, 8) if dt != "fp32" else (32, 4)
            idx = 0
            for epi in EPILOGUES:
                for c_dt in c_dtypes(dt, epi):
                    big = idx % 2 == 0
                    M = (129 if big else 34) if not akm else ((136 if big else 40) if epc == 8 else (132 if big else 36))
                    N = (132 if big else 4) if not (bkm and epc == 8) else (136 if big else 8)
                    steps = 1 + idx % 3
                    K = steps * ke if family == "lds128" else (steps - 1) * ke + epc
                    pa, pb, pc = (epc if idx % 4 == 1 else 0), (epc if idx % 4 == 2 else 0), (4 if idx % 4 == 3 else 0)
                    out.append(Case(family, 0, layout, dt, c_dt, epi, M, N, K, pa, pb, pc, epi in ("store", "gelu", "resid"), 0, 0,
                                    1, 0, (128, 128), 0))
                    idx += 1
    return out


def _splitk():
    """Split-K of the LDS-DMA kernel (both operands k-major, no bias, f32 C, ldc == N, a workspace): 17 k-steps in slices of 9 + 8,
    41 k-steps in slices of 9, 9, 9, 9, 5, and a workspace of 64 bytes, too small for any slab: the plan falls back to one slice."""
    out = []
    for dt in DTYPES:
        ke = 64 if dt != "fp32" else 32
        for epi in ("store", "accum"):
            for K, ws, split in ((17 * ke, -1, 2), (41 * ke, -1, 5), (41 * ke, 64, 1)):
                out.append(Case("lds128", 0, "tn", dt, "fp32", epi, 136, 136, K, 0, 0, 0, False, ws, 0, split, 0, (128, 128), 0))
    return out


def _wgrad():
    """Ring weight gradients (both operands k-major, K >= 2048, M >= 256, N >= 128, a workspace, no bias, f32 C): (264, 136) and
    (520, 264) are ragged by 8 in both directions at either tile; both tiles forced through variant bits 6-7 and chosen by the
    heuristic (fewer than four 256 x 256 tiles: 256 x 128).  66 k-stages: max_blocks = 16 over 9 tiles = one slice; over 6 tiles =
    two even slices of 33; over 2 or 4 tiles = 4 slices of 17, 17, 17, 15; a workspace of two slabs lowers 4 slices to 2; 514
    k-stages on 2 tiles and the whole chip: the cap of 16 slices, 15 of 33 and one of 19."""
    out = []
    for dt in ("bf16", "fp16"):
        for epi in ("store", "accum"):
            def add(M, N, K, wv, mb, ws, split, tile):
                out.append(Case("wgrad", wv << 6, "tn", dt, "fp32", epi, M, N, K, 0, 0, 0, False, ws, mb, split, 0, tile, 0))
            add(264, 136, 2112, 1, 16, -1, 4, (256, 128))
            add(264, 136, 2112, 2, 16, -1, 4, (256, 256))
            add(264, 136, 2112, 0, 16, -1, 4, (256, 128))
            add(264, 136, 2112, 1, 16, 2 * 264 * 136 * 4, 2, (256, 128))
            add(520, 264, 2112, 1, 16, -1, 1, (256, 128))
            add(520, 264, 2112, 2, 16, -1, 2, (256, 256))
            add(520, 264, 2112, 0, 0, -1, 4, (256, 256))
            add(264, 136, 16448, 2, 0, -1, 16, (256, 256))
    return out


CASES = _ring() + _small("lds128") + _small("generic") + _splitk() + _wgrad()

# pm_wgrad_group: (K, [(n_out, n_in)]) of the last two rows of test_gpu_ops.test_wgrad_group -- the MAE decoder block at a long K (48
# tiles x 4 ragged k-slices) and two problems with ragged tiles in both dimensions -- in both 16-bit types, with and without the
# bias gradients
GROUP_CASES = [(K, dims, dt, db) for K, dims in ((16384 + 32, ((512, 2048), (2048, 512), (512, 512), (1536, 512))),
                                                 (2080, ((264, 136), (520, 648))))
               for dt in ("bf16", "fp16") for db in (True, False)]
