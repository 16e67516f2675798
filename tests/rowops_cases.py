"""The shapes and inputs of the row-kernel tests (not a test module): the smallest that reach each branch of pm_layernorm.hip's
forward, pm_misc.hip, pm_mae.hip and pm_head.hip, shared by tests/test_rowops_ref_cpu.py (f32 emulations against the bounds) and
the tests/test_gpu_*_edges.py files.  Inputs come from seeded CPU generators."""
import torch

REGIMES = ("random", "offset64", "const", "tiny", "huge")
PRECS = ("bf16", "fp16", "fp32")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def rows(M, D, regime, seed=1):
    """M rows of D in one of the input regimes of anything that normalises a row."""
    z = randn(M, D, seed=seed)
    if regime == "random":
        return 2.0 * z + 0.5          # the suite's
    if regime == "offset64":
        return z + 64.0               # |mean| >> std: one-pass variance and a lost mean digit show here
    if regime == "const":
        return torch.full((M, D), 3.25)   # var = 0: eps decides rstd
    if regime == "tiny":
        return 1e-4 * z               # var = 1e-8 << eps
    if regime == "huge":
        return 1e4 * z
    raise ValueError(regime)


def affine(D, seed=2):
    return 1 + 0.1 * randn(D, seed=seed), 0.1 * randn(D, seed=seed + 1)


# ---- pm_layernorm_fwd --------------------------------------------------------------------------
LN_D = (4,      # one live lane
        68,     # a ragged first slot (17 lanes)
        256,    # exactly one slot
        260,    # the first lane of slot 2
        768,    # three full slots of NV = 4: the fourth empty
        1024,   # NV = 4 full
        1028,   # NV = 5: the first lane of slot 5
        1280)   # NV = 5 full
LN_M = (1,      # three waves of the workgroup have no row
        3, 5,   # a ragged workgroup; a second workgroup with one row
        37)
LN_GRID = (16389, 32)   # 4 x 4096 rows per grid-stride trip: five rows make the second one
# (M, D, regime) run on the device in every precision: every D at M = 5 and every M at the two ragged D, random rows; every regime
# at D = 68 (ragged) and 768 (the model's)
LN_CASES = ([(5, D, "random") for D in LN_D] + [(M, D, "random") for M in LN_M if M != 5 for D in (260, 1028)] +
            [(37, D, r) for D in (68, 768) for r in REGIMES] + [(37, 1280, "offset64"), (3, 4, "const")])
LN_PITCH = ("D", "D+4", "5D")   # ldx = D; a column slice of a wider buffer; rows one sample of five tokens apart


def ln_pitch(D, pitch):
    return {"D": D, "D+4": D + 4, "5D": 5 * D}[pitch]


# ---- token path --------------------------------------------------------------------------------
IM2COL = ((32, 8, 3),     # vector path, PE = 192
          (28, 14, 3),    # p % 4 != 0: the element-wise path, 588 -> 640
          (24, 12, 3),    # vector path with row padding, 432 -> 448
          (16, 4, 1),     # one channel, 4 vectors
          (64, 32, 3),    # 768 vectors: the second and third trip of the v += blockDim.x loop
          (32, 16, 4))    # PE = 1024
IM2COL_KEEP = ("null", "one", "perm", "quarter")
ASSEMBLE = ((3, 5, 4), (3, 5, 68), (2, 7, 256), (2, 7, 260), (2, 3, 1280),   # (B, keep, D): one lane .. a second trip of the column loop
            (3, 1, 68),        # keep = 1
            (130, 127, 4))     # 16640 rows: past the 4096-workgroup cap
CLS_B = (1, 3, 4,     # the tail loop only (B < 13), with waves that have no sample
         13,          # wave 0 alone enters the unrolled body
         16,          # all four waves in it, no tail
         17, 29,      # body + tail in wave 0; a second trip for wave 0 only
         37, 64)      # a second trip and a tail; four trips, no tail
CLS_D = (4, 64, 68, 132)   # one block partly live; one full block; a ragged second / third 64-column block
GATHER_ROW_BYTES = (4, 8, 136, 1536)
SCATTER_ROW_BYTES = (16, 1536)
GATHER_GRID = (4099, 1024)        # R x row_bytes: 1049344 words > 4096 x 256
SCATTER_GRID = (8195, 4096)       # M x row_bytes (33.6 MB): 2097920 vectors > 8192 x 256


def cast_table():
    """Every f32 whose high half is any of the 65536 and whose low half is 0x0000 (exact in bf16), 0x7FFF (just below the bf16 tie),
    0x8000 (the tie: to even), 0x8001 (just above it) or 0xFFFF: 327680 values with bf16 ties, fp16 ties (low 13 bits 0x1000 come
    with the high halves), fp16 subnormals, fp16 overflow, infinities and NaNs."""
    hi = torch.arange(65536, dtype=torch.int64)
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)
    bits = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32)


def fp16_tie_table():
    """f32 values exactly half-way between two fp16 neighbours, normal and subnormal, and around the overflow threshold 65520."""
    h = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).double()   # every finite non-negative fp16
    mid = (h[:-1] + h[1:]) / 2
    edge = torch.tensor([65519.996, 65520.0, 65520.004, 65504.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -26, 0.0], dtype=torch.float64)
    v = torch.cat([mid, edge]).float()
    return torch.cat([v, -v])


# ---- MAE ---------------------------------------------------------------------------------------
MASK_L = (1, 4, 196, 256, 257, 784, 1024)   # 256 / 257: the last size with one element per thread, the first with two
NOISE = ("random", "equal", "two", "descending", "zeros")


def noise(B, L, regime, seed=7):
    if regime == "random":
        return torch.rand(B, L, generator=gen(seed))
    if regime == "equal":
        return torch.full((B, L), 0.5)                       # stable: the identity
    if regime == "two":
        return (torch.rand(B, L, generator=gen(seed)) < 0.5).float()   # mass ties
    if regime == "descending":
        return torch.arange(L, 0, -1, dtype=torch.float32).expand(B, L).contiguous() / L
    if regime == "zeros":                                    # 0.0 == -0.0: a tie, broken by position
        n = torch.rand(B, L, generator=gen(seed)) - 0.5
        n[:, ::3] = 0.0
        n[:, 1::3] = -0.0
        return n
    raise ValueError(regime)


def keeps(L):
    return sorted({0, 1, L // 4, L})


UNSHUFFLE = ((2, 9, 9, 4),      # (B, L, keep, D): keep = L, the mask token never used
             (2, 9, 1, 68), (3, 16, 4, 260), (2, 5, 2, 1280),
             (17, 1024, 256, 4))   # 17425 rows: past the 4096-workgroup cap
UNSHUFFLE_BWD_CAP = (70, 1024, 64, 4)   # 67200 masked positions > 65536: the 1024-row cap of the first stage
LOSS = ((8, 2, 1),      # (img, p, C): PE = 4, one live lane
        (16, 8, 3),     # PE = 192: a partial slot
        (28, 14, 3),    # PE = 588
        (32, 16, 3),    # PE = 768
        (32, 16, 4))    # PE = 1024: kLossVec full
LOSS_GRID = (129, 32, 2, 1)   # (B, img, p, C): 33024 patches > 4 x 8192


def loss_inputs(B, img, p, C, seed=11):
    """Images with a constant patch (patch 0 of sample 0: var = 0, inv = 1000) and an offset-64 patch (patch 1) among random ones, a
    prediction, and the three masks."""
    imgs = randn(B, C, img, img, seed=seed)
    imgs[0, :, :p, :p] = 3.25
    if img // p > 1:
        imgs[0, :, :p, p:2 * p] += 64.0
    L = (img // p) ** 2
    pred = randn(B, L, p * p * C, seed=seed + 1)
    masks = {"ones": torch.ones(B, L), "single": torch.zeros(B, L), "random": (torch.rand(B, L, generator=gen(seed + 2)) < 0.75).float()}
    masks["single"][B - 1, L - 1] = 1.0
    masks["random"][0, 0] = 1.0   # never all zero, and the constant patch counts
    return imgs, pred, masks


# ---- heads -------------------------------------------------------------------------------------
# (B, N, D, pool, n_class, bias, head, regime).  head_pgrad_kernel's loops by B: 1, 3 tail only; 5 wave 0 once through the unrolled
# body; 9 wave 0 body + tail; 13 two trips of wave 0; 16 every wave twice through the body.
HEAD = ((1, 1, 4, 0, 1, True, True, "random"),        # the smallest everything; N = 1: no non-cls row to zero
        (3, 5, 68, 0, 2, True, True, "random"),       # ragged slot; four zero rows
        (5, 5, 256, 0, 8, False, True, "offset64"),   # bias = NULL; exactly one slot
        (9, 1, 260, 0, 9, True, True, "random"),      # the compact cls rows; first lane of slot 2
        (13, 5, 1024, 0, 17, True, True, "random"),   # kHeadVec full (ViT-L)
        (16, 5, 68, 0, 2, True, False, "const"),      # head = False: d feat given; constant rows
        (3, 2, 68, 1, 2, True, True, "random"),       # pool: one patch row, three waves without a row
        (5, 3, 4, 1, 1, True, True, "offset64"),
        (9, 6, 260, 1, 9, True, True, "random"),      # n_class 9: the second pass over the stored features
        (13, 50, 256, 1, 8, False, True, "random"),   # 49 rows: 13 trips of wave 0, 12 of the others
        (16, 6, 1024, 1, 17, True, True, "const"),    # three passes over the classes
        (5, 3, 68, 1, 2, True, False, "random"))      # pooled features only


def head_inputs(B, N, D, n_class, regime, seed=21):
    x = rows(B * N, D, regime, seed=seed).reshape(B, N, D)
    gamma, beta = affine(D, seed=seed + 1)
    W, bias = 0.2 * randn(n_class, D, seed=seed + 3), 0.1 * randn(n_class, seed=seed + 4)
    dlogits, dfeat = randn(B, n_class, seed=seed + 5), randn(B, D, seed=seed + 6)
    return x, gamma, beta, W, bias, dlogits, dfeat
