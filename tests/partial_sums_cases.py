"""The cases behind tests/golden/partial_sums.npz: the kernels that sum rows through partial rows and one fixed-order reduce launch
(pm_colsum_ws, the mask-token gradient of pm_mae_unshuffle_bwd, the three sums of pm_layernorm_bwd), at the smallest shapes that
reach every branch of the code they share.  Inputs come from fixed seeds; `outputs` runs every case through engine.Kernels,
`freeze` turns the results into what the fixture stores.  tests/golden/make_partial_sums.py writes the fixture,
tests/test_gpu_partial_sums.py holds the kernels to it."""
import hashlib

import numpy as np
import torch

DEV = "cuda"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

# pm_colsum_ws (M, N).  (5, 4): one split, waves without a row.  (1031, 260): two 256-column strips, ragged rows.  (8197, 68):
# 128 splits -- the unrolled body of strided_sum<8> runs in every group -- and 4 live lanes in the second 64-column reduce block.
COLSUM_SHAPES = [(5, 4), (1031, 260), (8197, 68)]
# pm_mae_unshuffle_bwd (B, L, keep, D).  (50, 196, 49, 68): 115 partial rows -- the unrolled body runs in groups 0 to 2 (partial
# rows b + 112 < 115), groups 3 to 15 take only the scalar tail.
UNSHUFFLE_SHAPES = [(1, 4, 1, 4), (50, 196, 49, 68)]
# pm_layernorm_bwd (M, D).  (4099, 68): 1024 partial rows, the unrolled body of strided_sum<16> taken.
LAYERNORM_SHAPES = [(7, 768), (4099, 68)]
STORE_WHOLE_BYTES = 4096  # f32 outputs up to this size are stored whole, anything else as the sha256 of its bytes


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def colsum_input(M, N, dtype):
    return rnd(M, N, seed=100 + M).to(DTYPES[dtype])


def colsum_start(N, filled):
    return rnd(N, seed=7, scale=3.0) if filled else torch.zeros(N, device=DEV)


def unshuffle_input(B, L, keep, D):
    """dx f32 [B (L + 1), D] and ids_shuffle int32 [B, L], a permutation per sample."""
    g = torch.Generator().manual_seed(200 + B)
    ids = torch.argsort(torch.rand(B, L, generator=g), dim=1).to(torch.int32).to(DEV)
    return rnd(B * (L + 1), D, seed=201 + B), ids


def outputs(kernels):
    """kernels(precision) -> engine.Kernels.  -> {case name: device tensor}, every case run once."""
    out = {}
    k = kernels("bf16")
    for dtype in DTYPES:
        for M, N in COLSUM_SHAPES:
            x = colsum_input(M, N, dtype)
            for filled in (False, True):
                o = colsum_start(N, filled)
                k.colsum(x, o, M, N)
                out[f"colsum/{dtype}/{M}x{N}/{'filled' if filled else 'zero'}"] = o
    for prec in ("bf16", "fp32"):
        k = kernels(prec)
        for B, L, keep, D in UNSHUFFLE_SHAPES:
            dx, ids = unshuffle_input(B, L, keep, D)
            demb = torch.empty(B * (keep + 1), D, dtype=k.act_dtype, device=DEV)
            dmask = torch.zeros(D, device=DEV)
            k.mae_unshuffle_bwd(dx, ids, demb, dmask, B, L, keep, D)
            tag = f"unshuffle/{prec}/{B}x{L}x{keep}x{D}"
            out[tag + "/dmask_token"], out[tag + "/demb"] = dmask, demb
        for M, D in LAYERNORM_SHAPES:
            x = rnd(M, D, seed=1, scale=2.0) + 0.5
            gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
            y = torch.empty(M, D, dtype=k.act_dtype, device=DEV)
            mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
            k.layernorm_fwd(x, gamma, beta, y, mean, rstd, M, D)
            dy, dres = rnd(M, D, seed=4).to(k.act_dtype), rnd(M, D, seed=5)
            dx = torch.empty(M, D, device=DEV)
            dx_act = torch.empty(M, D, dtype=k.act_dtype, device=DEV)
            sums = [torch.zeros(D, device=DEV) for _ in range(3)]
            k.layernorm_bwd(dy, x, gamma, mean, rstd, dres, dx, dx_act, *sums, M, D)
            tag = f"layernorm/{prec}/{M}x{D}"
            for name, t in zip(("dgamma", "dbeta", "dcolsum", "dx", "dx_act"), (*sums, dx, dx_act)):
                out[f"{tag}/{name}"] = t
    torch.cuda.synchronize()
    return out


def freeze(out):
    """-> {name: f32 array} for the small f32 outputs, {name + '.sha256': 32 bytes} for the rest."""
    frozen = {}
    for name, t in out.items():
        t = t.detach().contiguous().cpu()
        if t.dtype == torch.float32 and t.numel() * 4 <= STORE_WHOLE_BYTES:
            frozen[name] = t.numpy()
        else:
            raw = t.view(-1).view(torch.uint8).numpy().tobytes()
            frozen[name + ".sha256"] = np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8)
    return frozen
