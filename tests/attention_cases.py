"""The attention shapes the edge tests run (not a test module): the smallest (B, N, H, dh) at which each code path of
pm_attention.hip can go wrong.  tests/test_gpu_attention_edges.py runs every one in every precision; tests/test_host_cpu.py asks
pm_attention_plan what each launches and asserts that the table reaches every instantiation the plan can name.

N by tile ladder (a bar separates tile counts): the last tile full (32, 64, 96, 224, 256, 288), one key in it (33, 65, 97, 193,
225, 257), and a whole tile -- or, for the f32 80-wide heads staged in chunks of three tiles, a whole chunk -- of padding behind it."""
import torch

from attention_ref import DTYPES

CASES = [
    # dh 64: 1 | 2 | 7 tiles, head kernel | 7 tiles, persistent forward | 9 tiles
    (3, 1, 2, 64), (2, 31, 3, 64), (2, 32, 2, 64),
    (2, 33, 2, 64), (2, 64, 3, 64),
    (2, 65, 2, 64), (2, 96, 2, 64), (2, 97, 3, 64), (2, 192, 2, 64),
    (2, 193, 3, 64), (3, 197, 2, 64), (2, 224, 2, 64),
    (2, 225, 2, 64), (2, 256, 3, 64), (2, 257, 2, 64), (2, 288, 2, 64),
    # dh 32: H odd -> identity map; (2, 65, 8, 32): H even and B H % 16 == 0 -> the pair map of problem_of_block
    (2, 17, 3, 32), (2, 32, 2, 32),
    (2, 33, 2, 32), (2, 64, 3, 32),
    (2, 65, 8, 32), (3, 130, 2, 32), (2, 224, 2, 32),
    (2, 225, 3, 32), (2, 256, 2, 32), (2, 288, 2, 32),
    # dh 80: 3 | 9 tiles; f32 at 9 tiles is staged in chunks of 3: N = 97 has one key in the second chunk and a whole chunk of padding
    # behind it, N = 193 one key in the third chunk
    (2, 3, 2, 80), (2, 33, 3, 80), (2, 64, 2, 80), (2, 65, 2, 80), (2, 96, 2, 80),
    (2, 97, 3, 80), (2, 193, 2, 80), (2, 225, 2, 80), (2, 257, 2, 80), (2, 288, 2, 80),
    # persistent forward: the cases above walk one head per workgroup; B H = 259 two (buffer 0, then 1); B H = 513 three at grid
    # 171 (the third head lands in buffer 0 again while the second computes)
    (37, 197, 7, 64), (57, 197, 9, 64),
]
PRECS = ("bf16", "fp16", "fp32")

SPIKE = (1, 197, 2, 64)    # regime shapes
IDENTICAL_KEYS = (2, 197, 2, 64)


def case_id(case):
    return "x".join(str(v) for v in case)


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def inputs(case, prec, regime="random"):
    """(qkv [B, N, 3 H dh], dout [B, N, H dh]) on the CPU, rounded to the activation type of `prec`.
    random:         qkv = 1.5 randn, dout = randn (as test_attention_fwd_bwd)
    spike:          Q and K x 6 -- one dominant key per query
    identical_keys: every key of a head the same row -- a uniform softmax, every score tied for the maximum."""
    B, N, H, dh = case
    D = H * dh
    dt = DTYPES[prec]
    if regime == "random":
        qkv = _randn((B, N, 3 * D), 40, 1.5)
    elif regime == "spike":
        qkv = _randn((B, N, 3 * D), 42)
        qkv[:, :, :2 * D] *= 6.0
    elif regime == "identical_keys":
        qkv = _randn((B, N, 3 * D), 45, 1.5)
        qkv[:, :, D:2 * D] = qkv[:, :1, D:2 * D]
    else:
        raise ValueError(regime)
    return qkv.to(dt), _randn((B, N, D), 41).to(dt)
