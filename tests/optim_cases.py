"""The shapes, regimes and hyper-parameter sets of the optimizer-kernel tests (not a test module), shared by
tests/test_optim_ref_cpu.py (f32 emulations against the bounds of tests/optim_ref.py) and tests/test_gpu_optim_edges.py.  Inputs come
from seeded CPU generators."""
import math

import torch

from rowops_cases import gen, randn

f32 = torch.float32

# ---- AdamW ---------------------------------------------------------------------------------------
ADAMW_SIZES = (4,                  # one vector
               1020, 1024, 1028,   # one vector per lane of a workgroup, -1 and +1
               4096,               # exactly one chunk of kAdamwChunk = 4 x 256 vectors: the whole-chunk branch of a bounded grid
               4100)               # one chunk and a ragged vector
ADAMW_CAP = 4194304 + 4100         # past the 4096-workgroup cap of the unbounded grid: a second grid-stride trip (suite regime only)
ADAMW_MULTI_STEP = (1028, 4100)    # three consecutive steps
SEGMENT_BOUND = 3                  # max_blocks of the pm_adamw_segments runs
REGIMES = ("suite", "tiny", "huge", "zero_g", "cold")
STEPS = (1, 2, 1000, 100000)
# name: (lr, beta1, beta2, eps, weight decay, grad_scale = hyper[5], 1 / loss scale = hyper[10])
HYPERS = {
    "b95_wd": (1e-3, 0.9, 0.95, 1e-8, 0.05, 1.0, 0.0),
    "b999_wd0": (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0),
    "b999_wd": (1e-2, 0.9, 0.999, 1e-8, 0.05, 1.0, 0.0),
    "lr0": (0.0, 0.9, 0.95, 1e-8, 0.05, 1.0, 0.0),
    "half": (1e-2, 0.9, 0.95, 1e-8, 0.05, 0.5, 0.0),
    "half_inv1": (1e-3, 0.9, 0.999, 1e-8, 0.05, 0.5, 1.0),
    "half_inv1024": (1e-2, 0.9, 0.95, 1e-8, 0.05, 0.5, 1.0 / 1024),
    "half_inv2m40": (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5, 2.0 ** -40),
}
N_CPU = 20000   # elements per case of the CPU emulation


def hyper_gscale(name):
    h = HYPERS[name]
    return h[5] * (h[6] if h[6] != 0.0 else 1.0)   # powers of two: exact


def adamw_cases():
    """(regime, hyper name, step) of every element-wise case; `cold` (m = v = 0) is a first step."""
    return [(r, h, s) for r in REGIMES for h in HYPERS for s in STEPS if r != "cold" or s == 1]


def _loguniform(n, lo, hi, seed):
    e = torch.rand(n, generator=gen(seed), dtype=torch.float64) * (math.log10(hi) - math.log10(lo)) + math.log10(lo)
    sign = torch.where(torch.rand(n, generator=gen(seed + 1)) < 0.5, -1.0, 1.0).double()
    return sign * 10.0 ** e


def adamw_inputs(n, regime, gscale=1.0, seed=0):
    """p, g, m, v (f32, CPU).  The regime describes gr = g gscale, what the moments see; gscale is a power of two, so g = gr / gscale
    is exact.
      suite    gr ~ 1e-3, m ~ gr, v ~ gr^2, p ~ 0.05: the model tests'
      tiny     |gr| in 1e-12 .. 1e-8 (log-uniform), states alike: sqrt(v) <= eps, eps decides the step; >= 1e-15, nothing subnormal
      huge     gr ~ 1e15: gr^2 ~ 1e30 is within a few hundred of f32's largest
      zero_g   g = 0: only the decay of p, m and v
      cold     m = v = 0 (step 1)"""
    s = 100 * seed
    p = (randn(n, seed=s + 1) * 0.05).to(f32)
    if regime in ("suite", "zero_g", "cold"):
        gr, m = randn(n, seed=s + 2) * 1e-3, randn(n, seed=s + 3) * 1e-3
        v = (randn(n, seed=s + 4) * 1e-3).square()
    elif regime == "tiny":
        gr, m = _loguniform(n, 1e-12, 1e-8, s + 2), _loguniform(n, 1e-12, 1e-8, s + 4)
        v = _loguniform(n, 1e-12, 1e-8, s + 6).square()
    elif regime == "huge":
        gr, m = randn(n, seed=s + 2) * 1e15, randn(n, seed=s + 3) * 1e15
        v = (randn(n, seed=s + 4) * 1e15).square()
    else:
        raise ValueError(regime)
    gr, m, v = gr.to(f32), m.to(f32), v.to(f32)
    if regime == "zero_g":
        gr = torch.zeros(n, dtype=f32)
    if regime == "cold":
        m, v = torch.zeros(n, dtype=f32), torch.zeros(n, dtype=f32)
    g = gr / torch.tensor(gscale, dtype=f32)
    assert torch.equal(g * torch.tensor(gscale, dtype=f32), gr) and bool(torch.isfinite(g).all())
    return p, g, m, v


NONFINITE_AT = (0, 5, 1023, 4092, 4096, 4099)   # of n = 4100: the first vector, inside the chunk, its last vector, the ragged vector


# ---- ticks ---------------------------------------------------------------------------------------
TICK_N = (1, 64, 65, 200)     # one thread; one full 64-thread grid; the first thread of a second workgroup; four workgroups
TICK_STEPS = (0, 1, 9, 999, 65535, 16777215)
TICK_SATURATED = 16777216     # stays
TICK_BETAS = ((0.9, 0.95), (0.9, 0.999))


def tick_records(n, seed=0):
    """[n, 16] f32 records: presets cycle through TICK_STEPS + the saturated counter and both beta pairs, every third record (from the
    second) carries the skip flag, and every other slot holds a random value that nothing may touch."""
    h = randn(n, 16, seed=40 + seed).to(f32)
    steps = TICK_STEPS + (TICK_SATURATED,)
    for i in range(n):
        b1, b2 = TICK_BETAS[(i // len(steps)) % 2]
        h[i, 1], h[i, 2] = b1, b2
        h[i, 6] = float(steps[i % len(steps)])
        h[i, 9] = 1.0 if i % 3 == 1 else 0.0
    return h


def tick_list(n_records, n_list, seed=0):
    """n_list strictly ascending record indices."""
    return torch.randperm(n_records, generator=gen(50 + seed))[:n_list].sort().values.to(torch.int32)


# ---- loss scale ----------------------------------------------------------------------------------
LS_GROUPS = (1, 64, 65, 130)   # one thread; the 64 threads once; a second trip of the loop for thread 0; a third
LS_STATS = {"none": (3.5, 0.0, 0.0), "nan": (float("nan"), 3.0, 0.0), "inf": (float("inf"), 0.0, 2.0), "both": (float("nan"), 1.0, 7.0)}
LS_TRACKER = {"interval-2": (4, 2.0), "interval-1": (4, 3.0), "interval=1": (1, 0.0)}   # (growth interval, tracker before)
LS_FACTORS = {"2_half": (2.0, 0.5), "backoff1": (2.0, 1.0), "growth1": (1.0, 0.5)}       # (growth, backoff)
LS_SCALES = {"65536": 65536.0, "overflows": 3e38}   # 3e38 x 2 > f32's largest: the grown scale is inf


def loss_scale_cells():
    """Every cell of the table: (id, state [6], stats [3], growth, backoff, interval)."""
    cells = []
    for sn, stats in LS_STATS.items():
        for tn, (interval, tracker) in LS_TRACKER.items():
            for fn, (growth, backoff) in LS_FACTORS.items():
                for cn, scale in LS_SCALES.items():
                    state = [scale, tracker, 0.0, 5.0, 41.0, 0.25]
                    cells.append(("-".join((sn, tn, fn, cn)), state, list(stats), growth, backoff, interval))
    return cells


# ---- grad stats ----------------------------------------------------------------------------------
STATS_SIZES = (1, 2, 3,            # no vector: the tail only
               4, 5, 4099,         # one vector; with a tail element; 1024 vectors + 3
               100003,             # 98 workgroups
               1048576 + 1024 + 3)  # 262400 vectors: past the 1024-workgroup cap, a second trip for the first 256 threads
STATS_PRIOR = (0.75, 2.0, 1.0)     # what `out` holds before an accumulating call


def stats_input(n, seed=0):
    return randn(n, seed=60 + seed).to(f32)


def stats_plants(n):
    """{name: index} of the places a non-finite value is planted: the first vector, the last vector, the tail."""
    nvec, at = n >> 2, {}
    if nvec:
        at["first_vector"] = 1
        at["last_vector"] = 4 * nvec - 2
    if n & 3:
        at["tail"] = n - 1
    return at


# ---- dgelu / scale -------------------------------------------------------------------------------
DGELU_SIZES = (4, 1028, 4194304 + 4)   # one vector; 257 vectors; past the 4096-workgroup cap
SCALE_SIZES = (1, 257, 262144 + 1)     # one element; a second workgroup; past the 1024-workgroup cap


def dgelu_table(prec):
    """Every finite value of the 16-bit type in [-12, 12] (f32: the fp16 values, widened), as a tensor of the type."""
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float16}[prec]
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)
    x = x[torch.isfinite(x.float()) & (x.float().abs() <= 12)]
    return x.float() if prec == "fp32" else x


def dgelu_inputs(n, prec, seed=0):
    """dy: N(0, 1) of the type with +0 and -0 planted; pre: the table, repeated to n elements (from a seeded offset)."""
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": f32}[prec]
    t = dgelu_table(prec)
    idx = (torch.arange(n) + 7919 * seed) % t.numel()
    dy = randn(n, seed=70 + seed).to(dt)
    dy[::5] = 0.0
    dy[2::5] = -0.0
    return dy, t[idx].contiguous()
