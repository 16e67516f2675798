"""LayerNorm backward, row scheduling: several rows per wave with the next row's loads in flight, ragged tails, waves without a
row, a grid capped by the caller's workspace, and the deterministic two-stage column sums -- against the f32 PyTorch reference
with the bounds of test_gpu_ops.test_layernorm_fwd_bwd (dx 1e-5, dx_act per precision, the three sums 2e-5 of the largest
element; the reference itself is within 4.3e-7 of f64 at these shapes, a strictly sequential f32 sum within 2.3e-6)."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECS = ["bf16", "fp16", "fp32"]
CAP_BLOCKS = 64  # the smallest workspace pm_layernorm_bwd takes as one: 64 partial-row triples


def ptol(prec, bf16, fp32):
    return {"bf16": bf16, "fp16": bf16 * 1.5 / 8, "fp32": fp32}[prec]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


@functools.lru_cache(maxsize=None)
def _k(prec):
    from ssl4polyp_amd.engine import Kernels
    return Kernels(prec)


class Case:
    """Inputs as in test_layernorm_fwd_bwd, the kernel's own forward statistics, and the reference gradients (computed once)."""

    def __init__(self, M, D, prec):
        k = _k(prec)
        self.M, self.D, self.prec, self.k = M, D, prec, k
        self.x = rnd(M, D, seed=1, scale=2.0) + 0.5
        self.gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
        y = torch.empty(M, D, dtype=k.act_dtype, device=DEV)
        self.mean, self.rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        k.layernorm_fwd(self.x, self.gamma, beta, y, self.mean, self.rstd, M, D)
        self.dy = rnd(M, D, seed=4).to(k.act_dtype)
        self.dres = rnd(M, D, seed=5)
        xr = self.x.clone().requires_grad_(True)
        gr, br = self.gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        F.layer_norm(xr, (D,), gr, br, 1e-6).backward(self.dy.float())
        self.want = (xr.grad + self.dres).detach()
        self.want_plain = xr.grad.detach()
        self.dg, self.db, self.dc = gr.grad.detach(), br.grad.detach(), self.want.sum(0)
        self.tol_act = ptol(prec, 8e-3, 2e-6)

    def outputs(self, act=True):
        M, D = self.M, self.D
        dx = torch.full((M, D), float("nan"), device=DEV)
        dx_act = torch.full((M, D), float("nan"), dtype=self.k.act_dtype, device=DEV) if act else None
        return dx, dx_act, torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)

    def call(self, dres, dx, dx_act, dg, db, dc, ws, ws_bytes, M=None):
        """pm_layernorm_bwd through the C ABI, as engine.Kernels.layernorm_bwd calls it, with the workspace given here."""
        from ssl4polyp_amd import _lib
        from ssl4polyp_amd.engine import _ptr, _stream
        D, k = self.D, self.k
        _lib.check(k.lib.pm_layernorm_bwd(_ptr(self.dy), _lib.dtype_code(self.dy.dtype), _ptr(self.x), D, _ptr(self.gamma),
                                          _ptr(self.mean), _ptr(self.rstd), _ptr(dres), D, _ptr(dx), D, _ptr(dx_act), k.act,
                                          _ptr(dg), _ptr(db), _ptr(dc), self.M if M is None else M, D, _ptr(ws), ws_bytes,
                                          _stream()), "pm_layernorm_bwd")

    def check(self, dx, dx_act, dg, db, dc):
        for name, got, want, bound in (("dx", dx, self.want, 1e-5), ("dx_act", dx_act, self.want, self.tol_act),
                                       ("dgamma", dg, self.dg, 2e-5), ("dbeta", db, self.db, 2e-5), ("dcolsum", dc, self.dc, 2e-5)):
            if got is None:
                continue
            err = rel(got.float(), want)
            print(f"{name} M={self.M} D={self.D} {self.prec}: {err:.3e} (bound {bound:.1e})")
            assert err < bound, name


@functools.lru_cache(maxsize=None)
def case(M, D, prec):
    return Case(M, D, prec)


def capped_ws(D):
    return torch.empty(CAP_BLOCKS * 3 * D, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------
# several rows per wave, a ragged tail, waves without any row, every count of f32x4 slots per lane (3, 2, 5, 4)
@pytest.mark.parametrize("M,D", [(5, 768), (4099, 768), (777, 512), (300, 1280), (3001, 1024)])
@pytest.mark.parametrize("prec", PRECS)
def test_default_workspace_shapes(M, D, prec):
    c = case(M, D, prec)
    dx, dx_act, dg, db, dc = c.outputs()
    c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, c.dres, dx, dx_act, dg, db, dc, M, D)
    c.check(dx, dx_act, dg, db, dc)


@pytest.mark.parametrize("prec", PRECS)
def test_capped_grid(prec):
    """A workspace of exactly 64 partial-row triples: 256 waves cover 1000 rows, about four rows per wave with a ragged tail."""
    c = case(1000, 768, prec)
    ws = capped_ws(c.D)
    dx, dx_act, dg, db, dc = c.outputs()
    c.call(c.dres, dx, dx_act, dg, db, dc, ws, ws.numel() * 4)
    c.check(dx, dx_act, dg, db, dc)


@pytest.mark.parametrize("prec", PRECS)
def test_row_locality(prec):
    """A row's dx does not depend on which wave handled it, nor on the rows around it."""
    c = case(1000, 768, prec)
    ws = capped_ws(c.D)
    dx, dx_act, dg, db, dc = c.outputs()
    c.call(c.dres, dx, dx_act, dg, db, dc, ws, ws.numel() * 4)
    dx2, dx_act2, dg2, db2, dc2 = c.outputs()
    c.call(c.dres, dx2, dx_act2, dg2, db2, dc2, ws, ws.numel() * 4, M=37)
    assert torch.equal(dx[:37], dx2[:37]) and torch.equal(dx_act[:37], dx_act2[:37])
    assert torch.isnan(dx2[37:]).all() and torch.isnan(dx_act2[37:].float()).all()  # and nothing past the rows asked for


@pytest.mark.parametrize("capped", [False, True])
def test_determinism(capped):
    c = case(4099, 768, "bf16")
    runs = []
    for _ in range(2):
        dx, dx_act, dg, db, dc = c.outputs()
        if capped:
            ws = capped_ws(c.D)
            c.call(c.dres, dx, dx_act, dg, db, dc, ws, ws.numel() * 4)
        else:
            c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, c.dres, dx, dx_act, dg, db, dc, c.M, c.D)
        runs.append((dg, db, dc))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prec", PRECS)
def test_accumulation(prec):
    """The sums add into what dgamma / dbeta / dcolsum held."""
    c = case(1000, 768, prec)
    dx, dx_act, _, _, _ = c.outputs()
    init = [rnd(c.D, seed=20 + i, scale=3.0) for i in range(3)]
    dg, db, dc = (t.clone() for t in init)
    c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, c.dres, dx, dx_act, dg, db, dc, c.M, c.D)
    for got, start, want in zip((dg, db, dc), init, (c.dg, c.db, c.dc)):
        assert not torch.equal(got, start)
        assert rel(got, start + want) < 2e-5


@pytest.mark.parametrize("present", [p for p in itertools.product([False, True], repeat=3) if not all(p)])
def test_optional_pointers(present):
    """Every combination of NULL sum pointers (all three NULL included), without dx_act."""
    c = case(1000, 768, "bf16")
    dx, _, dg, db, dc = c.outputs(act=False)
    dg, db, dc = (t if p else None for t, p in zip((dg, db, dc), present))
    c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, c.dres, dx, None, dg, db, dc, c.M, c.D)
    c.check(dx, None, dg, db, dc)


@pytest.mark.parametrize("prec", PRECS)
def test_in_place_residual(prec):
    """dres aliases dx row for row, with and without the sums (the prefetched row is never the row being stored)."""
    c = case(4099, 768, prec)
    _, dx_act, dg, db, dc = c.outputs()
    dx = c.dres.clone()
    c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, dx, dx, dx_act, dg, db, dc, c.M, c.D)
    c.check(dx, dx_act, dg, db, dc)
    dx = c.dres.clone()
    c.k.layernorm_bwd(c.dy, c.x, c.gamma, c.mean, c.rstd, dx, dx, None, None, None, None, c.M, c.D)
    c.check(dx, None, None, None, None)


@pytest.mark.parametrize("prec", PRECS)
def test_no_workspace(prec):
    """Without a workspace the column sums go through one atomic per column per workgroup: same bounds, no residual here."""
    c = case(4099, 768, prec)
    dx, dx_act, dg, db, dc = c.outputs()
    c.call(None, dx, dx_act, dg, db, dc, None, 0)
    assert rel(dx, c.want_plain) < 1e-5
    assert rel(dx_act.float(), c.want_plain) < c.tol_act
    assert rel(dg, c.dg) < 2e-5
    assert rel(db, c.db) < 2e-5
    assert rel(dc, c.want_plain.sum(0)) < 2e-5
